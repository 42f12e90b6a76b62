"""The AlexNet LPIPS loss (transeditor_amd.lpips_alex.AlexLPIPSLoss) and the loss of encoder training (transeditor_amd.encoder_loss) on
the CPU: the host's chaining of the forward and backward kernels, with the `_lib` bindings replaced by torch restatements of their
contracts in fp64 (the convention of test_id_loss_cpu.py), against torch autograd of the restated formula; the stem weight's layout;
the golden file against the restatement; the refusals and their messages; EncoderLoss against the formulas of calc_loss with stub
losses.  The kernels themselves are tested on the GPU (test_gpu_lpips_alex_loss.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import id_loss_restated as IR
import lpips_alex_loss_restated as LR
import lpips_alex_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 24, 16, 16)


@pytest.fixture
def emulated(monkeypatch):
    """every binding the loss calls, restated in fp64 on the CPU.  The data gradients are restated from the PREPARED weights, so a wrong
    layout on the host shows in the gradient"""
    from transeditor_amd import _lib
    d = torch.float64

    def conv2d(x, w, bias, stride=1, pad=(0, 0), act=0, out=None, c0=0):
        assert act == 1 and out is None
        return F.relu(F.conv2d(x.to(d), w.to(d), bias.to(d), stride, pad))

    def pool3(x, mode, out=None, c0=0):
        assert mode == _lib.POOL3_MAX_S2 and out is None
        return F.max_pool2d(x, 3, 2)

    def head_fwd(f, t_hat, w):
        return (((LR.normalize(f) - t_hat) ** 2) * w.to(d).view(1, -1, 1, 1)).sum(1).flatten(1).sum(1, keepdim=True)

    def conv2d_dgrad(g, wt, x_shape, kernel, stride=1, pad=(0, 0), pre=None, slope=None, in_scale=None, add=None, add_stride=1):
        assert pre is None and slope is None and in_scale is None and add is None and g.is_contiguous()
        assert tuple(g.shape[2:]) == _lib.conv2d_out_hw(x_shape[2], x_shape[3], *kernel, stride, pad)
        return IR.dgrad_acc_from_layout(g.to(d), wt, x_shape, kernel, stride, pad)

    def stem_dgrad(g, wt, img_shape):
        assert tuple(g.shape[2:]) == _lib.conv2d_out_hw(img_shape[2], img_shape[3], 11, 11, 4, (2, 2))
        return LR.stem_dgrad(g, LR.stem_weight_from_layout(wt, g.shape[1]), img_shape[2:])

    for name, fn in dict(
            alex_stem_fwd=lambda img, w, b: F.relu(F.conv2d(LR.scale(img, d), w.to(d), b.to(d), 4, 2)), pool3=pool3, conv2d=conv2d,
            lpips_normalize=LR.normalize, lpips_head_fwd=head_fwd,
            lpips_dist=lambda partials, hws: sum(p.sum(1) / hw for p, hw in zip(partials, hws)),
            lpips_head_bwd=LR.head_bwd, conv2d_dgrad=conv2d_dgrad, pool3s2_max_bwd=LR.pool3s2_max_bwd, alex_stem_dgrad=stem_dgrad).items():
        assert hasattr(_lib, name), name
        monkeypatch.setattr(_lib, name, fn)


@pytest.mark.parametrize('H,W', [(31, 31), (45, 39)])
def test_value_and_gradient_through_the_hosts_chaining(emulated, H, W):
    """the loss and d loss / d x of the one autograd.Function against torch autograd of the restated formula in fp64, to 1e-10 of the
    largest element: five heads, four data gradients, both pools (at 45x39 with an unreached edge in front of each) and the stem"""
    from transeditor_amd import lpips_alex
    sd, lin = R.state_dict(3, WIDTHS), LR.lin_state_dict(4, WIDTHS)
    mod = lpips_alex.AlexLPIPSLoss(state_dict=sd, lin_state_dict=lin).cpu().double()
    assert mod.widths == WIDTHS and not list(mod.parameters())
    x, y = R.images(5, 2, H, W), R.images(6, 2, H, W)
    want_v, want_g = LR.value_and_grad(x, y, sd, lin, torch.float64)
    xin, yin = x.double().requires_grad_(True), y.double().requires_grad_(True)
    v = lpips_alex._Loss.apply(xin, mod, yin)
    assert v.ndim == 0 and abs(float(v.detach()) - float(want_v)) <= 1e-12 * float(want_v) and float(want_v) > 1e-3
    (3 * v).backward()
    assert yin.grad is None                                                     # the gradient goes to x only
    scale = float(want_g.abs().max())
    err = float((xin.grad / 3 - want_g).abs().max()) / scale
    print(f'AlexLPIPSLoss {H}x{W}: max |grad - autograd| / max |autograd| = {err:.2e}')
    assert scale > 1e-6 and err <= 1e-10
    with pytest.raises(RuntimeError, match='second time'):
        v.backward()


def test_stem_weight_layout_and_its_adjoint():
    """_lib.alex_stem_dgrad_weight: 363 Co floats, every tap in exactly one row phase, read back as te_hip.h words it; the restated
    gradient built on it is the adjoint of the forward stem: <conv(s(x)) - conv(s(0)), g> = <x, dgrad(g)>"""
    from transeditor_amd import _lib
    g = torch.Generator().manual_seed(7)
    w = torch.randn(5, 3, 11, 11, generator=g, dtype=torch.float64)
    wt = _lib.alex_stem_dgrad_weight(w)
    assert wt.shape == (363 * 5,) and wt.is_contiguous() and _lib.ALEX_STEM_ROW_TAPS == (2, 3, 0, 1)
    assert torch.equal(LR.stem_weight_from_layout(wt, 5), w)
    assert torch.equal(wt[:5 * 99].view(5, 3, 11, 3)[2, 1, 4, 0], w[2, 0, 6, 4])          # ry = 0: rows 2, 6, 10
    with pytest.raises(RuntimeError, match=r'\[Co,3,11,11\]'):
        _lib.alex_stem_dgrad_weight(w[:, :, :7, :7])
    for H, W in [(30, 33), (11, 13)]:
        x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
        Ho, Wo = _lib.conv2d_out_hw(H, W, 11, 11, 4, (2, 2))
        gr = torch.randn(2, 5, Ho, Wo, generator=g, dtype=torch.float64)
        got = LR.stem_dgrad(gr, w, (H, W))
        fwd = lambda t: F.conv2d(LR.scale(t, torch.float64), w, None, 4, 2)
        lhs, rhs = float(((fwd(x) - fwd(torch.zeros_like(x))) * gr).sum()), float((x * got).sum())
        assert abs(lhs - rhs) <= 1e-10 * (abs(lhs) + 1)
        if H == 30:
            assert bool((got[:, :, 29] == 0).all()) and bool((got[:, :, 28] != 0).all())  # row 29 of 30: no window reaches it


def test_golden_file_matches_the_restatement():
    """what the reference's own class returned (tools/lpips_alex_loss_golden.py) against the restatement the GPU tests measure with"""
    G = LR.GOLDEN
    ref = np.load(os.path.join(ROOT, 'tests', 'golden', 'lpips_alex_loss_ref.npz'))
    assert all(int(ref[k]) == v for k, v in G.items())
    lin = {f'lin{l}.model.1.weight': torch.from_numpy(ref[f'lin{l}']).view(1, -1, 1, 1) for l in range(5)}
    assert [ref[f'lin{l}'].size for l in range(5)] == list(R.WIDTHS) and all(ref[f'lin{l}'].dtype == np.float32 for l in range(5))
    sd = R.state_dict(G['seed'])
    x, y = torch.from_numpy(ref['x']), torch.from_numpy(ref['y'])
    for t, seed in ((x, G['x_seed']), (y, G['y_seed'])):                        # the seeded images, to the last bits of this CPU's fp32 tanh
        assert t.dtype == torch.float32 and float((t - R.images(seed, G['B'], G['S'])).abs().max()) <= 2.0 ** -22
    v64, g64 = LR.value_and_grad(x, y, sd, lin, torch.float64)
    assert ref['g64'].dtype == np.float64 and ref['g_ref'].dtype == np.float32 and ref['g64'].shape == tuple(x.shape)
    assert abs(float(v64) - float(ref['v64'])) <= 1e-13 * float(v64)
    assert R.rel_l2(g64, torch.from_numpy(ref['g64'])) <= 1e-13
    yard_v = abs(float(ref['v_ref']) - float(ref['v64'])) / float(ref['v64'])
    yard_g = R.rel_l2(torch.from_numpy(ref['g_ref']), torch.from_numpy(ref['g64']))
    print(f"golden: value {float(ref['v64']):.9f}; the reference in fp32 against fp64: value {yard_v:.3e}, gradient rel_l2 {yard_g:.3e}")
    assert yard_v <= 2.0 ** -20 and yard_g <= 1e-5 and float(ref['v64']) > 0.01
    assert LR.zero_pixels(x, sd) == [0] * 5                                     # te_lpips_head_bwd_f32's NaN deviation is not exercised


def test_state_dict_refusals():
    from transeditor_amd.lpips_alex import AlexLPIPSLoss
    sd, lin = R.state_dict(3, WIDTHS), LR.lin_state_dict(4, WIDTHS)
    renamed = {k.replace('lin', '').replace('model.', ''): v for k, v in lin.items()}
    assert set(renamed) == {f'{l}.1.weight' for l in range(5)}
    a, b = AlexLPIPSLoss(state_dict=sd, lin_state_dict=lin), AlexLPIPSLoss(state_dict=sd, lin_state_dict=renamed)
    assert all(torch.equal(a._lin(l), b._lin(l)) and a._lin(l).shape == (WIDTHS[l],) for l in range(5))
    assert set(a.state_dict()) == {f'{n}{l}' for n in ('w', 'b', 'lin') for l in range(5)}          # the prepared weights are derived
    assert a.wt0.shape == (363 * WIDTHS[0],) and a.wt1.numel() == a.w1.numel() and not a.training
    with pytest.raises(ValueError, match=r'AlexLPIPSLoss: lin_state_dict has no lin3.model.1.weight \(not an LPIPS v0.1 alex head file'):
        AlexLPIPSLoss(state_dict=sd, lin_state_dict={k: v for k, v in lin.items() if not k.startswith('lin3')})
    with pytest.raises(ValueError, match=r'AlexLPIPSLoss: lin1.model.1.weight is \(16,\), expected \(1, None, 1, 1\)'):
        AlexLPIPSLoss(state_dict=sd, lin_state_dict={**lin, 'lin1.model.1.weight': torch.zeros(16)})
    with pytest.raises(ValueError, match='AlexLPIPSLoss: lin2.model.1.weight has 16 channels, but its tap features.6 has 24'):
        AlexLPIPSLoss(state_dict=sd, lin_state_dict={**lin, 'lin2.model.1.weight': torch.zeros(1, 16, 1, 1)})
    with pytest.raises(ValueError, match=r'AlexLPIPSLoss: state_dict has no features.8.weight / features.8.bias \(not a torchvision alexnet'):
        AlexLPIPSLoss(state_dict={k: v for k, v in sd.items() if k != 'features.8.bias'}, lin_state_dict=lin)
    with pytest.raises(ValueError, match='AlexLPIPSLoss: features.3.weight is'):
        AlexLPIPSLoss(state_dict={**sd, 'features.3.weight': torch.zeros(16, 8, 3, 3)}, lin_state_dict=lin)
    with pytest.raises(ValueError, match='give alexnet_path or state_dict, not both'):
        AlexLPIPSLoss('alexnet.pth', state_dict=sd, lin_state_dict=lin)
    with pytest.raises(FileNotFoundError, match='AlexLPIPSLoss: LPIPS v0.1 alex head'):
        AlexLPIPSLoss(state_dict=sd, lin_path='/nonexistent/alex.pth')
    with pytest.raises(FileNotFoundError, match='nothing is downloaded'):
        AlexLPIPSLoss('/nonexistent/alexnet.pth', lin_state_dict=lin)


def test_input_refusals():
    from transeditor_amd.lpips_alex import AlexLPIPSLoss
    mod = AlexLPIPSLoss(state_dict=R.state_dict(3, WIDTHS), lin_state_dict=LR.lin_state_dict(4, WIDTHS))
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(ValueError, match=r'30x40 images leave a 2x4 plane in front of the max pool of features.5, which needs 3x3: H and W must be at least 31'):
        mod(z(2, 3, 30, 40), z(2, 3, 30, 40))
    with pytest.raises(ValueError, match=r'40x14 images leave a 9x2 plane in front of the max pool of features.2'):
        mod(z(2, 3, 40, 14), z(2, 3, 40, 14))
    with pytest.raises(ValueError, match=r'5x64 images leave a 0x15 plane'):
        mod(z(1, 3, 5, 64), z(1, 3, 5, 64))
    with pytest.raises(ValueError, match=r'expected \[B,3,H,W\] images'):
        mod(z(2, 1, 64, 64), z(2, 1, 64, 64))
    with pytest.raises(ValueError, match='one shape'):
        mod(z(2, 3, 64, 64), z(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match='AlexLPIPS needs a GPU'):
        mod(torch.zeros(2, 3, 31, 31), torch.zeros(2, 3, 31, 31))


# ---------------------------------------------------------------------------------------------------------------- EncoderLoss
class _StubID(torch.nn.Module):
    def forward(self, y_hat, y, x):
        self.args = (y_hat, y, x)
        loss = ((y_hat - y) ** 2).sum() * 0.01
        return loss, 0.25, [{'diff_target': 0.5, 'diff_input': 0.5, 'diff_views': 0.25}] * y_hat.shape[0]


class _StubLPIPS(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.shapes = []

    def forward(self, x, y):
        self.shapes.append((tuple(x.shape), tuple(y.shape)))
        return (x - y).abs().mean() * 2


def test_encoder_loss_terms_keys_and_crop():
    from transeditor_amd.encoder_loss import CROP, EncoderLoss, w_norm
    g = torch.Generator().manual_seed(3)
    real, inv = torch.rand(2, 3, 256, 256, generator=g, dtype=torch.float64), torch.rand(2, 3, 256, 256, generator=g, dtype=torch.float64)
    z, p = torch.randn(2, 16, 32, generator=g, dtype=torch.float64), torch.randn(2, 16, 32, generator=g, dtype=torch.float64)
    za, pa = torch.randn(16, 32, generator=g, dtype=torch.float64), torch.randn(16, 32, generator=g, dtype=torch.float64)
    assert CROP == (35, 223, 32, 220)
    cr = lambda t: t[:, :, 35:223, 32:220]
    # the reference's defaults: id, l2, lpips in this order
    ids, lp = _StubID(), _StubLPIPS()
    crit = EncoderLoss(id_loss=ids, lpips_loss=lp)
    assert (crit.id_lambda, crit.l2_lambda, crit.lpips_lambda, crit.lpips_lambda_crop, crit.l2_lambda_crop, crit.w_norm_lambda) == (0.1, 1.0, 0.8, 0, 0, 0)
    x = inv.clone().requires_grad_(True)
    loss, d, logs = crit(real, x, z, p)
    assert ids.args[0] is x and ids.args[1] is real and ids.args[2] is real      # id_loss(inversed, real, real)
    want = ((inv - real) ** 2).sum() * 0.01 * 0.1 + F.mse_loss(inv, real) * 1.0 + (inv - real).abs().mean() * 2 * 0.8
    assert list(d) == ['loss_id', 'id_improve', 'loss_l2', 'loss_lpips', 'loss'] and len(logs) == 2 and d['id_improve'] == 0.25
    assert abs(float(loss.detach()) - float(want)) <= 1e-12 and d['loss'] == float(loss.detach()) and all(isinstance(v, float) for v in d.values())
    assert abs(d['loss_l2'] - float(F.mse_loss(inv, real))) <= 1e-15 and lp.shapes == [((2, 3, 256, 256),) * 2]
    loss.backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    # every term, with the latent averages
    lp = _StubLPIPS()
    crit = EncoderLoss(id_loss=ids, lpips_loss=lp, id_lambda=0.2, l2_lambda=0.5, lpips_lambda=0.3, lpips_lambda_crop=0.6, l2_lambda_crop=0.7,
                       w_norm_lambda=0.005, start_from_latent_avg=True)
    loss, d, logs = crit(real, inv, z, p, za, pa)
    wn = lambda t, a: torch.sum((t - a).norm(2, dim=(1, 2))) / t.shape[0]
    want = (((inv - real) ** 2).sum() * 0.01 * 0.2 + F.mse_loss(inv, real) * 0.5 + (inv - real).abs().mean() * 2 * 0.3
            + (cr(inv) - cr(real)).abs().mean() * 2 * 0.6 + F.mse_loss(cr(inv), cr(real)) * 0.7 + (wn(z, za) + wn(p, pa)) * 0.005)
    assert list(d) == ['loss_id', 'id_improve', 'loss_l2', 'loss_lpips', 'loss_lpips_crop', 'loss_l2_crop', 'loss_w_norm', 'loss']
    assert abs(float(loss) - float(want)) <= 1e-12 and lp.shapes == [((2, 3, 256, 256),) * 2, ((2, 3, 188, 188),) * 2]
    assert abs(d['loss_w_norm'] - float(wn(z, za) + wn(p, pa))) <= 1e-12 and abs(d['loss_l2_crop'] - float(F.mse_loss(cr(inv), cr(real)))) <= 1e-15
    assert abs(float(w_norm(z)) - float(z.norm(2, dim=(1, 2)).mean())) <= 1e-12
    # terms that are switched off are not computed; nothing at all gives the float 0.0 of calc_loss
    crit = EncoderLoss(id_lambda=0, l2_lambda=0, lpips_lambda=0, w_norm_lambda=1.0)
    loss, d, logs = crit(real, inv, z, p)
    assert logs is None and list(d) == ['loss_w_norm', 'loss'] and abs(float(loss) - float(wn(z, 0) + wn(p, 0))) <= 1e-12
    loss, d, logs = EncoderLoss(id_lambda=0, l2_lambda=0, lpips_lambda=0)(real, inv, z, p)
    assert loss == 0.0 and d == {'loss': 0.0} and logs is None


def test_encoder_loss_refusals():
    from transeditor_amd.encoder_loss import EncoderLoss
    with pytest.raises(ValueError, match='id_lambda = 0.1 needs id_loss'):
        EncoderLoss(lpips_loss=_StubLPIPS())
    with pytest.raises(ValueError, match='lpips_lambda = 0.8 needs lpips_loss'):
        EncoderLoss(id_loss=_StubID())
    with pytest.raises(ValueError, match='lpips_lambda_crop = 0.5 needs lpips_loss'):
        EncoderLoss(id_loss=_StubID(), lpips_lambda=0, lpips_lambda_crop=0.5)
    crit = EncoderLoss(id_lambda=0, lpips_lambda=0, w_norm_lambda=1.0, start_from_latent_avg=True)
    with pytest.raises(ValueError, match='needs the latent averages'):
        crit(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4))


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_entry_points_and_the_build():
    """the two entry points are declared, bound and exported by the library built from csrc/lpips_alex_bwd.hip; their argument checks
    run on the host and launch nothing"""
    from transeditor_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    names = ('te_pool3s2_max_bwd_f32', 'te_alex_stem_dgrad_f32')
    for name in names:
        assert name in _lib.EXPORTS and header.count(name + '(') == 1           # declared once
    assert 'M8b' in header and 'lpips.py:29-35' in header
    assert 'lpips_alex_bwd.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'lpips_alex_bwd.hip'))
    build.build()                                                               # (a no-op when the library is up to date)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16                   # validation only: never dereferenced
    pool, stem = L.te_pool3s2_max_bwd_f32, L.te_alex_stem_dgrad_f32
    assert pool(None, p, p, 4, 7, 7, None) == -1 and pool(p, None, p, 4, 7, 7, None) == -1 and pool(p, p, None, 4, 7, 7, None) == -1
    assert b'NULL' in L.te_last_error_string()
    for planes, H, W in [(0, 7, 7), (-1, 7, 7), (4, 2, 7), (4, 7, 2), (4, 0, 7), (4, 7, -3), (1, 65536, 65536), (1 << 40, 64, 64)]:
        assert pool(p, p, p, planes, H, W, None) == -2, (planes, H, W)
    assert pool(p, p, p, 4, 2, 7, None) == -2 and b'3 x 3 window does not fit a 2 x 7 plane' in L.te_last_error_string()
    assert stem(None, p, p, 1, 40, 40, 8, None) == -1 and stem(p, None, p, 1, 40, 40, 8, None) == -1 and stem(p, p, None, 1, 40, 40, 8, None) == -1
    for N, H, W, Co in [(0, 40, 40, 8), (-1, 40, 40, 8), (65536, 40, 40, 8), (1, 0, 40, 8), (1, 40, -1, 8), (1, 6, 40, 8), (1, 40, 6, 8),
                        (1, 32768, 32768, 8), (1, 40, 40, 0), (1, 40, 40, -3), (1, 4096, 4096, 4096)]:
        assert stem(p, p, p, N, H, W, Co, None) == -2, (N, H, W, Co)
    assert stem(p, p, p, 1, 6, 40, 8, None) == -2 and b'11 x 11 kernel with padding 2 does not fit a 6 x 40 image' in L.te_last_error_string()

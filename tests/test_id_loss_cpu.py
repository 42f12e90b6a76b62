"""The identity loss (transeditor_amd.id_loss, ArcFaceID.embed_grad, irse_units.unit_backward) on the CPU: the host's chaining of the
backward kernels, with the `_lib` bindings replaced by torch restatements of their contracts in fp64 (the convention of
test_closed_families_cpu.py); the host's phase split and flipped layout of a data gradient's weight against F.conv_transpose2d; the
messages.  The kernels themselves are tested on the GPU (test_gpu_id_loss.py)."""
import os

import pytest
import torch
import torch.nn.functional as F

import arcface_restated as R
import id_loss_restated as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, BOX, POOL, DIM = 32, (3, 29, 2, 30), 11, 24
# one unit of stride 2 with a convolution shortcut in each; the MaxPool2d(1, 2) shortcut and the plain one beside it.  11 -> 6 -> 3 / 6:
# an odd and an even plane in front of a stride-2 layer
NETS = {'conv-sc+plain': [(8, 16, 2), (16, 16, 1)], 'pool-sc+conv-sc': [(8, 8, 2), (8, 16, 2)]}


@pytest.fixture
def emulated(monkeypatch):
    """every binding the differentiable chain calls, restated in fp64 on the CPU.  The data gradient is restated from the PREPARED weight
    (IR.dgrad_acc_from_layout), so a wrong phase split or flip on the host shows in the gradient"""
    from transeditor_amd import _lib
    d = torch.float64

    def prelu(t, slope):
        return torch.where(t > 0, t, t * slope.to(d).view(1, -1, 1, 1))

    def conv2d_prelu_keep(x, w, bias, slope, in_scale=None, in_shift=None, stride=1, pad=(0, 0)):
        v = x.to(d)
        if in_scale is not None:
            v = v * in_scale.to(d).view(1, -1, 1, 1) + in_shift.to(d).view(1, -1, 1, 1)
        pre = F.conv2d(F.pad(v, (pad[1], pad[1], pad[0], pad[0])), w.to(d), bias.to(d), stride)
        return prelu(pre, slope), pre

    def id_stem_keep(img, w, b, slope, box, pool):
        y0, y1, x0, x1 = box
        pre = F.conv2d(F.adaptive_avg_pool2d(img.to(d)[:, :, y0:y1, x0:x1], (pool, pool)), w.to(d), b.to(d), 1, 1)
        return prelu(pre, slope), pre

    def conv2d(x, w, bias, stride=1, pad=(0, 0), act=0, out=None, c0=0):
        assert act == 0 and out is None
        return F.conv2d(x.to(d), w.to(d), bias.to(d), stride, pad)

    def conv2d_dgrad(g, wt, x_shape, kernel, stride=1, pad=(0, 0), pre=None, slope=None, in_scale=None, add=None, add_stride=1):
        assert g.is_contiguous() and tuple(g.shape[2:]) == _lib.conv2d_out_hw(x_shape[2], x_shape[3], *kernel, stride, pad)
        return IR.dgrad_epilogue(IR.dgrad_acc_from_layout(g.to(d), wt, x_shape, kernel, stride, pad), pre, slope, in_scale, add, add_stride)

    def id_stem_bwd(g, wt, pre, slope, img_shape, box, pool):
        gp = IR.dgrad_acc_from_layout(IR.dgrad_epilogue(g.to(d), pre, slope), wt, (g.shape[0], 3, pool, pool), (3, 3), 1, (1, 1))
        img = torch.zeros(img_shape, dtype=d, requires_grad=True)
        y0, y1, x0, x1 = box
        with torch.enable_grad():
            return torch.autograd.grad(F.adaptive_avg_pool2d(img[:, :, y0:y1, x0:x1], (pool, pool)), img, gp)[0]

    for name, fn in dict(
            conv2d_prelu_keep=conv2d_prelu_keep, id_stem_keep=id_stem_keep, conv2d=conv2d, conv2d_dgrad=conv2d_dgrad, id_stem_bwd=id_stem_bwd,
            adaptive_avgpool=lambda x, OH=7, OW=7: F.adaptive_avg_pool2d(x.to(d), (OH, OW)),
            se_excite=lambda p, w1, w2: torch.sigmoid(F.relu(p.to(d) @ w1.to(d).t()) @ w2.to(d).t()),
            se_scale_add=lambda res, gate, sc, stride=1: (res if gate is None else res * gate[:, :, None, None]) + sc[:, :, ::stride, ::stride],
            fc_stream=lambda a, w, bias, act=0: a.to(d) @ w.to(d).t() + bias.to(d),
            rows_unit=lambda a: a / a.norm(dim=1, keepdim=True), rows_dot=lambda a, b: (a.to(d) * b.to(d)).sum(1),
            se_bwd=IR.se_bwd, rows_unit_bwd=IR.rows_unit_bwd).items():
        assert hasattr(_lib, name), name
        monkeypatch.setattr(_lib, name, fn)


def _net64(sd, units):
    """IDLoss whose buffers are the fp64 folded values (before their one rounding): what the restatement computes with"""
    from transeditor_amd import arcface, id_loss
    from transeditor_amd.irse_units import register_units
    loss = id_loss.IDLoss(state_dict=sd, box=BOX, pool=POOL, units=units)
    net, p64 = loss.facenet, arcface.parse_state_dict(sd, units=units, pool=POOL, dtype=torch.float64)
    for name, t in zip(('stem_w', 'stem_b', 'stem_slope', 'fc_w', 'fc_b'), (*p64['stem'], *p64['fc'])):
        net.register_buffer(name, t)
    register_units(net, p64['units'])
    return loss


@pytest.mark.parametrize('which', list(NETS))
def test_gradient_through_the_hosts_chaining(emulated, monkeypatch, which):
    """d loss / d y_hat of IDLoss and d <e, c> / d images of embed_grad against torch autograd of the restated network in fp64, to 1e-10
    (relative to the largest element): stem, both shortcut kinds, a gate, stride 2 on an odd and an even plane, the Linear and the norm"""
    from transeditor_amd import arcface
    units = NETS[which]
    B = 3
    y_hat, y, x = (R.images(s, B, S) for s in (5, 6, 7))
    sd = R.state_dict(4, units=units, images=y_hat, box=BOX, pool=POOL, dim=DIM, reduction=4)
    loss_mod = _net64(sd, units)
    # the device check is the one thing of embed / embed_grad that cannot run here
    monkeypatch.setattr(arcface.ArcFaceID, 'embed_grad', lambda self, im: arcface._Embed.apply(im.double(), self))
    monkeypatch.setattr(arcface.ArcFaceID, 'embed', lambda self, im: arcface._Embed.apply(im.detach().double(), self).detach())
    gates, pres = [], []
    want_loss, want_sim, want_logs, want_grad = IR.id_loss(y_hat, y, x, sd, torch.float64, units, BOX, POOL, gates, pres)
    assert float(torch.cat(gates).detach().min()) < 0.2 and float(torch.cat(gates).detach().max()) > 0.8 and float(want_loss) > 0.1
    assert 0.2 < float((torch.cat(pres) > 0).double().mean()) < 0.8
    yh, yy, xx = y_hat.double().requires_grad_(True), y.double().requires_grad_(True), x.double().requires_grad_(True)
    loss, sim, logs = loss_mod(yh, yy, xx)
    assert loss.ndim == 0 and isinstance(sim, float) and len(logs) == B and set(logs[0]) == {'diff_target', 'diff_input', 'diff_views'}
    assert abs(float(loss) - float(want_loss)) <= 1e-10 and abs(sim - want_sim) <= 1e-10
    assert all(abs(a[k] - b[k]) <= 1e-10 for a, b in zip(logs, want_logs) for k in a)
    loss.backward()
    assert yy.grad is None and xx.grad is None                                  # the gradient goes to y_hat only
    scale = float(want_grad.abs().max())
    assert scale > 1e-4
    err = float((yh.grad - want_grad).abs().max()) / scale
    print(f'IDLoss {which}: max |grad - autograd| / max |autograd| = {err:.2e}')
    assert err <= 1e-10
    y0, y1, x0, x1 = BOX
    outside = torch.ones(S, S, dtype=torch.bool)
    outside[y0:y1, x0:x1] = False
    assert bool((yh.grad[:, :, outside] == 0).all()) and bool((yh.grad[:, :, ~outside] != 0).all())
    # embed_grad alone, against a fixed cotangent
    c = torch.randn(B, DIM, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    im = y_hat.double().requires_grad_(True)
    e = loss_mod.facenet.embed_grad(im)
    (e * c).sum().backward()
    ref_in = y_hat.double().requires_grad_(True)
    e64 = IR.embed(ref_in, sd, torch.float64, units, BOX, POOL)
    assert float((e.detach() - e64.detach()).abs().max()) <= 1e-12
    want, = torch.autograd.grad((e64 * c).sum(), ref_in)
    assert float((im.grad - want).abs().max()) <= 1e-10 * float(want.abs().max())


# (Ci, Co, H, W, k, stride, pad): 3x3 and 1x1 at both strides on odd, even and non-square planes, and what the loop takes for free
LAYOUT_CASES = [(5, 4, 9, 9, 3, 2, 1), (5, 4, 8, 8, 3, 2, 1), (3, 6, 7, 10, 3, 2, 1), (4, 4, 6, 6, 3, 1, 1), (4, 6, 9, 9, 1, 2, 0), (4, 6, 8, 7, 1, 1, 0),
                (3, 2, 11, 8, 7, 2, 3), (3, 2, 9, 9, 5, 2, 2), (2, 3, 10, 9, 3, 2, 0), (2, 3, 1, 1, 3, 2, 1)]


@pytest.mark.parametrize('Ci,Co,H,W,k,s,p', LAYOUT_CASES)
def test_phase_split_and_flipped_layout(Ci, Co, H, W, k, s, p):
    """_lib.dgrad_weight: the phases, read back as te_hip.h words them, give F.conv_transpose2d of the forward's own weight in fp64"""
    from transeditor_amd import _lib
    g = torch.Generator().manual_seed(H * 100 + W * 10 + k + s)
    w = torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64)
    Ho, Wo = _lib.conv2d_out_hw(H, W, k, k, s, (p, p))
    gr = torch.randn(2, Co, Ho, Wo, generator=g, dtype=torch.float64)
    wt = _lib.dgrad_weight(w, s, (p, p))
    ny, nx = (sum(n for _, n in _lib.dgrad_phases(k, s, p)),) * 2
    assert wt.ndim == 1 and wt.is_contiguous() and wt.numel() == Ci * Co * ny * nx == w.numel()        # every tap lands in exactly one phase
    if s == 1:
        assert torch.equal(wt.view(Ci, Co * k * k), w.flip(2, 3).transpose(0, 1).reshape(Ci, -1))
    if (k, s, p) == (3, 2, 1):
        assert _lib.dgrad_phases(3, 2, 1) == [(1, 1), (0, 2)]                   # even rows: the middle tap; odd rows: the outer two
    got = IR.dgrad_acc_from_layout(gr, wt, (2, Ci, H, W), (k, k), s, (p, p))
    want = IR.dgrad_acc(gr, w, (H, W), s, (p, p))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max() + 1)
    # ... which is the adjoint of the forward: <conv(x), g> = <x, dgrad(g)>
    x = torch.randn(2, Ci, H, W, generator=g, dtype=torch.float64)
    lhs, rhs = float((F.conv2d(x, w, None, s, p) * gr).sum()), float((x * got).sum())
    assert abs(lhs - rhs) <= 1e-10 * (abs(lhs) + 1)


def test_messages_without_a_gpu():
    from transeditor_amd import arcface, id_loss
    units = NETS['conv-sc+plain']
    x = R.images(5, 2, S)
    sd = R.state_dict(4, units=units, box=BOX, pool=POOL, dim=DIM, reduction=4)
    mod = id_loss.IDLoss(state_dict=sd, box=BOX, pool=POOL, units=units)
    assert isinstance(mod.facenet, arcface.ArcFaceID) and not list(mod.parameters())
    with pytest.raises(ValueError, match='one shape'):
        mod(x, x[:1], x)
    with pytest.raises(ValueError, match=r'\[B,3,S,S\]'):
        mod.facenet.embed_grad(x[:, :1])
    with pytest.raises(ValueError, match='does not lie inside'):
        mod.facenet.embed_grad(x[:, :, :24, :24])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='ArcFaceID needs a GPU'):
            mod.facenet.embed_grad(x.requires_grad_(True))
        with pytest.raises(RuntimeError, match='ArcFaceID needs a GPU'):
            mod(x, x, x)


def test_abi_entry_points_and_the_build():
    """the six entry points are declared, bound and exported by the library built from csrc/irse_bwd.hip and csrc/irse.hip; their
    argument checks run on the host"""
    import ctypes
    from transeditor_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    names = ('te_conv2d_prelu_keep_f32', 'te_id_stem_keep_f32', 'te_conv2d_dgrad_f32', 'te_se_bwd_f32', 'te_id_stem_bwd_f32', 'te_rows_unit_bwd_f32')
    for name in names:
        assert name in _lib.EXPORTS and name + '(' in header
    assert 'M9b' in header and 'id_loss.py:23-45' in header
    assert 'irse_bwd.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'irse_bwd.hip'))
    build.build()                                                               # (a no-op when the library is up to date)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16                   # validation only: never dereferenced
    geo = (1, 3, 4, 8, 8, 3, 3, 2, 1, 1)

    def dgrad(gx=p, g=p, wt=p, pre=None, slope=None, scale=None, add=None, geo=geo, add_s=1):
        return L.te_conv2d_dgrad_f32(gx, g, wt, pre, slope, scale, add, *geo, add_s, None)
    assert dgrad(gx=None) == -1 and dgrad(g=None) == -1 and dgrad(wt=None) == -1 and b'NULL' in L.te_last_error_string()
    assert dgrad(pre=p) == -1 and dgrad(slope=p) == -1 and b'both' in L.te_last_error_string()
    assert dgrad(pre=p, slope=p, scale=p) == -3 and dgrad(pre=p, slope=p, add=p) == -3
    assert dgrad(add=p, add_s=3) == -3 and dgrad(add=p, add_s=0) == -3
    assert dgrad(geo=(1, 3, 4, 8, 8, 3, 3, 3, 1, 1)) == -3 and b'stride' in L.te_last_error_string()
    assert dgrad(geo=(1, 3, 4, 8, 8, 8, 3, 1, 1, 1)) == -3 and dgrad(geo=(1, 3, 4, 8, 8, 3, 3, 1, 3, 1)) == -2
    assert dgrad(geo=(0, 3, 4, 8, 8, 3, 3, 1, 1, 1)) == -2 and dgrad(geo=(1, 3, 4, 2, 8, 5, 3, 1, 1, 1)) == -2
    assert L.te_conv2d_prelu_keep_f32(p, None, p, p, p, p, None, None, 1, 3, 4, 8, 8, 3, 3, 1, 1, 1, None) == -1
    assert L.te_conv2d_prelu_keep_f32(p, p, p, p, p, p, None, None, 1, 3, 4, 8, 8, 3, 3, 3, 1, 1, None) == -3
    assert L.te_id_stem_keep_f32(p, None, p, p, p, p, 1, 40, 40, 4, 36, 4, 36, 16, 8, None) == -1
    assert L.te_id_stem_keep_f32(p, p, p, p, p, p, 1, 40, 40, 4, 41, 4, 36, 16, 8, None) == -2
    assert L.te_se_bwd_f32(p, p, p, p, p, p, p, None, 2, 8, 4, 7, 7, None) == -1
    for B, C, Rn, Ho, Wo in [(0, 8, 4, 7, 7), (2, 0, 4, 7, 7), (2, 8, 0, 7, 7), (2, 8, 1025, 7, 7), (2, 8, 4, 0, 7), (2, 8, 4, 7, 0)]:
        assert L.te_se_bwd_f32(p, p, p, p, p, p, p, p, B, C, Rn, Ho, Wo, None) == -2, (B, C, Rn, Ho, Wo)
    assert L.te_id_stem_bwd_f32(p, p, p, p, None, p, 1, 40, 40, 4, 36, 4, 36, 16, 8, None) == -1
    for N, H, W, y0, y1, x0, x1, Pn, Co in [(1, 40, 40, 4, 4, 4, 36, 16, 8), (1, 40, 40, 4, 41, 4, 36, 16, 8), (1, 40, 40, 4, 36, 4, 36, 0, 8),
                                            (0, 40, 40, 4, 36, 4, 36, 16, 8), (1, 40, 40, 4, 36, 4, 36, 16, 0)]:
        assert L.te_id_stem_bwd_f32(p, p, p, p, p, p, N, H, W, y0, y1, x0, x1, Pn, Co, None) == -2, (N, H, W, y0, y1, x0, x1, Pn, Co)
    assert L.te_rows_unit_bwd_f32(p, p, p, None, 5, 8, None) == -1
    assert L.te_rows_unit_bwd_f32(p, p, p, p, 0, 8, None) == -2 and L.te_rows_unit_bwd_f32(p, p, p, p, 5, 0, None) == -2

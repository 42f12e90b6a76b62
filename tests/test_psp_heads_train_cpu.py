"""Host side of encoder head training (transeditor_amd.psp_heads_train) without a GPU: the pinned restatement
(tests/psp_heads_bwd_restated.py) against torch's own autograd, the export of the trained parameters under the reference's key names
against the packing of the launch program, the handling of EqualLinear's scale in the gradients, the shape checks of the new bindings,
the C ABI's refusals and the split rule of the weight gradient, the command line."""
import ctypes
import math
import os

import pytest
import torch
import torch.nn.functional as F

import arcface_restated as R
import psp_encoder_restated as P
import psp_heads_bwd_restated as HB
from conftest import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = P.SMALL
KW = dict(taps=G['taps'], units=G['units'])


@pytest.fixture(scope='module')
def small():
    x = R.images(211, 2, G['S'])
    return x, P.small_state_dict(6, images=x)


@pytest.fixture(scope='module')
def heads(small):
    from transeditor_amd.psp_heads_train import TrainableHeads
    return TrainableHeads(state_dict=small[1], **KW)


# ---------------------------------------------------------------------------------------------------------- the restatement
def test_pinned_restatement_is_autograd_of_the_unpinned_one(small):
    """with the masks fp64 itself takes, x * where(mask, 1, slope) differentiates to what F.leaky_relu does; the stage from the features on
    is psp_encoder_restated.encode; a flipped mask changes the gradient (the pin is live)"""
    x, sd = small
    c = HB.features(x, sd, torch.float64, G['units'], G['taps'])
    g = torch.Generator().manual_seed(17)
    gz, gp = torch.randn(2, G['D'], G['tokens'], generator=g, dtype=torch.float64), torch.randn(2, G['D'], G['spatials'], generator=g, dtype=torch.float64)
    free = HB.gradients(c, sd, gz, gp, torch.float64)
    z64, p64 = P.encode(x, sd, torch.float64, G['units'], G['taps'])
    assert torch.equal(free['z'], z64) and torch.equal(free['p'], p64)
    assert set(free['grads']) == set(HB.trained_keys(sd)) | {'c1', 'c2', 'c3'}
    assert len(free['masks']) == sum(P._depth(sd, q) for q in HB.head_prefixes(sd)) == 2 * 2 + 3 + 2 * 4 + 4 * 2
    share = torch.cat([m.reshape(-1) for m in free['masks'].values()]).double().mean()
    assert 0.2 < float(share) < 0.8
    pinned = HB.gradients(c, sd, gz, gp, torch.float64, masks=free['masks'])
    assert rel_l2(pinned['z'], free['z']) < 1e-14 and rel_l2(pinned['p'], free['p']) < 1e-14
    for k, v in free['grads'].items():
        assert float(v.abs().max()) > 0, k
        assert rel_l2(pinned['grads'][k], v) < 1e-13, k
    flipped = dict(free['masks'])
    flipped['styles.4', 0] = ~flipped['styles.4', 0]
    other = HB.gradients(c, sd, gz, gp, torch.float64, masks=flipped)
    assert rel_l2(other['grads']['styles.4.convs.0.weight'], free['grads']['styles.4.convs.0.weight']) > 0.1
    assert torch.equal(other['grads']['styles.0.convs.0.weight'], pinned['grads']['styles.0.convs.0.weight'])


# ---------------------------------------------------------------------------------------------------------- export and packing
def test_parameters_and_reference_keys(small, heads):
    from transeditor_amd import psp_encoder as E
    _, sd = small
    assert set(heads.reference_keys()) == set(HB.trained_keys(sd)) and len(heads.reference_keys()) == len(set(heads.reference_keys()))
    net = E.parse_state_dict(sd, **KW)
    D, n = 64, 9
    shapes = {k: tuple(p.shape) for k, p in heads.named_parameters()}
    assert list(shapes) == heads.names
    for i, l in enumerate(net['launches']):
        Gn = len(l['heads'])
        # [G*D, Ci, 3, 3]: every dim but the first is one output channel's row, what Ranger centralises in the reference's [D, Ci, 3, 3]
        assert shapes[f'h{i}_w'] == (Gn * D, l['w'].shape[2], 3, 3) and shapes[f'h{i}_b'] == (Gn * D,)
        assert torch.equal(getattr(heads, f'h{i}_w').detach().view_as(l['w']), l['w']) and torch.equal(getattr(heads, f'h{i}_b').detach(), l['b'])
    assert shapes['lin_w'] == (n * D, D) and shapes['adjust_w'] == (4, 5) and shapes['lat1_w'] == (64, 32, 1, 1) and shapes['lat2_w'] == (64, 16, 1, 1)
    assert all(p.dtype == torch.float32 and p.requires_grad for p in heads.parameters())
    # the EqualLinear weights are the STORED ones; the scales are the reference's
    assert torch.equal(heads.lin_w.detach()[:D], sd['styles.0.linear.weight']) and torch.equal(heads.adjust_w.detach(), sd['adjust_style.weight'])
    assert heads.lin_scale == 1 / math.sqrt(D) and heads.adjust_scale == 1 / math.sqrt(5)
    assert sum(p.numel() for p in heads.parameters()) == sum(sd[k].numel() for k in HB.trained_keys(sd))


def test_export_round_trips_through_the_parser(small):
    """trained values go out under the reference's keys and come back through parse_state_dict as the same packed tensors, bit for bit;
    the backbone's entries are the source's own; the checkpoint layout is coach_new.py's"""
    from transeditor_amd import psp_encoder as E
    from transeditor_amd.psp_heads_train import TrainableHeads
    _, sd = small
    heads = TrainableHeads(state_dict=sd, **KW)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in heads.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.05)
    out = heads.export_state_dict(sd)
    assert set(out) == set(sd) and all(out[k].shape == sd[k].shape and out[k].dtype == sd[k].dtype for k in sd)
    trained = set(HB.trained_keys(sd))
    for k in sd:
        assert torch.equal(out[k], sd[k]) != (k in trained), k                   # every head key moved, nothing else did
    net = E.parse_state_dict(out, **KW)
    for i, l in enumerate(net['launches']):
        assert torch.equal(l['w'].view(-1, *l['w'].shape[2:]), getattr(heads, f'h{i}_w').detach()) and torch.equal(l['b'], getattr(heads, f'h{i}_b').detach())
    assert torch.equal(net['stored']['lin_w'].view(-1, 64), heads.lin_w.detach()) and torch.equal(net['lin'][1], heads.lin_b.detach())
    assert torch.equal(net['stored']['A'], heads.adjust_w.detach()) and torch.equal(net['bz'], heads.adjust_b.detach())
    assert torch.equal(net['lat1'][0], heads.lat1_w.detach()) and torch.equal(net['lat2'][1], heads.lat2_b.detach())
    again = TrainableHeads(state_dict=out, **KW)
    assert all(torch.equal(a, b) for a, b in zip(again.parameters(), heads.parameters()))
    ck = heads.checkpoint(P.checkpoint(sd, plus=True, averages=True))
    assert set(ck) == {'state_dict', 'opts', 'z_plus_latent_avg', 'p_plus_latent_avg'} and 'decoder.style.0.weight' in ck['state_dict']
    enc, opts, za, _, plus = E.split_checkpoint(ck)
    assert plus and opts['start_from_latent_avg'] and za.shape == (1, 64, 4) and all(torch.equal(enc[k], out[k]) for k in out)
    bare = heads.checkpoint(sd)
    assert set(bare) == {'state_dict', 'opts'} and set(bare['state_dict']) == {f'encoder.{k}' for k in sd}
    assert all(torch.equal(a, b) for a, b in zip(TrainableHeads(state_dict=bare, **KW).parameters(), heads.parameters()))
    with pytest.raises(ValueError, match='not the encoder these heads were built from'):
        heads.export_state_dict({k: v for k, v in sd.items() if k != 'styles.3.convs.4.bias'})


def test_a_packed_gradient_maps_back_to_its_reference_key(small, heads):
    """every reference key gets a tensor that names it; packed by the parser and read back by `unpack`, each head of each level returns
    its own"""
    from transeditor_amd import psp_encoder as E
    from transeditor_amd.psp_heads_train import unpack
    _, sd = small
    keys = HB.trained_keys(sd)
    tagged = dict(sd)
    for n, k in enumerate(keys):
        tagged[k] = torch.arange(sd[k].numel(), dtype=torch.float32).reshape(sd[k].shape) * 2.0 ** -12 + float(n + 1)
    net = E.parse_state_dict(tagged, **KW)
    named = {}
    for i, l in enumerate(net['launches']):
        named[f'h{i}_w'], named[f'h{i}_b'] = l['w'].view(-1, *l['w'].shape[2:]), l['b']
    named['lin_w'], named['lin_b'] = net['stored']['lin_w'].view(-1, 64), net['lin'][1]
    named['adjust_w'], named['adjust_b'] = net['stored']['A'], net['bz']
    (named['lat1_w'], named['lat1_b']), (named['lat2_w'], named['lat2_b']) = net['lat1'], net['lat2']
    assert set(named) == set(heads.names)
    back = unpack(named, heads.launch_heads, 64, 5, 4)
    assert set(back) == set(keys)
    for k in keys:
        assert torch.equal(back[k], tagged[k]), k


def test_equal_linear_scale_in_the_gradients():
    """the node folds the scale into the weight on the way in (fp64, one rounding) and multiplies the folded weight's gradient by it on
    the way out: that is autograd's gradient of the STORED weight, for the heads' linears and for adjust_style"""
    from transeditor_amd.psp_heads_train import fold
    g = torch.Generator().manual_seed(5)
    D, Ns, B, T = 64, 5, 3, 4
    for shape, scale, x in (((D, D), 1 / math.sqrt(D), torch.randn(B, D, generator=g, dtype=torch.float64)),
                            ((T, Ns), 1 / math.sqrt(Ns), torch.randn(B, D, Ns, generator=g, dtype=torch.float64))):
        w = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
        cot = torch.randn(*x.shape[:-1], shape[0], generator=g, dtype=torch.float64)
        want, = torch.autograd.grad(F.linear(x, w * scale), w, cot)             # EqualLinear.forward: F.linear(input, self.weight * self.scale)
        wf = fold(w, scale).requires_grad_(True)
        assert torch.equal(wf.detach(), w.detach() * scale)
        gf, = torch.autograd.grad(F.linear(x, wf), wf, cot)
        assert rel_l2(gf * scale, want) < 1e-15
    w32 = torch.randn(D, D, generator=g)
    assert fold(w32, 0.125).dtype == torch.float32 and torch.equal(fold(w32, 0.125), w32 * 0.125)


# ---------------------------------------------------------------------------------------------------------- the bindings
def test_wrapper_shape_checks_raise_before_the_library():
    from transeditor_amd import _lib
    z = torch.zeros
    w = z(2, 64, 64, 3, 3)
    wt = _lib.heads_dgrad_weight(w, 2, (1, 1))
    assert wt.shape == (2 * 64 * 64 * 9,)
    # the layout: per phase, the heads' flipped [Ci, Cg, ny, nx] blocks one behind the other = dgrad_weight per head
    w = torch.randn(2, 64, 64, 3, 3, generator=torch.Generator().manual_seed(1))
    per_head = [_lib.dgrad_weight(w[g], 2, (1, 1)) for g in range(2)]
    wt, at, off = _lib.heads_dgrad_weight(w, 2, (1, 1)), 0, 0
    for ny, nx in ((1, 1), (1, 2), (2, 1), (2, 2)):                             # the phases (ry, rx) of a 3 x 3 stride-2 pad-1 layer, ry-major
        size = 64 * 64 * ny * nx
        for g in range(2):
            assert torch.equal(wt[at:at + size], per_head[g][off:off + size]), (ny, nx, g)
            at += size
        off += size
    assert at == wt.numel()
    with pytest.raises(RuntimeError, match='heads_dgrad_weight expects'):
        _lib.heads_dgrad_weight(z(64, 64, 3, 3))
    g = z(2, 128, 4, 4)
    with pytest.raises(RuntimeError, match='conv2d_heads_dgrad: inconsistent shapes'):
        _lib.conv2d_heads_dgrad(g, wt[:-1], (2, 128, 8, 8), 2, (3, 3), 2, (1, 1))
    with pytest.raises(RuntimeError, match='conv2d_heads_dgrad: inconsistent shapes'):
        _lib.conv2d_heads_dgrad(g, wt, (2, 128, 8, 8), 2, (3, 3), 2, (1, 1), act=z(2, 128, 8, 4))
    with pytest.raises(RuntimeError, match='conv2d_heads_dgrad: inconsistent shapes'):
        _lib.conv2d_heads_dgrad(g, wt, (2, 128, 8, 8), 3, (3, 3), 2, (1, 1))
    with pytest.raises(RuntimeError, match=r'conv2d_heads_dgrad: g must be \[2,Ctot,4,4\]'):
        _lib.conv2d_heads_dgrad(z(2, 128, 4, 5), wt, (2, 128, 8, 8), 2, (3, 3), 2, (1, 1))
    with pytest.raises(RuntimeError, match=r'channels \[64, 64 \+ 128\) inside it'):
        _lib.conv2d_heads_dgrad(g, wt, (2, 128, 8, 8), 2, (3, 3), 2, (1, 1), c0=64)
    with pytest.raises(RuntimeError, match='conv2d_heads_wgrad: inconsistent shapes'):
        _lib.conv2d_heads_wgrad(g, z(2, 128, 8, 8), (2, 64, 64, 3, 3), 2, (1, 1), shared=True)
    with pytest.raises(RuntimeError, match='conv2d_heads_wgrad: inconsistent shapes'):
        _lib.conv2d_heads_wgrad(g, z(2, 64, 8, 8), (2, 64, 64, 3, 3), 2, (1, 1), shared=False)
    with pytest.raises(RuntimeError, match=r'conv2d_heads_wgrad: g must be \[2,Ctot,4,4\]'):
        _lib.conv2d_heads_wgrad(z(2, 127, 4, 4), z(2, 128, 8, 8), (2, 64, 64, 3, 3), 2, (1, 1))
    with pytest.raises(RuntimeError, match='upsample_add_bwd expects'):
        _lib.upsample_add_bwd(z(2, 3, 8, 8), (2, 4, 4, 4))
    with pytest.raises(RuntimeError, match='upsample_add_bwd expects'):
        _lib.upsample_add_bwd(z(2, 3, 8, 8), (2, 3, 4, 4), add=z(2, 3, 4, 5))
    with pytest.raises(RuntimeError, match='psp_codes_bwd: inconsistent shapes'):
        _lib.psp_codes_bwd(z(2, 64, 4), z(2, 64, 4), z(2, 9, 64), z(4, 6))
    with pytest.raises(RuntimeError, match='psp_codes_bwd: inconsistent shapes'):
        _lib.psp_codes_bwd(z(2, 64, 4), z(3, 64, 4), z(2, 9, 64), z(4, 5))
    with pytest.raises(RuntimeError, match='no CPU path'):
        _lib.psp_codes_bwd(z(2, 64, 4), z(2, 64, 4), z(2, 9, 64), z(4, 5))


def test_abi_entry_points_refusals_and_the_split_rule():
    from transeditor_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    names = ('te_conv2d_heads_dgrad_f32', 'te_conv2d_heads_wgrad_splits', 'te_conv2d_heads_wgrad_ws_bytes', 'te_conv2d_heads_wgrad_f32',
             'te_upsample_add_bwd_f32', 'te_psp_codes_bwd_f32')
    for name in names:
        assert name in _lib.EXPORTS and name + '(' in header
    section = ' '.join(header.split('M10b')[1].replace(' * ', ' ').split())
    assert 'coach_new.py:128-135' in section and 'nothing is launched on a refusal' in section and 'psp_encoders_new.py:11-32' in section
    assert 'psp_heads_bwd.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'psp_heads_bwd.hip'))
    build.build()                                                               # (a no-op when the library is up to date)
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16                   # validation only: never dereferenced
    dg = dict(B=2, G=2, Ci=64, Cg=64, H=8, W=8, kh=3, kw=3, s=2, py=1, px=1, gCtot=128, gc0=0, slope=0.01)

    def dgrad(gx=p, g=p, wt=p, act=p, **kw):
        return L.te_conv2d_heads_dgrad_f32(gx, g, wt, act, *dict(dg, **kw).values(), None)
    assert dgrad(gx=None) == -1 and dgrad(g=None) == -1 and dgrad(wt=None) == -1 and b'NULL' in L.te_last_error_string()
    assert dgrad(Ci=72) == -3 and b'multiple of 64' in L.te_last_error_string()
    assert dgrad(slope=0.0) == -3 and dgrad(slope=-0.01) == -3 and dgrad(slope=float('nan')) == -3 and b'positive' in L.te_last_error_string()
    assert dgrad(s=3) == -3 and dgrad(kh=8) == -3 and dgrad(G=0) == -2 and dgrad(B=0) == -2 and dgrad(py=3) == -2
    assert dgrad(gc0=1) == -2 and dgrad(gCtot=127) == -2 and b'outside' in L.te_last_error_string()
    wg = dict(B=2, G=2, Ci=16, Cg=64, H=8, W=8, kh=3, kw=3, s=2, py=1, px=1, gCtot=128, gc0=0, shared=0, splits=1)

    def wgrad(gw=p, gb=p, ws=None, ws_bytes=0, g=p, x=p, **kw):
        return L.te_conv2d_heads_wgrad_f32(gw, gb, ws, ws_bytes, g, x, *dict(wg, **kw).values(), None)
    assert wgrad(gw=None) == -1 and wgrad(gb=None) == -1 and wgrad(g=None) == -1 and wgrad(x=None) == -1
    assert wgrad(Cg=72) == -3 and wgrad(s=3) == -3 and wgrad(kw=8) == -3
    assert wgrad(G=0) == -2 and wgrad(B=0) == -2 and wgrad(px=3) == -2 and wgrad(gc0=64) == -2 and wgrad(splits=17) == -2 and wgrad(splits=-1) == -2
    assert wgrad(splits=2) == -2 and b'non-empty' in L.te_last_error_string()   # R = 32: one step
    assert wgrad(H=32, W=32, splits=2) == -4 and wgrad(H=32, W=32, splits=2, ws=p, ws_bytes=2 * 128 * 144 * 4 - 4) == -4
    assert b'workspace' in L.te_last_error_string()
    # the rule is a function of (M, N, R) alone.  The head launches of the true geometry have 576 tiles per head: never split.  The
    # laterals have 32 and 16 tiles and R = B * 1024 and B * 4096
    S = L.te_conv2d_heads_wgrad_splits
    assert S(512, 512, 3, 3, 8, 32, 32) == 1 and S(512, 512, 3, 3, 8, 1, 1) == 1 and S(512, 512, 1, 1, 8, 1, 1) == 1
    assert S(512, 256, 1, 1, 8, 32, 32) == 8 and S(512, 128, 1, 1, 8, 64, 64) == 16
    assert S(64, 8, 3, 3, 5, 16, 16) == 10 and S(64, 8, 3, 3, 1, 4, 4) == 1      # 40 steps in ranges of at least 4; one step
    assert S(72, 8, 3, 3, 5, 16, 16) < 0 and S(64, 0, 3, 3, 5, 16, 16) < 0 and S(64, 8, 9, 3, 5, 16, 16) < 0
    W = L.te_conv2d_heads_wgrad_ws_bytes
    assert W(8, 1, 512, 256, 1, 1, 32, 32) == 8 * 512 * 256 * 4 and W(8, 30, 512, 512, 3, 3, 4, 4) == 0 and W(0, 1, 512, 256, 1, 1, 32, 32) < 0
    assert L.te_upsample_add_bwd_f32(None, p, None, 4, 4, 4, 8, 8, None) == -1 and L.te_upsample_add_bwd_f32(p, None, None, 4, 4, 4, 8, 8, None) == -1
    assert L.te_upsample_add_bwd_f32(p, p, None, 0, 4, 4, 8, 8, None) == -2 and L.te_upsample_add_bwd_f32(p, p, None, 65536, 4, 4, 8, 8, None) == -2
    assert L.te_upsample_add_bwd_f32(p, p, None, 4, 0, 4, 8, 8, None) == -2 and L.te_upsample_add_bwd_f32(p, p, None, 4, 4, 4, 8, 32769, None) == -2
    for hole in range(7):
        args = [p] * 7
        args[hole] = None
        assert L.te_psp_codes_bwd_f32(*args, 2, 5, 4, 64, 4, None) == -1, hole
    for bad in [(0, 5, 4, 64, 4), (2, 0, 4, 64, 4), (2, 5, 0, 64, 4), (2, 5, 4, 0, 4), (2, 5, 4, 64, 0)]:
        assert L.te_psp_codes_bwd_f32(*([p] * 7), *bad, None) == -2, bad


# ---------------------------------------------------------------------------------------------------------- the module
def test_module_docstring_command_line_and_decoder(small, heads):
    from transeditor_amd import psp_heads_train as T
    doc = T.__doc__
    for phrase in ('Out of scope', "backbone's backward pass", 'fake-guide step', 'coach_new.py:137-151', 'train_decoder', 'validation loop', 'logging',
                   'coach_new.py:128-135', 'face_pool'):
        assert phrase in doc, phrase
    parse = T.build_parser().parse_args
    a = parse(['--ckpt', 'psp.pt', '--g_ckpt', 'G.pt', '--images', 'X.pt', '--steps', '5', '--out', 'tuned.pt'])
    assert (a.ckpt, a.g_ckpt, a.images, a.steps, a.out, a.lr, a.batch, a.id_ckpt, a.alexnet, a.lpips_alex_lin) == \
        ('psp.pt', 'G.pt', 'X.pt', 5, 'tuned.pt', 1e-4, 8, None, None, None)
    for bad in (['--g_ckpt', 'G.pt', '--images', 'X.pt', '--steps', '5', '--out', 't.pt'], ['--ckpt', 'p.pt', '--g_ckpt', 'G.pt', '--images', 'X.pt', '--out', 't.pt']):
        with pytest.raises(SystemExit):
            parse(bad)
    base = ['--ckpt', 'psp.pt', '--g_ckpt', 'G.pt', '--images', 'X.pt', '--out', 't.pt']
    with pytest.raises(SystemExit):
        T.main(base + ['--steps', '0'])
    with pytest.raises(SystemExit):
        T.main(base + ['--steps', '2', '--alexnet', 'a.pth'])

    class Gen(torch.nn.Module):
        def __init__(self, size):
            super().__init__()
            self.size, self.w = size, torch.nn.Parameter(torch.ones(3))

        def forward(self, z, p, return_latents=False, **kw):
            self.kw = kw
            return z.sum() + p.sum() + self.w.sum(), None, None
    with pytest.raises(ValueError, match='face_pool is the identity for a 256 px generator only; this one is 32 px'):
        T.generator_decoder(Gen(32), True)
    gen = Gen(256)
    decode = T.generator_decoder(gen, True)
    assert not gen.w.requires_grad
    z = torch.ones(1, 2, 3, requires_grad=True)
    out = decode(z, torch.ones(1, 2, 3))
    assert gen.kw == dict(use_spatial_mapping=False, use_style_mapping=False) and out.requires_grad
    T.generator_decoder(gen, False, resize=False)(z, z)
    assert gen.kw == {}
    if not torch.cuda.is_available():
        x, _ = small
        with pytest.raises(RuntimeError, match='TrainableHeads needs a GPU'):
            heads(None, None, torch.zeros(2, 64, 4, 4))
        with pytest.raises(RuntimeError, match='TrainableHeads needs a GPU'):
            T.main(base + ['--steps', '2'])

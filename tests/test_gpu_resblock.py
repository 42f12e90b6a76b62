"""The discriminator's ResBlock as one autograd node (op/resblock.py; reference ResBlock.forward,
model_spatial_query.py:780-798) and the two kernel features it stands on: the residual epilogue of te_conv_res_f32 and the
activation-gradient epilogue of the adjoint blur (te_blur_gradact_f32).  Checked against the CPU oracle (forward, dx, every
parameter gradient, R1-style double backward) and against the unfused route of the same module."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, rel_l2
from oracle import te_oracle as O
from transeditor_amd import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _block(cin, cout, seed):
    from transeditor_amd.model_spatial_query import ResBlock
    rb = ResBlock(cin, cout)
    sd = rb.state_dict()
    synth.fill_state_dict(sd, seed)
    for k in sd:
        if k.endswith('bias'):                       # FusedLeakyReLU biases start at zero: give them values
            sd[k].copy_(0.3 * synth.normal(tuple(sd[k].shape), f'rb.b.{k}.{seed}'))
    rb.load_state_dict(sd)
    return rb.to(DEV), {k: v.clone() for k, v in sd.items()}


def _oracle_block(P, x):
    h = O.conv_layer(P, 'conv1', x, 3)
    h = O.conv_layer(P, 'conv2', h, 3, downsample=True)
    s = O.conv_layer(P, 'skip', x, 1, downsample=True, bias=False, activate=False)
    return (h + s) / math.sqrt(2)


@pytest.mark.parametrize('cin,cout,H,B', [(16, 32, 16, 3), (64, 128, 32, 2), (128, 256, 64, 2), (24, 40, 10, 2), (512, 512, 8, 4)])
def test_resblock_node_vs_oracle(cin, cout, H, B):
    rb, sd = _block(cin, cout, 3)
    assert rb._standard()
    x = synth.normal((B, cin, H, H), f'rb.x.{cin}.{H}')
    gy = synth.normal((B, cout, H // 2, H // 2), f'rb.g.{cout}.{H}')
    P = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'kernel' not in k else v) for k, v in sd.items()}
    xc = x.clone().requires_grad_(True)
    ref = _oracle_block(P, xc)
    names = [k for k, v in P.items() if v.requires_grad]
    gref = torch.autograd.grad((ref * gy).sum(), [xc] + [P[k] for k in names])
    xd = x.to(DEV).requires_grad_(True)
    out = rb(xd)
    assert out.grad_fn is not None and 'ResBlock' in type(out.grad_fn).__name__
    assert rel_err(out, ref) < 2e-5
    params = dict(rb.named_parameters())
    got = torch.autograd.grad((out * gy.to(DEV)).sum(), [xd] + [params[k] for k in names])
    for n, a, b in zip(['dx'] + names, got, gref):
        assert rel_l2(a, b) < 2e-5, n
        assert rel_err(a, b) < 2e-4, n


def test_resblock_node_frozen_weights_and_unfused_route():
    """G step: the discriminator is frozen, only dx flows.  And the node equals the unfused route (second_order()) of the module."""
    from transeditor_amd.op.modconv import second_order
    rb, _ = _block(64, 128, 5)
    x = synth.normal((2, 64, 32, 32), 'rb.x2').to(DEV)
    gy = synth.normal((2, 128, 16, 16), 'rb.g2').to(DEV)
    xa = x.clone().requires_grad_(True)
    with second_order():
        ya = rb(xa)
    ga = torch.autograd.grad((ya * gy).sum(), [xa] + list(rb.parameters()))
    for p in rb.parameters():
        p.requires_grad_(False)
    xb = x.clone().requires_grad_(True)
    yb = rb(xb)
    gb, = torch.autograd.grad((yb * gy).sum(), [xb])
    assert rel_err(yb, ya) < 1e-5 and rel_l2(gb, ga[0]) < 1e-5


def test_resblock_node_double_backward_matches_oracle():
    """R1-style: d/dparams of || d out . gy / dx ||^2 through the node's recorded backward vs the CPU oracle."""
    rb, sd = _block(32, 64, 7)
    x = synth.normal((2, 32, 16, 16), 'rb.x3')
    gy = synth.normal((2, 64, 8, 8), 'rb.g3')
    P = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'kernel' not in k else v) for k, v in sd.items()}
    names = [k for k, v in P.items() if v.requires_grad]
    xc = x.clone().requires_grad_(True)
    gx, = torch.autograd.grad((_oracle_block(P, xc) * gy).sum(), xc, create_graph=True)
    ref = torch.autograd.grad(gx.pow(2).sum(), [P[k] for k in names], allow_unused=True)
    xd = x.to(DEV).requires_grad_(True)
    out = rb(xd)                                               # fused node; its backward is recorded below
    gxd, = torch.autograd.grad((out * gy.to(DEV)).sum(), xd, create_graph=True)
    assert rel_l2(gxd, gx) < 2e-5
    params = dict(rb.named_parameters())
    got = torch.autograd.grad(gxd.pow(2).sum(), [params[k] for k in names], allow_unused=True)
    for n, a, b in zip(names, got, ref):
        if b is None or float(b.abs().max()) == 0:
            assert a is None or float(a.abs().max()) < 1e-6, n
            continue
        assert rel_l2(a, b) < 1e-4, n


@pytest.mark.parametrize('kind,K,M,H,B', [('3x3', 64, 128, 32, 2), ('1x1', 128, 256, 64, 2), ('3x3', 512, 512, 8, 4),
                                         ('1x1', 256, 512, 4, 4), ('3x3', 20, 24, 9, 3)])
def test_conv_residual_epilogue(kind, K, M, H, B):
    """out = act(conv + bias) + res, on the one-pass and on the split-K (small image) route"""
    from transeditor_amd import _lib
    ks = 3 if kind == '3x3' else 1
    x = synth.normal((B, K, H, H), f'cr.x.{K}.{H}')
    w = synth.normal((M, K, ks, ks), f'cr.w.{K}.{M}') / math.sqrt(K * ks * ks)
    b = 0.2 * synth.normal((M,), f'cr.b.{M}')
    r = synth.normal((B, M, H, H), f'cr.r.{M}.{H}')
    for act in (0, 3):
        ref = F.conv2d(x, w, b, padding=ks // 2)
        if act:
            ref = F.leaky_relu(ref, 0.2) * math.sqrt(2)
        ref = ref + r
        wp = _lib.conv_pack(w.to(DEV), _lib.PACK_FWD, 1.0)
        out = _lib.conv(x.to(DEV), wp, _lib.CONV_3X3 if ks == 3 else _lib.CONV_1X1, M, H, H, None, None, b.to(DEV), act, res=r.to(DEV))
        assert rel_err(out, ref) < 2e-5, act


@pytest.mark.parametrize('C,H,B', [(8, 64, 2), (5, 32, 3), (3, 128, 1), (16, 8, 2), (2, 256, 1), (4, 20, 2)])
def test_blur_gradact_kernel(C, H, B):
    """gx = adjoint_blur(g) * slope(ref), bias-gradient = its sum over batch and pixels (pad (2,2) blur: (H+1) -> H)"""
    from transeditor_amd import _lib
    k = O.fir_kernel((1, 3, 3, 1))
    g = synth.normal((B, C, H + 1, H + 1), f'bg.g.{C}.{H}')
    y = synth.normal((B, C, H, H), f'bg.y.{C}.{H}')
    # forward blur pad (2,2): H -> H+1; its adjoint has pads (1,1): H+1 -> H
    adj = O.upfirdn2d(g, torch.flip(k, [0, 1]), pad=(1, 1))
    ref = adj * torch.where(y > 0, math.sqrt(2), 0.2 * math.sqrt(2))
    gx, gb = _lib.blur_gradact(g.to(DEV), y.to(DEV), torch.flip(k, [0, 1]).contiguous().to(DEV), (1, 1, 1, 1), 0.2, math.sqrt(2))
    assert rel_err(gx, ref) < 1e-5
    assert rel_err(gb, ref.sum(dim=(0, 2, 3))) < 1e-5


@pytest.mark.parametrize('C,H,B', [(128, 64, 2), (64, 32, 3), (512, 8, 2)])
def test_from_rgb_stem_streaming_path(C, H, B):
    """ConvLayer(3, C, 1) (the discriminator's first layer, model_spatial_query.py:815) on the streaming kernels
    (te_rgb_expand_f32 forward, te_rgb_fwd_f32 data gradient, te_rgb_wgrad_f32 weight gradient) vs the CPU oracle."""
    from transeditor_amd.model_spatial_query import ConvLayer
    layer = ConvLayer(3, C, 1)
    sd = layer.state_dict()
    synth.fill_state_dict(sd, 17)
    sd['1.bias'].copy_(0.3 * synth.normal((C,), f'stem.b.{C}'))
    layer.load_state_dict(sd)
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    x = synth.normal((B, 3, H, H), f'stem.x.{H}')
    gy = synth.normal((B, C, H, H), f'stem.g.{C}.{H}')
    xc = x.clone().requires_grad_(True)
    ref = O.conv_layer({'s.0.weight': P['0.weight'], 's.1.bias': P['1.bias']}, 's', xc, 1)
    gy = gy * (ref.detach().abs() > 1e-4)                      # no upstream gradient at the leaky-ReLU kink
    gref = torch.autograd.grad((ref * gy).sum(), [xc, P['0.weight'], P['1.bias']])
    layer = layer.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = layer(xd)
    assert rel_err(out, ref) < 1e-5
    params = dict(layer.named_parameters())
    got = torch.autograd.grad((out * gy.to(DEV)).sum(), [xd, params['0.weight'], params['1.bias']])
    for n, a, b in zip(('dx', 'dW', 'db'), got, gref):
        assert rel_l2(a, b) < 2e-5 and rel_err(a, b) < 2e-4, n


@pytest.mark.parametrize('frozen', [False, True])
def test_discriminator_stem_plus_first_block_node(frozen):
    """Discriminator(64): from-RGB layer + first ResBlock run as ONE node (stem's activation gradient in the mask stage of the
    block's data-gradient epilogue, dW0 / db0 from one te_rgb_wgrad_sum_f32 pass).  Prediction, d/d image and every parameter
    gradient against the CPU oracle; `frozen` = the G step (only the image gradient flows)."""
    from transeditor_amd.model_spatial_query import Discriminator
    Dn = Discriminator(64)
    sd = Dn.state_dict()
    synth.fill_state_dict(sd, 5)
    for k in sd:
        if k.endswith('bias'):
            sd[k].copy_(0.2 * synth.normal(tuple(sd[k].shape), f'dst.b.{k}'))
    Dn.load_state_dict(sd)
    img = synth.normal((4, 3, 64, 64), 'dst.img').clamp(-1, 1)
    P = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'kernel' not in k else v) for k, v in sd.items()}
    names = [k for k, v in P.items() if v.requires_grad]
    from pinning import capture, pinned, record_oracle
    ic = img.clone().requires_grad_(True)
    with record_oracle() as bank:                     # the slope signs the oracle takes: the HIP passes below are pinned to them
        ref = O.discriminator_forward(P, ic, 64)
    w = synth.normal((4, 1), 'dst.w')
    gref = torch.autograd.grad((ref * w).sum(), [ic] + [P[k] for k in names])
    Dn = Dn.to(DEV)
    if frozen:
        for p in Dn.parameters():
            p.requires_grad_(False)
    params = dict(Dn.named_parameters())

    def run(second=False, bank_=None):
        from transeditor_amd.op.modconv import second_order
        import contextlib
        idv = img.to(DEV).requires_grad_(True)
        if not second:
            assert Dn._stem_fusable(idv)
        with (pinned(bank_) if bank_ is not None else contextlib.nullcontext({})) as st, (second_order() if second else contextlib.nullcontext()):
            pred = Dn(idv)
            got = torch.autograd.grad((pred * w.to(DEV)).sum(), [idv] + ([] if frozen else [params[k] for k in names]))
        if bank_ is not None:
            assert not st['unmatched'], st['unmatched']
        return pred, got, st

    # GATING comparison: slopes pinned to the oracle's (tests/pinning.py) - no flip is left, every gradient element-wise at 1e-4
    pred, got, st = run(bank_=bank)
    assert rel_err(pred, ref) < 1e-4
    worst = 0.0
    for n, a, b in zip(['dimg'] + names, got, gref):
        worst = max(worst, rel_l2(a, b))
        assert rel_l2(a, b) < 1e-4, (n, rel_l2(a, b))
    # the node against the unfused route of the same module (same kernels underneath, separate autograd nodes), pinned likewise
    pred2, got2, _ = run(second=True, bank_=bank)
    assert rel_err(pred2, pred) < 1e-5
    for n, a, b in zip(['dimg'] + names, got, got2):
        assert rel_l2(a, b) < 1e-4, (n, rel_l2(a, b))
    # INFORMATIONAL: the same comparison with free slopes.  A pre-activation within round-off of the kink takes the other slope in one
    # of two correct fp32 implementations and moves single gradient entries by parts in a thousand (measured 2.0e-3 for the image
    # gradient), so this bar only catches O(1) errors; precision is judged by the pinned comparison above.
    _, free, _ = run()
    flip = max(rel_l2(a, b) for a, b in zip(free, gref))
    print(f'stem + first block (frozen={frozen}): pinned worst {worst:.2e} ({st["flips"]} of {st["elements"]} slopes pinned); free slopes {flip:.2e}')
    assert flip < 2e-2


def test_resblock_backward_launches_the_kinds_its_forward_planned():
    """The forward decides each data gradient's convolution kind once and keeps it next to the packed weights: flipping
    modconv.USE_SPLIT_BF16 between forward and backward changes what the planners answer, but the backward still launches the split
    kernels its buffers were packed for.  The weight gradients follow the flag (fp32 kernels, another slab partition): dx and every
    parameter gradient match an unflipped run at 5e-6."""
    from transeditor_amd import _lib
    from transeditor_amd.op import modconv
    B, cin, cout, H = 32, 128, 256, 64
    w1, w2, ws = torch.empty(cin, cin, 3, 3), torch.empty(cout, cin, 3, 3), torch.empty(cout, cin, 1, 1)
    h = H // 2
    kinds = lambda: (modconv.fwd_kinds('3x3', B, w1, H, H)[1], modconv.bwd_kinds('3x3', B, w1, H, H)[1],
                     modconv.fwd_kinds('down', B, w2, h, h)[1], modconv.bwd_kinds('down', B, w2, h, h)[1],
                     modconv.plain_1x1_kinds(B, ws, h, h)[1], modconv.plain_1x1_kinds(B, ws, h, h, dgrad=True)[1])
    assert modconv.USE_SPLIT_BF16
    assert kinds() == (_lib.CONV_3X3W6, _lib.CONV_3X3W6, _lib.CONV_S2S6, _lib.CONV_T2S6, _lib.CONV_1X1S6, _lib.CONV_1X1S6)
    rb, _ = _block(cin, cout, 9)
    assert rb._standard()
    params = list(rb.parameters())
    x = synth.normal((B, cin, H, H), 'rb.once.x').to(DEV)
    gy = synth.normal((B, cout, h, h), 'rb.once.g').to(DEV)

    def grads(flip):
        xd = x.clone().requires_grad_(True)
        out = rb(xd)
        assert 'ResBlock' in type(out.grad_fn).__name__
        try:
            if flip:
                modconv.USE_SPLIT_BF16 = False
                assert _lib.wgrad_split() == 0 and _lib.CONV_3X3W6 not in kinds() and _lib.CONV_1X1S6 not in kinds()
            return torch.autograd.grad((out * gy).sum(), [xd] + params)
        finally:
            modconv.USE_SPLIT_BF16 = True

    want, got = grads(False), grads(True)
    assert _lib.wgrad_split() == 1
    for n, a, b in zip(['dx'] + [n for n, _ in rb.named_parameters()], got, want):
        assert rel_err(a, b) < 5e-6, n

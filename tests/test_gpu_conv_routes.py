"""The convolution ops the model calls - conv_core, the fused modconv node, modconv_closed under second_order() and the ResBlock
node - on every route of tests/conv_routes.py, against fp64 references built from stock torch ops on the GPU, through first and
second order, at bars near the kernel tests' ones.  Each test re-asserts its entry's routes before it compares numbers, so a
predicate change cannot silently move a case to another kernel.  Inputs also come as contiguous views at a 4-byte storage offset.

Bars: forward and data gradient 1e-5 (max-abs relative error); reductions (weight / scale / bias gradients) 2e-5 grown by
sqrt(reduction length / 4096); second order 1e-4.  The worst error per route and quantity is printed at the end of the module.
Measured on the MI355X: at most 1e-6 in first order and 7e-7 in second order on every route (7e-6 rel_l2 for the ResBlock's
bias gradient over 131 k pixels).  The bars stay at the fp32 class of the per-kernel tests (5e-6 there) instead of 4x those
numbers: a max-abs relative error of a few ulps moves with the seed and the reduction length, and these shapes are the smallest
per route, not the ones with the longest sums.  A packing, scaling or route slip of 1e-4 stays above every bar."""
import math
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

import conv_routes as cr
from conftest import rel_err, rel_l2
from fp64_check import off16
from transeditor_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SQRT2 = math.sqrt(2.0)

FWD_TOL = 1e-5
SO_TOL = 1e-4
WORST = defaultdict(float)


def red_tol(n):
    return 2e-5 * max(1.0, math.sqrt(n / 4096))


def _record(route, what, err, bar):
    key = (route, what)
    WORST[key] = max(WORST[key], err)
    assert err <= bar, f'{route}: {what} error {err:.3e} > {bar:.1e}'


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nworst errors per route (tests/test_gpu_conv_routes.py):')
    for (route, what), e in sorted(WORST.items()):
        print(f'  {route:28s} {what:22s} {e:.2e}')


def _gpu(shape, key, scale=1.0, offset=False):
    t = synth.normal(shape, key)
    if scale != 1.0:
        t = t * scale
    return off16(t, 4, DEV) if offset else t.to(DEV)


def _operands(route, tag, offset=False):
    B, K, M, H, W = route.shape
    ks = 1 if route.op in ('1x1', 'skip') else 3
    x = _gpu((B, K) + cr.in_hw(route.op, H, W), f'rt.x.{tag}', offset=offset)
    w = _gpu((M, K, ks, ks), f'rt.w.{tag}', 1.0 / math.sqrt(K * ks * ks))
    gy = _gpu((B, M) + cr.out_hw(route.op, H, W), f'rt.g.{tag}', offset=offset)
    return x, w, gy


CONV = [r for r in cr.ROUTES if r.op != 'skip']
IDS = lambda r: r.name


@pytest.mark.parametrize('offset', [False, True], ids=['dense', 'offset'])
@pytest.mark.parametrize('route', CONV, ids=IDS)
def test_conv_core_first_order(route, offset):
    B, K, M, H, W = route.shape
    ws = 0.7
    with cr.switches(**route.switches) as mc:
        cr.check(route)
        x, w, gy = _operands(route, route.name, offset)
        xd, wd = x.detach().requires_grad_(True), w.detach().clone().requires_grad_(True)
        y = mc.conv_core(xd, wd, route.op, ws)
        gx, gw = torch.autograd.grad(y, (xd, wd), gy)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = cr.ref_conv(route.op, x64, w64 * ws)
    gx64, gw64 = torch.autograd.grad(y64, (x64, w64), gy.double())
    sfx = ' (offset)' if offset else ''
    _record(route.name, 'core y' + sfx, rel_err(y, y64), FWD_TOL)
    _record(route.name, 'core dx' + sfx, rel_err(gx, gx64), FWD_TOL)
    _record(route.name, 'core dW' + sfx, rel_err(gw, gw64), red_tol(B * H * W))


@pytest.mark.parametrize('route', CONV, ids=IDS)
def test_conv_core_second_order(route):
    """d/d(x, w) of || dL/ds ||^2 + || dL/dw ||^2 with L = <y, gy> + ||y||^2 / 4, y = conv(x * s, w) (what R1 / path length
    differentiate), on every route.  The quadratic term makes the upstream gradient depend on y, so the second backward also runs
    the weight-gradient node's own backward"""
    ws = 0.7
    with cr.switches(**route.switches) as mc:
        cr.check(route)
        x, w, gy = _operands(route, route.name + '.so')
        s = (1 + 0.3 * synth.normal((route.shape[0], route.shape[1]), 'rt.s.' + route.name)).to(DEV)

        def f(conv, x, w, s):
            y = conv(x * s[:, :, None, None], w)
            gs, gw = torch.autograd.grad((y * gy.to(y.dtype)).sum() + 0.25 * y.square().sum(), (s, w), create_graph=True)
            return torch.autograd.grad(gs.pow(2).sum() + gw.pow(2).sum(), (x, w))

        got = f(lambda a, b: mc.conv_core(a, b, route.op, ws), *(t.detach().clone().requires_grad_(True) for t in (x, w, s)))
    ref = f(lambda a, b: cr.ref_conv(route.op, a, b * ws), *(t.double().requires_grad_(True) for t in (x, w, s)))
    for name, a, b in zip(('d2x', 'd2W'), got, ref):
        _record(route.name, 'core ' + name, rel_err(a, b), SO_TOL)
        _record(route.name, 'core ' + name + ' l2', rel_l2(a, b), SO_TOL)


def _demod64(w, isc, ws, eps):
    w3 = (w * ws).reshape(w.shape[0], w.shape[1], -1)
    return torch.rsqrt((w3[None] * isc[:, None, :, None]).square().sum(dim=(2, 3)) + eps)


# (upsampling layers fuse their activation into the blur that follows instead: no 'up' case with act)
MODC = [pytest.param(r, s, a, id=f'{r.name}-{s}-{"lrelu" if a else "linear"}')
        for r in CONV for s in ('demod', 'osc') for a in (False, True) if not (r.op == 'up' and a)]


@pytest.mark.parametrize('route,scales,act', MODC)
def test_modconv_fused_node(route, scales, act):
    """the fused first-order node: style scale, demodulation (in the node) or an explicit output scale, bias, leaky-ReLU"""
    B, K, M, H, W = route.shape
    ws, eps = 0.8, 1e-8
    with cr.switches(**route.switches) as mc:
        cr.check(route)
        x, w, gy = _operands(route, route.name + '.mc')
        isc = (1 + 0.5 * synth.normal((B, K), 'rt.i.' + route.name)).to(DEV)
        osc = ((1 + 0.3 * synth.normal((B, M), 'rt.o.' + route.name)).abs() + 0.1).to(DEV)
        bias = (0.5 * synth.normal((M,), 'rt.b.' + route.name)).to(DEV)
        leaves = [t.detach().clone().requires_grad_(True) for t in (x, w, isc, osc, bias)]
        if scales == 'demod':
            y = mc.modconv(leaves[0], leaves[1], leaves[2], None, leaves[4], act, route.op, ws, demod_eps=eps)
        else:
            y = mc.modconv(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], act, route.op, ws)
        want = [t for i, t in enumerate(leaves) if not (scales == 'demod' and i == 3)]
        # (upstream gradient masked where the pre-activation is within round-off of the kink: the slope may differ there)
        L64 = [t.double().requires_grad_(True) for t in (x, w, isc, osc, bias)]
        o64 = _demod64(L64[1], L64[2], ws, eps) if scales == 'demod' else L64[3]
        pre = cr.ref_conv(route.op, L64[0] * L64[2][:, :, None, None], L64[1] * ws) * o64[:, :, None, None] + L64[4][None, :, None, None]
        y64 = F.leaky_relu(pre, 0.2) * SQRT2 if act else pre
        g = gy.double() * (pre.detach().abs() > 1e-4) if act else gy.double()
        got = torch.autograd.grad(y, want, g.float())
    ref = torch.autograd.grad(y64, [t for i, t in enumerate(L64) if not (scales == 'demod' and i == 3)], g)
    Hi, Wi = cr.in_hw(route.op, H, W)
    Ho, Wo = cr.out_hw(route.op, H, W)
    names = ['dx', 'dW', 'disc'] + ([] if scales == 'demod' else ['dosc']) + ['dbias']
    bars = {'dx': FWD_TOL, 'dW': red_tol(B * H * W), 'disc': red_tol(Hi * Wi), 'dosc': red_tol(Ho * Wo), 'dbias': red_tol(B * Ho * Wo)}
    tag = f'mc[{scales},{"act" if act else "lin"}] '
    _record(route.name, tag + 'y', rel_err(y, y64), FWD_TOL)
    for n, a, b in zip(names, got, ref):
        _record(route.name, tag + n, rel_err(a, b), bars[n])


def test_modconv_demod_beyond_64_samples():
    """B > 64: modconv takes op/style.demod for the demodulation (outside the node)"""
    from transeditor_amd.op import modconv as mc
    B, K, M, H, W = 65, 16, 32, 4, 8
    ws, eps = 0.8, 1e-8
    x = _gpu((B, K, H, W), 'rt.d65.x')
    w = _gpu((M, K, 3, 3), 'rt.d65.w', 1 / 12)
    isc = (1 + 0.5 * synth.normal((B, K), 'rt.d65.i')).to(DEV)
    bias = (0.5 * synth.normal((M,), 'rt.d65.b')).to(DEV)
    gy = _gpu((B, M, H, W), 'rt.d65.g')
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, w, isc, bias)]
    y = mc.modconv(leaves[0], leaves[1], leaves[2], None, leaves[3], False, '3x3', ws, demod_eps=eps)
    got = torch.autograd.grad(y, leaves, gy)
    L64 = [t.double().requires_grad_(True) for t in (x, w, isc, bias)]
    y64 = F.conv2d(L64[0] * L64[2][:, :, None, None], L64[1] * ws, padding=1) * _demod64(L64[1], L64[2], ws, eps)[:, :, None, None] \
        + L64[3][None, :, None, None]
    ref = torch.autograd.grad(y64, L64, gy.double())
    _record('demod_b65', 'y', rel_err(y, y64), FWD_TOL)
    for n, a, b, bar in zip(('dx', 'dW', 'disc', 'dbias'), got, ref, (FWD_TOL, red_tol(B * H * W), red_tol(H * W), red_tol(B * H * W))):
        _record('demod_b65', n, rel_err(a, b), bar)


CLOSED = [r for r in cr.ROUTES if r.op in ('3x3', 'up', '1x1')]


@pytest.mark.parametrize('route', CLOSED, ids=IDS)
def test_modconv_closed_second_order(route):
    """modconv under second_order() - modconv_closed, or with USE_CLOSED_MODCONV off the chan_scale -> conv_core -> chan_scale
    composite: forward, the four first-order gradients, and the gradients of a scalar of them w.r.t. x, w, isc, osc.  The style
    vector has channels at |s| ~ 1e-3 and one exact 0 (the _nonzero floor of the closed family)."""
    B, K, M, H, W = route.shape
    ws = 0.9
    closed = route.switches.get('USE_CLOSED_MODCONV', True)
    with cr.switches(**route.switches) as mc:
        cr.check(route)
        x, w, gy = _operands(route, route.name + '.cl')
        isc = 1 + 0.5 * synth.normal((B, K), 'rt.ci.' + route.name)
        isc[:, 1] = 1e-3 * torch.sign(isc[:, 1])
        isc[:, 2] = -1.5e-3
        isc[0, 3] = 0.0
        isc = isc.to(DEV)
        osc = ((1 + 0.3 * synth.normal((B, M), 'rt.co.' + route.name)).abs() + 0.1).to(DEV)
        cot = [_gpu(tuple(t.shape), f'rt.cc{i}.' + route.name) for i, t in enumerate((x, w, isc, osc))]

        def f(conv, x, w, s, d):
            y = conv(x, w, s, d)
            g1 = torch.autograd.grad((y * gy.to(y.dtype)).sum(), (x, w, s, d), create_graph=True)
            S = sum((a * c.to(a.dtype)).sum() for a, c in zip(g1, cot))
            return (y,) + g1 + torch.autograd.grad(S, (x, w, s, d))

        leaves = [t.detach().clone().requires_grad_(True) for t in (x, w, isc, osc)]
        with mc.second_order():
            got = f(lambda x, w, s, d: mc.modconv(x, w, s, d, None, False, route.op, ws), *leaves)
    ref = f(lambda x, w, s, d: cr.ref_conv(route.op, x * s[:, :, None, None], w * ws) * d[:, :, None, None],
            *(t.double().requires_grad_(True) for t in (x, w, isc, osc)))
    Hi, Wi = cr.in_hw(route.op, H, W)
    Ho, Wo = cr.out_hw(route.op, H, W)
    _record(route.name, 'closed y', rel_err(got[0], ref[0]), FWD_TOL)
    for n, a, b, bar in zip(('dx', 'dW', 'disc', 'dosc'), got[1:5], ref[1:5],
                            (FWD_TOL, red_tol(B * H * W), red_tol(Hi * Wi), red_tol(Ho * Wo))):
        _record(route.name, 'closed ' + n, rel_err(a, b), bar)
    for n, a, b in zip(('d2x', 'd2W', 'd2osc'), (got[5], got[6], got[8]), (ref[5], ref[6], ref[8])):
        _record(route.name, 'closed ' + n, rel_err(a, b), SO_TOL)
        _record(route.name, 'closed ' + n + ' l2', rel_l2(a, b), SO_TOL)
    # d2/d isc.  Channels of ordinary size: the second-order bar.  The closed family forms d(dP/ds)/ds from two terms of size
    # |dP/ds| / |s| that cancel (_nonzero's docstring): the channels at |s| ~ 1e-3 are held to its error model, up to ~1e-6 |dP/ds| / |s|
    # on top of the bar (the ratio recorded is the error over twice the model).  At a scale below the floor (the exact zero) that
    # derivative carries no meaning in the closed family - only a finite value is required there; the composite, which does not
    # divide by the scale, is held to the ordinary bar on every channel
    a, b = got[7].double(), ref[7].detach()
    for t in got:
        assert torch.isfinite(t).all()
    floored = isc.abs() < 1e-20 if closed else torch.zeros_like(isc, dtype=torch.bool)
    small = (isc.abs() < 1e-2) & ~floored if closed else floored
    ordinary = ~small & ~floored
    scale = b[ordinary].abs().max()
    _record(route.name, 'closed d2isc', float((a - b)[ordinary].abs().max() / scale), SO_TOL)
    if closed:
        model = 1e-6 * ref[3].detach().abs()[small] / isc.double().abs()[small]
        excess = ((a - b)[small].abs() - SO_TOL * scale) / (2 * model)
        _record(route.name, 'closed d2isc small/model', float(excess.max().clamp_min(0)), 1.0)


# ------------------------------------------------------------------------------------------------ ResBlock
def _resblock(cin, cout, tag, far_from_kink):
    from transeditor_amd.model_spatial_query import ResBlock
    rb = ResBlock(cin, cout)
    sd = rb.state_dict()
    synth.fill_state_dict(sd, 5)
    for k in sd:
        if k.endswith('bias'):
            n = synth.normal(tuple(sd[k].shape), f'rt.rb.{k}.{tag}')
            # far_from_kink: biases well away from zero on both sides (+-4 at conv1, whose pre-activations are ~N(0, 1); +-20 at conv2).
            # The split skip routes need images of 16.7 M activations, where biases near zero leave pre-activations within fp32
            # round-off of the leaky-ReLU kink; their slope flips then dominate rel_l2 (3.8e-4 / 4.9e-4 measured for the split / fp32
            # skip route alike) and hide the kernels' error.  The small blocks keep ordinary biases, pre-activations on both sides
            sd[k].copy_(torch.sign(n) * ((4.0 if 'conv1' in k else 20.0) + 0.3 * n.abs()) if far_from_kink else 0.3 * n)
    rb.load_state_dict(sd)
    return rb.to(DEV)


def _blur64(x, k, pad, down=1):
    C = x.shape[1]
    kk = torch.flip(k.double(), [0, 1])[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(F.pad(x, (pad[0], pad[1], pad[0], pad[1])), kk, groups=C, stride=down)


def _resblock64(rb, x, P):
    c1, c2, sk = rb.conv1, rb.conv2, rb.skip
    g = 1 / SQRT2
    y1 = F.leaky_relu(F.conv2d(x, P['w1'] * c1[0].scale, padding=1) + P['b1'][None, :, None, None], 0.2) * SQRT2
    yb = _blur64(y1, c2[0].kernel, c2[0].pad)
    y2 = F.leaky_relu(F.conv2d(yb, P['w2'] * c2[1].scale, stride=2) + P['b2'][None, :, None, None], 0.2) * SQRT2 * g
    xs = _blur64(x, sk[0].kernel, sk[0].pad, down=2)
    return F.conv2d(xs, P['ws'] * sk[1].scale * g) + y2, (y1, y2)


SKIP = [r for r in cr.ROUTES if r.op == 'skip']


@pytest.mark.parametrize('offset', [False, True], ids=['dense', 'offset'])
@pytest.mark.parametrize('route', SKIP, ids=IDS)
def test_resblock_node(route, offset):
    """the discriminator's ResBlock node (skip branch on the entry's route; the split entry also has conv1 on 3X3W6 and conv2 on
    S2S6 / T2S6): forward, dx, every parameter gradient, and (dense inputs) an R1-style double backward"""
    B, K, M, H, W = route.shape
    with cr.switches(**route.switches) as mc:
        cr.check(route)
        if route.name in ('skip_p1s6', 'skip_fp32_split_convs'):
            w1, w2 = torch.empty(K, K, 3, 3), torch.empty(M, K, 3, 3)
            assert mc.fwd_kinds('3x3', B, w1, 2 * H, 2 * W)[1] == _lib.CONV_3X3W6
            assert mc.fwd_kinds('down', B, w2, H, W)[1] == _lib.CONV_S2S6 and mc.bwd_kinds('down', B, w2, H, W)[1] == _lib.CONV_T2S6
        rb = _resblock(K, M, route.name, far_from_kink=B * K * 4 * H * W > 2 ** 20)
        x = _gpu((B, K, 2 * H, 2 * W), 'rt.rbx.' + route.name, offset=offset)
        gy = _gpu((B, M, H, W), 'rt.rbg.' + route.name, offset=offset)
        names = ('w1', 'b1', 'w2', 'b2', 'ws')
        params = (rb.conv1[0].weight, rb.conv1[1].bias, rb.conv2[1].weight, rb.conv2[2].bias, rb.skip[1].weight)
        xd = x.detach().requires_grad_(True)
        out = rb(xd)
        assert 'ResBlock' in type(out.grad_fn).__name__
        got = torch.autograd.grad(out, (xd,) + params, gy)
        P = {n: p.detach().double().requires_grad_(True) for n, p in zip(names, params)}
        x64 = x.double().requires_grad_(True)
        ref, (y1, y2) = _resblock64(rb, x64, P)
        rg = torch.autograd.grad(ref, [x64] + [P[n] for n in names], gy.double(), retain_graph=True)
        sfx = ' (offset)' if offset else ''
        _record(route.name, 'rb out' + sfx, rel_err(out, ref), FWD_TOL)
        bars = {'dx': FWD_TOL, 'w1': red_tol(B * 4 * H * W), 'b1': red_tol(B * 4 * H * W), 'w2': red_tol(B * H * W),
                'b2': red_tol(B * H * W), 'ws': red_tol(B * H * W)}
        for n, a, b in zip(('dx',) + names, got, rg):
            _record(route.name, f'rb {n} l2{sfx}', rel_l2(a, b), bars[n])
            _record(route.name, f'rb {n}{sfx}', rel_err(a, b), bars[n])
        if offset:
            return
        # R1: d/dparams of || d<out, gy>/dx ||^2 through the node's recorded backward
        xd = x.detach().requires_grad_(True)
        out = rb(xd)
        gx, = torch.autograd.grad((out * gy).sum(), xd, create_graph=True)
        got2 = torch.autograd.grad(gx.pow(2).sum(), params)
    gx64, = torch.autograd.grad((ref * gy.double()).sum(), x64, create_graph=True)
    ref2 = torch.autograd.grad(gx64.pow(2).sum(), [P[n] for n in names])
    for n, a, b in zip(names, got2, ref2):
        _record(route.name, f'rb R1 d{n} l2', rel_l2(a, b), SO_TOL)
        _record(route.name, f'rb R1 d{n}', rel_err(a, b), SO_TOL)


# ------------------------------------------------------------------------------------------------ the bindings on offset views
@pytest.mark.parametrize('kind', ['1X1S6', '3X3W6'])
def test_conv_binding_takes_offset_operands(kind):
    """te_conv_f32's split kinds want 16-byte aligned activations / residuals: the binding hands them aligned ones"""
    if kind == '1X1S6':
        B, K, M, H, W, ks, pk = 2, 128, 128, 128, 128, 1, _lib.PACK_P6FWD
        assert _lib.p1s6_ok(B, K, M, H, W)
    else:
        B, K, M, H, W, ks, pk = 1, 64, 64, 8, 32, 3, _lib.PACK_W6FWD
        assert _lib.wino6_ok(B, K, M, H, W)
    x = _gpu((B, K, H, W), 'rt.bx.' + kind, offset=True)
    w = _gpu((M, K, ks, ks), 'rt.bw.' + kind, 1 / math.sqrt(K * ks * ks))
    res = _gpu((B, M, H, W), 'rt.br.' + kind, offset=True)
    got = _lib.conv(x, _lib.conv_pack(w, pk), getattr(_lib, 'CONV_' + kind), M, H, W, res=res)
    want = F.conv2d(x.double(), w.double(), padding=ks // 2) + res.double()
    _record('binding ' + kind, 'y (offset)', rel_err(got, want), FWD_TOL)

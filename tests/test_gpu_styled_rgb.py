"""The StyledConv + ToRGB training node (op/styled_rgb.py, `_ModConvRGB`) and the kernels only it reaches, against fp64.

A. te_bias_act_bwd_rgb_f32 (`bias_act_bwd_rgb_rows_kernel` + `bias_parts_sum_kernel`) at the binding, element by element against a
   round-off bound (not a norm), with te_bias_act_bwd_f32 through the same reference; the ABI's refusals as return codes.
B. The node against an fp64 restatement of the two layers: every branch of its backward (fused / unfused activation-gradient pass,
   each upstream gradient present or absent, `needs_input_grad` subsets, upstream gradients at a 4-byte storage offset, the recorded
   backward), at the `rgb_wgrad_kernel` geometries no other test reaches.  Each case asserts the branch it takes first.
C. `Generator._conv_rgb`: when the model builds the node, and that the separate-layer path it takes otherwise meets the same bars.

Bars.  A: 16 (fused) / 3 (plain) fp32 roundings of the element's own magnitude for `gi`; for `gb` the longest chain of additions (32 in
the row kernels, outer * inner / 256 + 9 in the per-channel kernel) against the fp64 sum of the kernel's own `gi`.  B, C: those of
test_gpu_conv_routes.py - 1e-5 for activations and data gradients, 2e-5 grown by sqrt(reduction length / 4096) for reductions, 1e-4
for the recorded backward.  The leaky-ReLU slope of the gradient reference is the node's own decision (`a > 0` on its output, the rule
of the kernel), checked against the fp64 pre-activation wherever that is further than 1e-4 from the kink.

Worst figures measured on the MI355X (the table printed at the end of the module, the three upstream variants of a quantity folded
into their worst; rel_err unless it says otherwise):
  A  te_bias_act_bwd_rgb_f32, ratio to the bound    gi 0.15 (1x1x32x32)  0.23 (2x5x32x36, 3x7x64x68)  0.20 (2x3x128x64)  0.22 (5x2x32x32)
                                                    gb 5.7e-3 at most (2x5x32x36)
     te_bias_act_bwd_f32, ratio to the bound        gi 0.52 - 0.55 on all seven cases (two roundings against the count 3)
                                                    gb 4.1e-3 at most (2x5x30x34, the per-channel kernel)
  B1 unfused        a 2.4e-7  rgb 2.1e-7  gx 4.2e-7  gw 1.7e-7  gs 2.1e-7  gbias 1.5e-7  gwr 1.5e-7  gsr 2.0e-7  gbr 5.9e-8
                    recorded backward: d2w 2.3e-7  d2s 5.5e-7  d2wr 1.6e-7  d2sr 1.9e-7 (rel_l2 4.3e-7 at most)
  B2 fused K2=16    a 3.4e-7  rgb 5.0e-7  gx 4.0e-7  gw 2.2e-7  gs 2.3e-7  gbias 1.1e-7  gwr 1.7e-7  gsr 2.6e-7  gbr 7.2e-8
                    recorded backward: d2w 3.6e-7  d2s 3.3e-7  d2wr 3.8e-7  d2sr 1.8e-7 (rel_l2 3.0e-7 at most)
  B3 ragged K2=64   a 4.1e-7  rgb 3.4e-7  gx 6.1e-7  gw 3.2e-7  gs 2.6e-7  gbias 1.7e-7  gwr 2.7e-7  gsr 2.8e-7  gbr 1.8e-7
  B4 K2=256 K<256   a 3.3e-7  rgb 3.7e-7  gx 4.6e-7  gw 2.5e-7  gs 2.4e-7  gbias 1.5e-7  gwr 2.4e-7  gsr 2.7e-7  gbr 2.0e-7
  B5 K2=512 tail    a 4.6e-7  rgb 4.7e-7  gx 4.1e-7  gw 2.9e-7  gs 4.4e-7  gbias 2.0e-7  gwr 2.1e-7  gsr 1.0e-7  gbr 1.3e-7
  B6 K=512 8 tiles  a 3.5e-7  rgb 8.3e-7  gx 4.5e-7  gw 2.1e-7  gs 2.8e-7  gbias 1.3e-7  gwr 1.9e-7  gsr 1.5e-7  gbr 6.1e-8
  (rel_l2 of every first-order gradient: 3.6e-7 at most.)  `needs_input_grad` subsets and offset upstream gradients: bit-identical
  to the all-leaves / aligned run in every gradient, so no case needed the 1e-6 allowance for another kernel form.
  C  node (with and without skip), second_order(), noise injection, no_grad: a 4.8e-7, rgb 5.2e-7, gx 3.5e-7, every parameter
     gradient 2.9e-7 at most (rel_l2 3.4e-7)
  bindings on offset views against fp64: rgb_fwd 1.7e-7, rgb_dgrad 8.8e-8, rgb_expand 1.1e-7, rgb_wgrad_slabs 1.1e-7; all four
  bit-identical to the aligned run (rgb_wgrad_slabs through the kernel's scalar staging path).
Before the bindings aligned their operands, test_node_offset_upstream_gradients failed with "te_bias_act_bwd_rgb_f32 failed (code -3):
16-byte aligned tensors required".
"""
import ctypes
import functools
import math
from collections import defaultdict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, rel_l2
from fp64_check import U32 as EPS32, off16
from transeditor_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SQRT2 = math.sqrt(2.0)

FWD_TOL = 1e-5
SO_TOL = 1e-4
WORST = defaultdict(float)


def red_tol(n):
    return 2e-5 * max(1.0, math.sqrt(n / 4096))


def _record(case, what, err, bar):
    key = (case, what)
    WORST[key] = max(WORST[key], err)
    assert err <= bar, f'{case}: {what} {err:.3e} > {bar:.1e}'


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nworst figures per case (tests/test_gpu_styled_rgb.py):')
    for (case, what), e in sorted(WORST.items()):
        print(f'  {case:34s} {what:24s} {e:.2e}')


def _f32(v):
    """the value a float argument has once it crossed the C ABI"""
    return float(np.float32(v))


def _gpu(shape, key, scale=1.0, offset=False):
    t = synth.normal(shape, key)
    if scale != 1.0:
        t = t * scale
    return off16(t, 4, DEV) if offset else t.to(DEV)


# ================================================================================================ A. the kernels at the binding
A_SHAPES = [(1, 1, 32, 32), (2, 5, 32, 36), (3, 7, 64, 68), (2, 3, 128, 64), (5, 2, 32, 32)]
A_ID = lambda s: 'x'.join(map(str, s))
A_WSCALE = 0.37


def _a_inputs(shape, offset=False):
    """g, ref (a few +0.0 / -0.0 elements: both take the slope alpha), grgb, wrgb (rows of scale 1 / 10 / 100), srgb"""
    n, C, H, W = shape
    tag = A_ID(shape)
    g = _gpu(shape, 'srgb.A.g.' + tag, offset=offset)
    ref = synth.normal(shape, 'srgb.A.ref.' + tag)
    flat = ref.view(-1)
    idx = torch.arange(0, flat.numel(), max(1, flat.numel() // 13))
    flat[idx[0::2]] = 0.0
    flat[idx[1::2]] = -0.0
    ref = off16(ref, 4, DEV) if offset else ref.to(DEV)
    grgb = _gpu((n, 3, H, W), 'srgb.A.grgb.' + tag)
    wrgb = (synth.normal((3, C), 'srgb.A.w.' + tag) * torch.tensor([1.0, 10.0, 100.0])[:, None]).to(DEV)
    srgb = (1 + 0.5 * synth.normal((n, C), 'srgb.A.s.' + tag)).to(DEV)
    return g, ref, grgb, wrgb, srgb


def _gi_ref(g, ref, grgb, wrgb, srgb, wscale, alpha, scale, roundings):
    """(gi in fp64 from the fp32 inputs, the element's round-off bound): gi = (g + sum_o coef_o grgb_o) * slope(ref) * scale"""
    acc = torch.zeros(ref.shape, dtype=torch.float64, device=ref.device)
    mag = torch.zeros_like(acc)
    if g is not None:
        acc, mag = acc + g.double(), mag + g.double().abs()
    if grgb is not None:
        s = srgb.double() if srgb is not None else torch.ones(ref.shape[:2], dtype=torch.float64, device=ref.device)
        coef = _f32(wscale) * s[:, None, :] * wrgb.double()[None]                               # [n, o, c]
        terms = coef[:, :, :, None, None] * grgb.double()[:, :, None]                            # [n, o, c, H, W]
        acc, mag = acc + terms.sum(1), mag + terms.abs().sum(1)
    slope = torch.where(ref > 0, 1.0, _f32(alpha)).double() * _f32(scale)
    return acc * slope, roundings * EPS32 * mag * slope


def _check_gi(case, got, want, bound):
    err = (got.double() - want).abs()
    assert bool((err[bound == 0] == 0).all())
    _record(case, 'gi / bound', float((err / bound.clamp_min(1e-300)).max()), 1.0)


def _check_gb(case, gb, gi, chain):
    """the reduction alone: against the fp64 sum of the kernel's own gi, `chain` = the longest chain of additions"""
    want = gi.double().sum((0, 2, 3))
    bound = chain * EPS32 * gi.double().abs().sum((0, 2, 3))
    _record(case, 'gb / bound', float(((gb.double() - want).abs() / bound.clamp_min(1e-300)).max()), 1.0)


@pytest.mark.parametrize('alpha,scale', [(0.2, SQRT2), (0.2, 1.0)], ids=['sqrt2', 'gain1'])
@pytest.mark.parametrize('with_s', [True, False], ids=['srgb', 'nosrgb'])
@pytest.mark.parametrize('with_g', [True, False], ids=['g', 'nog'])
@pytest.mark.parametrize('shape', A_SHAPES, ids=A_ID)
def test_bias_act_bwd_rgb_elementwise(shape, with_g, with_s, alpha, scale):
    """te_bias_act_bwd_rgb_f32: every gi element within 16 roundings of its own magnitude, gb within the 32-addition chain of the
    reduction; gb bit-identical from call to call; gi bit-identical with and without the bias gradient"""
    g, ref, grgb, wrgb, srgb = _a_inputs(shape)
    g, srgb = (g if with_g else None), (srgb if with_s else None)
    assert _lib.bias_act_bwd_rgb_supported(shape)
    gi, gb = _lib.bias_act_bwd_rgb(g, ref, grgb, wrgb, srgb, A_WSCALE, alpha, scale, want_bias=True)
    gi2, gb2 = _lib.bias_act_bwd_rgb(g, ref, grgb, wrgb, srgb, A_WSCALE, alpha, scale, want_bias=True)
    gi3, gb3 = _lib.bias_act_bwd_rgb(g, ref, grgb, wrgb, srgb, A_WSCALE, alpha, scale, want_bias=False)
    assert gb3 is None and gb.shape == (shape[1],)
    assert torch.equal(gb, gb2) and torch.equal(gi, gi2) and torch.equal(gi, gi3)
    want, bound = _gi_ref(g, ref, grgb, wrgb, srgb, A_WSCALE, alpha, scale, 16)
    case = 'A rgb ' + A_ID(shape)
    _check_gi(case, gi, want, bound)
    _check_gb(case, gb, gi, 32)


PLAIN = [pytest.param(s, False, id=A_ID(s)) for s in A_SHAPES] + [pytest.param((2, 5, 30, 34), False, id='2x5x30x34'),
                                                                  pytest.param((3, 7, 64, 68), True, id='3x7x64x68-offset')]


@pytest.mark.parametrize('alpha,scale', [(0.2, SQRT2), (0.2, 1.0)], ids=['sqrt2', 'gain1'])
@pytest.mark.parametrize('shape,offset', PLAIN)
def test_bias_act_bwd_plain_elementwise(shape, offset, alpha, scale):
    """te_bias_act_bwd_f32 through the same reference with the ToRGB term absent: the row kernel (the five shapes), the per-channel
    kernel by shape (inner = 1020) and by misalignment (operands 4 bytes into their storage)"""
    g, ref, _, _, _ = _a_inputs(shape, offset)
    n, C, H, W = shape
    rows = bool(_lib.lib().te_bias_act_bwd_ws_floats(n, C, H * W) > 0) and not offset
    assert rows == (shape in A_SHAPES and not offset)
    gi, gb = _lib.bias_act_bwd(g, ref, alpha, scale, want_bias=True)
    gi2, gb2 = _lib.bias_act_bwd(g, ref, alpha, scale, want_bias=True)
    gi3, gb3 = _lib.bias_act_bwd(g, ref, alpha, scale, want_bias=False)
    assert gb3 is None and torch.equal(gb, gb2) and torch.equal(gi, gi2) and torch.equal(gi, gi3)
    want, bound = _gi_ref(g, ref, None, None, None, 1.0, alpha, scale, 3)
    case = 'A plain ' + A_ID(shape) + (' offset' if offset else '')
    _check_gi(case, gi, want, bound)
    # per-channel kernel: one thread adds up to ceil(outer * inner / 256) terms in sequence, then 6 + 3 in the block's tree
    _check_gb(case, gb, gi, 32 if rows else -(-n * H * W // 256) + 9)


def test_bias_act_bwd_rgb_refusals():
    """the ABI refuses, before any launch: inner % 4 != 0, inner < 1024, a gi / ref / grgb pointer 4 bytes off, gb without a
    workspace.  Return codes only; the outputs keep their sentinel"""
    L = _lib.lib()
    P = ctypes.c_void_p
    SENT = -77.0

    def call(shape, off=None, ws=True, gb=True):
        n, C, H, W = shape
        inner = H * W
        t = {k: torch.full((n * (3 if k == 'grgb' else C) * inner + 1,), SENT, device=DEV) for k in ('gi', 'g', 'ref', 'grgb')}
        ptr = {k: v.data_ptr() + (4 if k == off else 0) for k, v in t.items()}
        wrgb, gbt, wst = torch.ones(3, C, device=DEV), torch.full((C,), SENT, device=DEV), torch.full((n * C * 8,), SENT, device=DEV)
        rc = L.te_bias_act_bwd_rgb_f32(P(ptr['gi']), P(gbt.data_ptr()) if gb else None, P(wst.data_ptr()) if ws else None,
                                       P(ptr['g']), P(ptr['ref']), P(ptr['grgb']), P(wrgb.data_ptr()), None, 1.0, 0.2, 1.0,
                                       n, C, inner, P(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for v in (t['gi'], gbt, wst):
            assert bool((v == SENT).all()), 'a refused call wrote to its outputs'
        return rc

    ok = (2, 3, 32, 32)
    assert L.te_bias_act_bwd_rgb_supported(2, 3, 1024) == 1 and _lib.bias_act_bwd_rgb_supported(ok)
    for shape in ((2, 5, 30, 34), (2, 3, 16, 32)):                      # inner = 1020, inner = 512
        n, C, H, W = shape
        assert L.te_bias_act_bwd_rgb_supported(n, C, H * W) == 0 and not _lib.bias_act_bwd_rgb_supported(shape)
        assert call(shape) == -3
        assert b'inner' in L.te_last_error_string()
    for off in ('gi', 'ref', 'grgb', 'g'):
        assert call(ok, off=off) == -3, off
        assert b'aligned' in L.te_last_error_string()
    assert call(ok, ws=False) == -1
    assert b'workspace' in L.te_last_error_string()


# ================================================================================================ B. the node
# (B, Ci, Co, H, W), fused activation-gradient pass?, what the case is for
B_CASES = [((2, 8, 12, 16, 16), False, 'unfused'),
           ((2, 8, 12, 32, 32), True, 'fused K2=16'),
           ((3, 16, 40, 32, 36), True, 'fused ragged K2=64'),
           ((1, 8, 130, 32, 32), True, 'K2=256 K<256'),
           ((1, 8, 300, 32, 32), True, 'K2=512 tail'),
           ((2, 8, 512, 16, 16), False, 'K=512 8 tiles')]
B_EPS = 1e-8
LEAVES = ('x', 'w', 's', 'bias', 'wr', 'sr', 'br')
# keys of the recorded-backward test, chosen on the CPU so that no pre-activation is within 1e-5 of the kink
SO_KEYS = {0: 'so0', 1: 'so13'}


def _b_name(i):
    return f'B{i + 1} ' + B_CASES[i][2]


def b_inputs(i, key='fo'):
    """fp32 CPU leaves and upstream gradients of case i (a pure function of (i, key))"""
    B, Ci, Co, H, W = B_CASES[i][0]
    k = f'srgb.B{i}.{key}.'
    t = dict(x=synth.normal((B, Ci, H, W), k + 'x'), w=synth.normal((Co, Ci, 3, 3), k + 'w'),
             s=1 + 0.5 * synth.normal((B, Ci), k + 's'), bias=0.3 * synth.normal((Co,), k + 'bias'),
             wr=synth.normal((3, Co, 1, 1), k + 'wr'), sr=1 + 0.5 * synth.normal((B, Co), k + 'sr'),
             br=0.3 * synth.normal((3,), k + 'br'), ga=synth.normal((B, Co, H, W), k + 'ga'),
             grgb=synth.normal((B, 3, H, W), k + 'grgb'))
    return t, (1 / math.sqrt(9 * Ci), B_EPS, 1 / math.sqrt(Co))


def _slope(mask, dtype):
    return torch.where(mask, torch.ones((), dtype=dtype), torch.full((), 0.2, dtype=dtype))


def restate64(x, w, s, bias, wr, sr, br, cfg, mask=None):
    """the two layers from stock ops, in the dtype of the operands (fp64).  mask: the leaky-ReLU decision taken as a constant;
    None: the true leaky-ReLU.  -> (pre, a, rgb)"""
    wscale, eps, wscale_r = cfg
    ws = w * wscale
    d = torch.rsqrt((ws[None] * s[:, None, :, None, None]).square().sum(dim=(2, 3, 4)) + eps)
    pre = d[:, :, None, None] * F.conv2d(x * s[:, :, None, None], ws, padding=1) + bias[None, :, None, None]
    if mask is None:
        a = F.leaky_relu(pre, 0.2) * SQRT2
    else:
        a = pre * _slope(mask, pre.dtype) * SQRT2
    rgb = F.conv2d(a * sr[:, :, None, None], wr * wscale_r) + br[None, :, None, None]
    return pre, a, rgb


def _node(leaves, cfg):
    from transeditor_amd.op import styled_rgb
    return styled_rgb.styled_conv_rgb(*leaves, *cfg)


def _is_node(t):
    return t.grad_fn is not None and '_ModConvRGB' in type(t.grad_fn).__name__


def _dev_leaves(t, needs=LEAVES):
    return [t[n].to(DEV).requires_grad_(n in needs) for n in LEAVES]


def _red_len(i):
    B, Ci, Co, H, W = B_CASES[i][0]
    return dict(gx=None, gw=B * H * W, gs=H * W, gbias=B * H * W, gwr=B * H * W, gsr=H * W, gbr=B * H * W)


@functools.lru_cache(maxsize=None)
def _b_case(i):
    """case i once: the node's forward and its three first-order backwards on the GPU, the fp64 restatement with the node's own mask
    on the CPU.  The branch assertions come before any comparison"""
    from transeditor_amd.op import styled_rgb
    shape, fused, _ = B_CASES[i]
    B, Ci, Co, H, W = shape
    t, cfg = b_inputs(i)
    leaves = _dev_leaves(t)
    assert styled_rgb.supported(leaves[0], leaves[1], leaves[4])
    a, rgb = _node(leaves, cfg)
    assert _lib.bias_act_bwd_rgb_supported(a.shape) == fused
    assert _is_node(a) and rgb.grad_fn is a.grad_fn
    ga, grgb = t['ga'].to(DEV), t['grgb'].to(DEV)
    got = {'both': torch.autograd.grad([a, rgb], leaves, [ga, grgb], retain_graph=True),
           'a': torch.autograd.grad(a, leaves, ga, retain_graph=True, allow_unused=True),
           'rgb': torch.autograd.grad(rgb, leaves, grgb, allow_unused=True)}
    mask = (a.detach() > 0).cpu()
    L64 = [t[n].double().requires_grad_(True) for n in LEAVES]
    pre, a64, rgb64 = restate64(*L64, cfg, mask=mask)
    _, a_true, rgb_true = restate64(*[v.detach() for v in L64], cfg)
    ga64, grgb64 = t['ga'].double(), t['grgb'].double()
    ref = {'both': torch.autograd.grad([a64, rgb64], L64, [ga64, grgb64], retain_graph=True),
           'a': torch.autograd.grad(a64, L64, ga64, retain_graph=True, allow_unused=True),
           'rgb': torch.autograd.grad(rgb64, L64, grgb64, allow_unused=True)}
    return dict(a=a.detach(), rgb=rgb.detach(), got=got, ref=ref, pre=pre.detach(), a_true=a_true, rgb_true=rgb_true, mask=mask,
                t=t, cfg=cfg)


@pytest.mark.parametrize('i', range(len(B_CASES)), ids=_b_name)
def test_node_forward(i):
    """a and rgb against the true fp64 leaky-ReLU; the node's slope decision equals the sign of the fp64 pre-activation wherever
    that is further than 1e-4 from zero, and both slopes occur in every channel"""
    c = _b_case(i)
    _record(_b_name(i), 'a', rel_err(c['a'], c['a_true']), FWD_TOL)
    _record(_b_name(i), 'rgb', rel_err(c['rgb'], c['rgb_true']), FWD_TOL)
    clear = c['pre'].abs() > 1e-4
    assert torch.equal(c['mask'][clear], (c['pre'] > 0)[clear])
    per_channel = c['mask'].float().mean(dim=(0, 2, 3))
    assert float(per_channel.min()) > 0 and float(per_channel.max()) < 1
    if B_CASES[i][0][2] == 512:        # the plan of rgb_wgrad_kernel at K = 512: 32-pixel tiles, one slab per tile
        B, _, Co, H, W = B_CASES[i][0]
        assert _lib.lib().te_rgb_wgrad_slab_count(B, Co, H * W) == H * W // 32 == 8


@pytest.mark.parametrize('up', ['both', 'a', 'rgb'])
@pytest.mark.parametrize('i', range(len(B_CASES)), ids=_b_name)
def test_node_first_order(i, up):
    """every gradient of the node for [a, rgb] with both upstream gradients, for `a` alone (no ToRGB gradient: gwr, gsr, gbr are
    None) and for `rgb` alone (the kernel's g is NULL) - three branches, since the node does not materialise absent gradients"""
    c = _b_case(i)
    got, ref, n = c['got'][up], c['ref'][up], _red_len(i)
    for name, a, b in zip(n, got, ref):
        if up == 'a' and name in ('gwr', 'gsr', 'gbr'):
            assert a is None and b is None, name
            continue
        bar = FWD_TOL if n[name] is None else red_tol(n[name])
        _record(_b_name(i), f'{name} [{up}]', rel_err(a, b), bar)
        _record(_b_name(i), f'{name} [{up}] l2', rel_l2(a, b), bar)


SUBSETS = {'only x': ('x',), 'all but x': ('w', 's', 'bias', 'wr', 'sr', 'br'), 'all but bias': ('x', 'w', 's', 'wr', 'sr', 'br'),
           'all but wr, sr': ('x', 'w', 's', 'bias', 'br'), 'only br': ('br',)}


@pytest.mark.parametrize('subset', SUBSETS, ids=lambda s: s.replace(' ', '_').replace(',', ''))
@pytest.mark.parametrize('i', [0, 1], ids=_b_name)
def test_node_needs_input_grad_subsets(i, subset):
    """leaves that do not require a gradient change which kernels run (no backward weight pack, want_bias = False, no ToRGB slabs),
    never a value: every returned gradient is bit-identical to the one of the all-leaves run.  bias / br and s / sr have equal or
    similar shapes, so a gradient in the wrong slot shows only in its values"""
    c = _b_case(i)
    needs = SUBSETS[subset]
    leaves = _dev_leaves(c['t'], needs)
    a, rgb = _node(leaves, c['cfg'])
    assert _is_node(a) and torch.equal(a, c['a']) and torch.equal(rgb, c['rgb'])
    got = torch.autograd.grad([a, rgb], [l for l in leaves if l.requires_grad], [c['t']['ga'].to(DEV), c['t']['grgb'].to(DEV)])
    full = dict(zip(LEAVES, c['got']['both']))
    for name, g in zip(needs, got):
        _record(_b_name(i), f'subset [{subset}] vs all', rel_err(g, full[name]), 0.0)
        assert torch.equal(g, full[name]), name


def test_node_offset_upstream_gradients():
    """upstream gradients that are contiguous views 4 bytes into their storage (case 2, the fused kernel with its 16-byte
    accesses): the binding hands te_bias_act_bwd_rgb_f32 aligned copies, the results are bit-identical to the aligned run"""
    c = _b_case(1)
    leaves = _dev_leaves(c['t'])
    a, rgb = _node(leaves, c['cfg'])
    ga, grgb = off16(c['t']['ga'], 4, DEV), off16(c['t']['grgb'], 4, DEV)
    assert ga.data_ptr() % 16 == 4 and grgb.data_ptr() % 16 == 4
    got = torch.autograd.grad([a, rgb], leaves, [ga, grgb])
    for name, g, want in zip(LEAVES, got, c['got']['both']):
        assert torch.equal(g, want), name


def _rgb_binding_operands():
    B, K, H, W = 2, 12, 32, 32
    x = synth.normal((B, K, H, W), 'srgb.off.x')
    g = synth.normal((B, 3, H, W), 'srgb.off.g')
    w = (synth.normal((3, K), 'srgb.off.w') / math.sqrt(K)).to(DEV)
    isc = (1 + 0.5 * synth.normal((B, K), 'srgb.off.i')).to(DEV)
    bias3, biask = synth.normal((3,), 'srgb.off.b3').to(DEV), synth.normal((K,), 'srgb.off.bk').to(DEV)
    return x, g, w, isc, bias3, biask


@pytest.mark.parametrize('which', ['rgb_fwd', 'rgb_dgrad', 'rgb_expand', 'rgb_wgrad_slabs'])
def test_rgb_bindings_take_offset_operands(which):
    """the ToRGB bindings on activation operands 4 bytes into their storage.  rgb_fwd / rgb_dgrad / rgb_expand read them with 16-byte
    accesses: the binding hands the kernel aligned copies (bit-identical results).  rgb_wgrad_slabs passes them on: its kernel takes
    the scalar staging path, which fills the same LDS tile, so its slabs are bit-identical too"""
    x, g, w, isc, bias3, biask = _rgb_binding_operands()
    ws = 0.6

    def run(x, g):
        if which == 'rgb_fwd':
            return _lib.rgb_fwd(x, w, isc, bias3, ws)
        if which == 'rgb_dgrad':
            return _lib.rgb_dgrad(g, w, isc, w.shape[1], ws)
        if which == 'rgb_expand':
            return _lib.rgb_expand(g, w, biask, 3, ws)
        return _lib.rgb_wgrad_slabs(g, x)

    dense = run(x.to(DEV), g.to(DEV))
    xo, go = off16(x, 4, DEV), off16(g, 4, DEV)
    assert xo.data_ptr() % 16 == 4 and go.data_ptr() % 16 == 4
    off = run(xo, go)
    assert torch.equal(off, dense)
    x64, g64, w64, i64 = x.double(), g.double(), w.double().cpu() * ws, isc.double().cpu()
    if which == 'rgb_fwd':
        want = torch.einsum('ok,bk,bkhw->bohw', w64, i64, x64) + bias3.double().cpu()[None, :, None, None]
    elif which == 'rgb_dgrad':
        want = torch.einsum('ok,bk,bohw->bkhw', w64, i64, g64)
    elif which == 'rgb_expand':
        want = F.leaky_relu(torch.einsum('ok,bohw->bkhw', w64, g64) + biask.double().cpu()[None, :, None, None], 0.2) * SQRT2
    else:
        want = torch.einsum('bohw,bkhw->bok', g64, x64)
        off = off.sum(dim=1).reshape(want.shape)
    _record('binding ' + which, 'offset vs fp64', rel_err(off, want), FWD_TOL if which != 'rgb_wgrad_slabs' else red_tol(32 * 32))


def _second_order(fn, leaves, ga, grgb):
    """d/d(w, s, wr, sr) of |dL/dx|^2 + |dL/ds|^2, L = <a, ga> + <rgb, grgb>"""
    a, rgb = fn(leaves)
    x, w, s, _, wr, sr, _ = leaves
    gx, gs = torch.autograd.grad((a * ga).sum() + (rgb * grgb).sum(), (x, s), create_graph=True)
    return (gx, gs) + torch.autograd.grad(gx.pow(2).sum() + gs.pow(2).sum(), (w, s, wr, sr))


def so_reference(i):
    """the fp64 side of the recorded-backward test and the smallest |pre-activation| of its inputs (CPU only)"""
    t, cfg = b_inputs(i, SO_KEYS[i])
    L64 = [t[n].double().requires_grad_(True) for n in LEAVES]
    pre = restate64(*[v.detach() for v in L64], cfg)[0]
    return _second_order(lambda L: restate64(*L, cfg)[1:], L64, t['ga'].double(), t['grgb'].double()), float(pre.abs().min())


@pytest.mark.parametrize('i', [0, 1], ids=_b_name)
def test_node_recorded_backward(i):
    """create_graph through the node (the composite of the two layers on the closed convolution family), then the gradients of
    |dL/dx|^2 + |dL/ds|^2 w.r.t. (w, s, wr, sr), against the same expression on the fp64 restatement with the true leaky-ReLU.
    A flipped slope would matter here: the inputs (synth keys 'srgb.B0.so0.*' for case 1, 'srgb.B1.so13.*' for case 2: SO_KEYS,
    the first whose fp64 pre-activations all stay further than 1e-4 from the kink) have a smallest |pre-activation| of 1.77e-4 /
    2.81e-4, asserted > 1e-5"""
    ref, pre_min = so_reference(i)
    assert pre_min > 1e-5
    t, cfg = b_inputs(i, SO_KEYS[i])
    leaves = _dev_leaves(t)
    got = _second_order(lambda L: _node(L, cfg), leaves, t['ga'].to(DEV), t['grgb'].to(DEV))
    for name, a, b in zip(('gx', 'gs', 'd2w', 'd2s', 'd2wr', 'd2sr'), got, ref):
        bar = SO_TOL if name.startswith('d2') else (FWD_TOL if name == 'gx' else red_tol(B_CASES[i][0][3] * B_CASES[i][0][4]))
        _record(_b_name(i), 'recorded ' + name, rel_err(a, b), bar)
        _record(_b_name(i), 'recorded ' + name + ' l2', rel_l2(a, b), bar)


def test_node_supported_predicate():
    from transeditor_amd.op import styled_rgb

    def sup(B, Ci, Co, H, W, rows=3):
        return styled_rgb.supported(torch.empty(B, Ci, H, W, device=DEV), torch.empty(Co, Ci, 3, 3, device=DEV),
                                    torch.empty(rows, Co, 1, 1, device=DEV))

    assert sup(2, 8, 12, 16, 16)
    assert not sup(2, 8, 12, 15, 15)          # H * W % 4 != 0
    assert not sup(2, 8, 12, 16, 16, rows=4)
    assert not sup(65, 8, 12, 16, 16)


# ================================================================================================ C. the model's choice of the node
STYLE_DIM = 32


def _layers(noise_injection):
    from transeditor_amd.model_spatial_query import StyledConv, ToRGB
    conv = StyledConv(8, 12, 3, STYLE_DIM, layer_noise_injection=noise_injection)
    to_rgb = ToRGB(12, STYLE_DIM)
    for tag, m in (('conv', conv), ('rgb', to_rgb)):
        sd = m.state_dict()
        synth.fill_state_dict({f'srgb.C.{tag}.{k}': v for k, v in sd.items()}, 3)
        m.load_state_dict(sd)
    with torch.no_grad():
        conv.activate.bias.mul_(3.0)       # 0.3 * normal: both slopes in every channel
    return conv.to(DEV), to_rgb.to(DEV)


def _upsample64(skip, k):
    """Upsample.forward: zero insertion by 2, then the 4-tap FIR (times 4) with padding (2, 1)"""
    B, C, H, W = skip.shape
    z = torch.zeros(B, C, 2 * H, 2 * W, dtype=skip.dtype)
    z[:, :, ::2, ::2] = skip
    kk = torch.flip(k.double().cpu(), [0, 1])[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(F.pad(z, (2, 1, 2, 1)), kk, groups=C)


def _has_node(t):
    seen, todo = set(), [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if '_ModConvRGB' in type(f).__name__:
            return True
        todo += [n for n, _ in f.next_functions]
    return False


def _model_case(mode, with_skip):
    """one call of Generator._conv_rgb against the fp64 restatement from the modules' parameters"""
    from transeditor_amd.model_spatial_query import Generator
    from transeditor_amd.op import modconv as mc
    B, H, W = 2, 32, 32
    conv, to_rgb = _layers(mode == 'noise')
    m, mr = conv.conv, to_rgb.conv
    x = _gpu((B, 8, H, W), 'srgb.C.x')
    lat_c, lat_r = _gpu((B, STYLE_DIM), 'srgb.C.lc'), _gpu((B, STYLE_DIM), 'srgb.C.lr')
    skip = _gpu((B, 3, H // 2, W // 2), 'srgb.C.skip') if with_skip else None
    noise = _gpu((B, 1, H, W), 'srgb.C.noise')
    ga, grgb = _gpu((B, 12, H, W), 'srgb.C.ga'), _gpu((B, 3, H, W), 'srgb.C.grgb')
    params = dict(w=m.weight, mw=m.modulation.weight, mb=m.modulation.bias, bias=conv.activate.bias, wr=mr.weight,
                  mrw=mr.modulation.weight, mrb=mr.modulation.bias, br=to_rgb.bias)
    if mode == 'noise':
        params['nw'] = conv.noise.weight
    xd = x.detach().requires_grad_(mode != 'no_grad')
    call = lambda: Generator._conv_rgb(None, conv, to_rgb, xd, lat_c, lat_r, skip, noise)
    if mode == 'no_grad':
        with torch.no_grad():
            out, rgb = call()
        assert out.grad_fn is None and rgb.grad_fn is None
    elif mode == 'second_order':
        with mc.second_order():
            out, rgb = call()
    else:
        out, rgb = call()
    if mode == 'node':
        assert _is_node(out) and _has_node(rgb)
    else:
        assert not _has_node(out) and not _has_node(rgb)
    # fp64 restatement (CPU), the slope decision of the path under test taken as a constant for the gradients
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in params.items()}
    x64 = x.double().cpu().requires_grad_(True)
    s = F.linear(lat_c.double().cpu(), P['mw'] * m.modulation.scale, P['mb'] * m.modulation.lr_mul)
    sr = F.linear(lat_r.double().cpu(), P['mrw'] * mr.modulation.scale, P['mrb'] * mr.modulation.lr_mul)
    cfg = (m.scale, m.eps, mr.scale)
    mask = (out.detach() > 0).cpu()

    def two_layers(mask):
        w64 = P['w'][0]
        ws = w64 * cfg[0]
        d = torch.rsqrt((ws[None] * s[:, None, :, None, None]).square().sum(dim=(2, 3, 4)) + cfg[1])
        pre = d[:, :, None, None] * F.conv2d(x64 * s[:, :, None, None], ws, padding=1)
        if mode == 'noise':
            pre = pre + P['nw'] * noise.double().cpu()
        pre = pre + P['bias'][None, :, None, None]
        a = F.leaky_relu(pre, 0.2) * SQRT2 if mask is None else pre * _slope(mask, pre.dtype) * SQRT2
        r = F.conv2d(a * sr[:, :, None, None], P['wr'][0] * cfg[2]) + P['br']
        if with_skip:
            r = r + _upsample64(skip.double().cpu(), to_rgb.upsample.kernel)
        return pre, a, r

    with torch.no_grad():
        pre, a_true, rgb_true = two_layers(None)
    case = f'C {mode}' + (' skip' if with_skip else '')
    _record(case, 'a', rel_err(out, a_true), FWD_TOL)
    _record(case, 'rgb', rel_err(rgb, rgb_true), FWD_TOL)
    clear = pre.abs() > 1e-4
    assert torch.equal(mask[clear], (pre > 0)[clear])
    if mode == 'no_grad':
        return
    names = list(params)
    got = torch.autograd.grad([out, rgb], [xd] + [params[k] for k in names], [ga, grgb])
    _, a64, rgb64 = two_layers(mask)
    ref = torch.autograd.grad([a64, rgb64], [x64] + [P[k] for k in names], [ga.double().cpu(), grgb.double().cpu()])
    n = dict(x=None, w=B * H * W, mw=H * W, mb=H * W, bias=B * H * W, wr=B * H * W, mrw=H * W, mrb=H * W, br=B * H * W,
             nw=B * 12 * H * W)
    for name, a, b in zip(['x'] + names, got, ref):
        bar = FWD_TOL if n[name] is None else red_tol(n[name])
        _record(case, 'g' + name, rel_err(a, b), bar)
        _record(case, 'g' + name + ' l2', rel_l2(a, b), bar)


@pytest.mark.parametrize('with_skip', [False, True], ids=['noskip', 'skip'])
def test_model_builds_the_node(with_skip):
    """gradients on, no noise injection, first order: Generator._conv_rgb runs the two layers as the node; outputs, dx and every
    parameter gradient (the two modulation layers included) against fp64, with and without the up-sampled skip image"""
    _model_case('node', with_skip)


@pytest.mark.parametrize('mode', ['second_order', 'noise', 'no_grad'])
def test_model_separate_layers(mode):
    """under second_order(), with layer_noise_injection and under torch.no_grad() the node is not built, and the separate-layer
    path meets the same bars against the same reference"""
    _model_case(mode, True)

"""Modulated convolution on the te_conv / te_wgrad kernels (reference: ModulatedConv2d.forward,
model_spatial_query.py:296-337).

Formulation: with ONE shared weight w (already multiplied by the
equalised-lr scale), style scale s[b,ci] and demodulation d[b,co],

    y[b,co] = d[b,co] * conv(s[b,ci] * x[b,ci], w)[co]        (+ bias, leaky-ReLU fused)

instead of the reference's B materialised weight copies + grouped convolution.

Two layers of autograd functions:

* ``_Fwd`` / ``_Dgrad`` / ``_Wgrad`` — the convolution with optional style and demodulation
  scales inside the kernels, a family closed under differentiation (each one's backward is
  expressed with the other two), so anything built on them is differentiable to any order
  (R1 / path-length regularisers).  ``conv_core`` enters it without scales (the plain bilinear
  convolution), ``modconv_closed`` with them.
* ``modconv`` (``_ModConvFused``) — the fast path: scales, bias and activation fused into the
  kernels, a hand-written backward that produces dx, dW, ds, dd from ONE data-gradient conv and
  ONE correlation pass (per-sample slabs + te_wgrad_reduce; ``_modconv_bwd``).  When its backward
  is itself being recorded (create_graph) it re-derives the gradients through the differentiable
  family (``recorded_backward``), so double backward stays exact.

The hints of the regulariser steps (``second_order()``, ``no_weight_grads()``) and their per-thread
state live in op/recorded.py and are re-exported here; the packed-weight and frozen-weight caches
live in op/weight_cache.py.

kinds: '3x3' (stride 1, pad 1), '1x1', 'up' (3x3 transposed stride 2 -> (2H+1)x(2W+1); the blur
that follows in the reference, model_spatial_query.py:318-321, is a separate upfirdn2d), 'down' (3x3 stride 2,
pad 0 over a (2H+1)x(2W+1) input -> HxW: the discriminator's blurred downsampling conv, :744-768; it is the
adjoint kernel pair of 'up').
"""
import os

import torch
from torch.autograd import Function

from .. import _lib
from .chanscale import _ChanDot, chan_scale
from .fused_act import fused_leaky_relu
# the hints of the regulariser steps live in op/recorded.py (state, threading note); callers reach them through this module too
from .recorded import (_DEFAULT_GRAPH, _STATE, current_graph, latent_producer_section, no_weight_grads, recorded_backward,      # noqa: F401
                       second_order, weights_skipped)
from .style import demod
from .weight_cache import _CACHES, cache_of, frozen_entry, keep_cache, packed, packed2


def _modconv_frozen(x, w, isc, osc, bias, act, kind, wscale, demod_eps):
    """forward only, weights taken from the frozen cache (no autograd node is created)"""
    H, W = _lowres_hw(kind, False, x)
    pk, ck = fwd_kinds(kind, x.shape[0], w, H, W)
    ent = frozen_entry(w, kind, wscale, demod_eps is not None, pk)
    if demod_eps is not None:
        osc = _lib.demod_from_wsq(ent['wsq'], isc, demod_eps)
    if _rgb_ok(kind, w.shape[0], w.shape[1], x, osc, act):
        return _lib.rgb_fwd(x, w.reshape(w.shape[0], w.shape[1]), isc, bias, wscale)
    return _lib.conv(x, ent['wp'], ck, w.shape[0], H, W, isc, osc, bias, _act_code(act))


_SQRT2 = 2 ** 0.5


def _act_gain(act):
    """`act` is False, True (the reference's lrelu * sqrt(2)) or the gain itself (sqrt(2) or 1.0)."""
    return _SQRT2 if act is True else float(act)


def _act_code(act):
    if not act:
        return 0
    g = _act_gain(act)
    if abs(g - _SQRT2) < 1e-6:
        return 3
    if abs(g - 1.0) < 1e-6:
        return 4
    raise RuntimeError(f'modconv: leaky-ReLU gain {g} is not one the kernels fuse (sqrt(2) or 1)')


def _lowres_hw(kind, is_output, t):
    """low-resolution (H, W) of the problem from the conv input (is_output=False) or output (True)."""
    H, W = t.shape[2], t.shape[3]
    if (kind == 'up' and is_output) or (kind == 'down' and not is_output):
        if H % 2 == 0 or W % 2 == 0:
            raise RuntimeError(f"kind '{kind}': high-resolution side must be (2H+1)x(2W+1), got {H}x{W}")
        return (H - 1) // 2, (W - 1) // 2
    return H, W


# Which kernel a convolution runs on, and which packed weight layout that kernel reads: decided by conv_route below from these tables
# and nowhere else.  The module switches are for A/B measurements; they are named in _ROUTES and read when a route is asked for, so an
# assignment at run time (tests, tools, the benchmark) takes effect at the next launch.
USE_WINOGRAD = True      # False: the direct 3x3 kernel everywhere
# TE_SPLIT_BF16=0 (or False here; written through set_split_bf16): fp32 matrix instructions everywhere.  The three below keep one family
# of launches on them while the others keep the split-bf16 form (TE_SPLIT_S2 / _T2 / _1X1 = 0)
USE_SPLIT_BF16 = os.environ.get('TE_SPLIT_BF16', '1') != '0'
USE_SPLIT_S2 = os.environ.get('TE_SPLIT_S2', '1') != '0'
USE_SPLIT_T2 = os.environ.get('TE_SPLIT_T2', '1') != '0'
USE_SPLIT_1X1 = os.environ.get('TE_SPLIT_1X1', '1') != '0'

# op -> (the fp32 kind, which covers every shape; the kinds preferred to it, best first: (switches that must all be on, the library's
# host predicate (B, K = input channels, M = output channels, H, W = low-resolution size), kind)).  'plain1x1' is the 1x1 product
# without scales, bias or activation, at most a residual: the skip branch of the discriminator's ResBlocks (op/resblock.py).
_ROUTES = {
    # 1-D Winograd F(2,3) (csrc/wino.hip: 2/3 of the MFMAs, same result to fp32 round-off), on the bf16 matrix pipe where the
    # three-piece split form covers the shape (csrc/wino6.hip: fp32-equivalent results)
    '3x3': (_lib.CONV_3X3, ((('USE_WINOGRAD', 'USE_SPLIT_BF16'), _lib.wino6_ok, _lib.CONV_3X3W6),
                            (('USE_WINOGRAD',), _lib.wino_ok, _lib.CONV_3X3W))),
    'down': (_lib.CONV_S2, ((('USE_SPLIT_BF16', 'USE_SPLIT_S2'), _lib.s2s6_ok, _lib.CONV_S2S6),)),          # csrc/s2s6.hip
    'up': (_lib.CONV_T2, ((('USE_SPLIT_BF16', 'USE_SPLIT_T2'), _lib.t2s6_ok, _lib.CONV_T2S6),)),            # csrc/t2s6.hip
    '1x1': (_lib.CONV_1X1, ()),
    'plain1x1': (_lib.CONV_1X1, ((('USE_SPLIT_BF16', 'USE_SPLIT_1X1'), _lib.p1s6_ok, _lib.CONV_1X1S6),)),   # csrc/p1s6.hip
}
# the data gradient of an op is the forward of its adjoint from Co to Ci channels: strided <-> transposed, the others their own
_ADJOINT = {'3x3': '3x3', 'down': 'up', 'up': 'down', '1x1': '1x1', 'plain1x1': 'plain1x1'}
# kind launched -> weight layout it reads (as a forward, as a data gradient)
_PACK = {
    _lib.CONV_3X3: (_lib.PACK_FWD, _lib.PACK_DGRAD), _lib.CONV_1X1: (_lib.PACK_FWD, _lib.PACK_DGRAD),
    _lib.CONV_T2: (_lib.PACK_FWD, _lib.PACK_SWAP), _lib.CONV_S2: (_lib.PACK_FWD, _lib.PACK_SWAP),
    _lib.CONV_3X3W: (_lib.PACK_WFWD, _lib.PACK_WDGRAD), _lib.CONV_3X3W6: (_lib.PACK_W6FWD, _lib.PACK_W6DGRAD),
    _lib.CONV_S2S6: (_lib.PACK_S6FWD, _lib.PACK_S6SWAP), _lib.CONV_T2S6: (_lib.PACK_T6FWD, _lib.PACK_T6SWAP),
    _lib.CONV_1X1S6: (_lib.PACK_P6FWD, _lib.PACK_P6DGRAD),
}


def conv_route(op, B, K, M, H, W, dgrad=False):
    """(weight pack kind, convolution kind code) of the launch that computes `op` from K to M channels, or with dgrad its data gradient
    (back from M to K channels); H, W = low-resolution size.  The first alternative whose switches are on and whose predicate holds."""
    if dgrad:
        op, K, M = _ADJOINT[op], M, K
    ck, preferred = _ROUTES[op]
    switch = globals().__getitem__
    for names, covers, kind in preferred:
        if all(map(switch, names)) and covers(B, K, M, H, W):
            ck = kind
            break
    return _PACK[ck][bool(dgrad)], ck


def fwd_kinds(kind, B, w, H, W):
    """(weight pack kind, convolution kind code) of the forward launch; H, W = low-resolution size"""
    return conv_route(kind, B, w.shape[1], w.shape[0], H, W)


def bwd_kinds(kind, B, w, H, W):
    """the same for the data gradient (a convolution from Co to Ci channels)"""
    return conv_route(kind, B, w.shape[1], w.shape[0], H, W, dgrad=True)


def plain_1x1_kinds(B, w, H, W, dgrad=False):
    """the same for a plain 1x1 product, forward (Ci -> Co) or data gradient (Co -> Ci)"""
    return conv_route('plain1x1', B, w.shape[1], w.shape[0], H, W, dgrad)


def packed_route(op, B, w, H, W, wscale, both):
    """Plan the forward of `op` with weights w and pack for it -> (packed layout, convolution kind, None).  both: a data gradient
    will be asked for - plan it now as well and pack the two layouts in one launch; the third value is then (its packed layout, its
    convolution kind), which _dgrad_raw(wp=...) launches later whatever the switches say by then."""
    K, M = w.shape[1], w.shape[0]
    pk, ck = conv_route(op, B, K, M, H, W)
    if not both:
        return packed(w, pk, wscale), ck, None
    pkb, ckb = conv_route(op, B, K, M, H, W, dgrad=True)
    wp, wpb = packed2(w, pk, pkb, wscale)
    return wp, ck, (wpb, ckb)


def _fwd_raw(x, w, kind, isc=None, osc=None, bias=None, act=0, wscale=1.0, with_bwd_pack=False):
    """with_bwd_pack: also return (the data-gradient packing of w, the convolution kind it is packed for) for _dgrad_raw(wp=...)."""
    H, W = _lowres_hw(kind, False, x)
    # (a no-grad forward inside a training loop: the same weights meet a backward later in the iteration, so pack for it ahead)
    ahead = _CACHES.pack_cache is not None and torch.is_grad_enabled() is False
    wp, ck, bwd = packed_route(kind, x.shape[0], w, H, W, wscale, with_bwd_pack or ahead)
    y = _lib.conv(x, wp, ck, w.shape[0], H, W, isc, osc, bias, act)
    return (y, bwd) if with_bwd_pack else y


def _dgrad_raw(g, w, kind, isc=None, osc=None, wscale=1.0, wp=None):
    """data gradient: g is shaped like the conv OUTPUT; returns a tensor shaped like the conv input.
    isc scales the channels of g ([B,Co]), osc the channels of the result ([B,Ci]).  wp: (w already packed for it, convolution kind)
    as _fwd_raw(with_bwd_pack=True) returned them; None plans both now."""
    H, W = _lowres_hw(kind, True, g)
    if wp is None:
        pk, ck = bwd_kinds(kind, g.shape[0], w, H, W)      # ('up': the strided kind is its adjoint; 'down': the transposed one)
        wp = packed(w, pk, wscale)
    else:
        wp, ck = wp
    return _lib.conv(g, wp, ck, w.shape[1], H, W, isc, osc)


def _wgrad_raw(g, x, kind, group=False):
    """per-sample correlation slabs [B, S, Co, Ci, taps] ('down': [B, S, Ci, Co, taps], see _slab_sum).  group=True: the caller
    only sums them (plain gradient), so several samples may share a slab (_lib.wgrad_slabs)."""
    if kind == 'down':     # same correlation as 'up' with the roles of the two tensors swapped
        H, W = g.shape[2], g.shape[3]
        return _lib.wgrad_slabs(x, g, _lib.CONV_T2, H, W, group)
    H, W = x.shape[2], x.shape[3]
    return _lib.wgrad_slabs(g, x, _ROUTES[kind][0], H, W, group)


def _slab_sum(slabs, kind):
    """plain (unmodulated) weight gradient [Co, Ci, taps] from the slabs"""
    gw = slabs.sum(dim=(0, 1))
    return gw.transpose(0, 1) if kind == 'down' else gw


def _wgrad_plain(gy, x, kind, ksize, wscale):
    """wscale * sum of the correlation slabs -> [Co, Ci, k, k] (te_wgrad_reduce_f32 without modulation; 'down' slabs come
    transposed and go through the framework's reduction)"""
    slabs = _wgrad_raw(gy, x, kind, group=True)
    Co, Ci = gy.shape[1], x.shape[1]
    if kind == 'down':
        gw = _slab_sum(slabs, kind)
        gw = gw * wscale if wscale != 1.0 else gw
    else:
        # (the reducer reads a weight operand only for the style / demodulation gradients, which are not asked for here)
        gw, _, _ = _lib.wgrad_reduce(slabs, slabs[0, 0], wscale, None, None, want_w=True)
    return gw.reshape(Co, Ci, ksize, ksize)


def set_split_bf16(on):
    """ONE switch for every split-bf16 kernel: the convolution kinds (gated here, by USE_SPLIT_BF16) and the weight-gradient kernels
    (gated in the library, te_wgrad_split_bf16).  Assigning `modconv.USE_SPLIT_BF16 = x` does the same (module property below), so an
    A/B that flips the Python flag can no longer leave the weight gradient on the other arithmetic."""
    on = bool(on)
    globals()['USE_SPLIT_BF16'] = on
    _lib.wgrad_split(int(on))
    return on


# The convolution y = d (.) conv(s (.) x, wscale w) as ONE family closed under differentiation (_Fwd / _Dgrad / _Wgrad below), with
# the style scale s[b,ci] and the demodulation d[b,co] each optional: without them it is the plain convolution (conv_core), with
# them the modulated one (modconv_closed).  It is one five-linear form
#     P(gy, x, w, s, d) = sum gy[b,co,p (+) t] x[b,ci,p] w[co,ci,t] s[b,ci] d[b,co]
# seen from its five arguments: y = dP/dgy, the data gradient dP/dx, the weight gradient dP/dw, and the two scale gradients
#     dP/ds[b,ci] = sum_p x * (dP/dx) / s ,      dP/dd[b,co] = sum_p gy * (dP/dgy) / d
# (the sums are te_chan_dot_f32 passes, the divisions [B,C]-sized).  The derivative of dP/da with respect to b, contracted with
# a cotangent c, is dP/db with a := c - so the three Functions name each other in their backwards, with the same constant wscale,
# and anything built on them differentiates to any order.  Unlike the chan_scale -> conv_core -> chan_scale composite of rounds
# 2-3, the scales ride INSIDE the convolution kernels (staging / epilogue, the arguments the fused first-order path has
# always used): per layer and order, three activation-sized elementwise passes and their autograd accumulations disappear
# (path-length step: 161 chan_scale launches and ~5 ms per step).
# What depends on a scale being there, each scale on its own: its gradient (and the tensor saved for it); the ToRGB streaming
# kernels, which want a style scale; and the weight gradient's slabs - per sample and through the reducer once a scale weighs the
# samples, the group plan of _wgrad_plain otherwise.  no_weight_grads() is honoured by the forward member's backward only.
_SCALE_FLOOR = 1e-20


def _nonzero(s):
    """The scale gradients of the closed family divide by the scale (dP/ds = sum_p x * (s U) / s with s U = the data gradient the
    kernel returns).  Scales of magnitude below 1e-20 - exact zeros included - are moved to +-1e-20 BEFORE they enter the family
    (kernels and divisions see the same value): the product s U then stays a normal number for every |U| > 1e-18, so the quotient is
    sum_p x U to fp32 accuracy instead of 0 / garbage (the former guard, 1.2e-38, let s U flush to zero), and the outputs move by less
    than 1e-20 |x w| - far below half an ulp of anything they are added to.  Both scales are guarded (the demodulation coefficient
    is rsqrt(... + 1e-8) > 0 in the model, but modconv_closed takes any osc).  What the division form cannot remove: under
    create_graph, d(dP/ds)/ds is two terms of size |dP/ds| / |s| that cancel analytically; their round-off, up to ~1e-6 |dP/ds| / |s|
    (each term carries the round-off of a pixel reduction: 8e-7 measured at a floored scale; at |s| = 1e-3 the error stays below
    1e-4 of the gradient on every op route), is what a channel with a small style
    scale adds to a second-order gradient (pinned second-order parity: tests/test_gpu_timed_second_order.py).
    The move is invisible to autograd (identity derivative, _Floor), so FIRST derivatives at a floored scale - an exact zero
    included - are the ones at the scale itself.  Second derivatives with respect to a floored scale carry no meaning: the round-off
    above is then ~1e-6 |dP/ds| / 1e-20, finite but arbitrary (every other first and second derivative is unaffected; checked in
    tests/test_gpu_conv_routes.py).  Only the chan_scale composite (USE_CLOSED_MODCONV off) differentiates twice through a zero scale."""
    if s is None:
        return None
    return _Floor.apply(s)


class _Floor(Function):
    """_nonzero's move of tiny scales, with the identity as its derivative (a torch.where would send no gradient to them)"""
    @staticmethod
    def forward(ctx, s):
        return torch.where(s.abs() < _SCALE_FLOOR, torch.where(s < 0, -_SCALE_FLOOR, _SCALE_FLOOR).to(s.dtype), s)

    @staticmethod
    def backward(ctx, g):
        return g


def _rgb_ok(kind, Co, Ci, x_like, osc, act=False):
    """ToRGB - a modulated 1x1 to 3 channels (te_rgb_supported asks for them) without demodulation or activation - is HBM-bound: the
    dedicated streaming kernels (csrc/rgb.hip) run it"""
    return kind == '1x1' and osc is None and not act and _lib.rgb_supported(Co, Ci, x_like.shape[2] * x_like.shape[3])


def _chan_dot(a, b):
    return _ChanDot.apply(a.contiguous(), b.contiguous())


def _dense(scale):
    return None if scale is None else scale.contiguous()


class _Fwd(Function):
    @staticmethod
    def forward(ctx, x, w, s, d, kind, wscale):        # d (.) conv(s (.) x, wscale w)
        ctx.kind, ctx.wscale = kind, wscale
        ctx.graph = current_graph()
        keep_cache(ctx)
        if s is not None and _rgb_ok(kind, w.shape[0], w.shape[1], x, d):
            y = _lib.rgb_fwd(x, w.reshape(3, w.shape[1]), s.contiguous(), None, wscale)
        else:
            y = _fwd_raw(x, w, kind, _dense(s), _dense(d), None, 0, wscale)
        ctx.save_for_backward(x, w, s, d, None if d is None else y)      # (y: for dP/dd only)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, s, d, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        skip_w = weights_skipped(ctx.graph)
        with cache_of(ctx):
            gx = _Dgrad.apply(gy, w, s, d, ctx.kind, ctx.wscale) if (need[0] or need[2]) else None
            gw = _Wgrad.apply(gy, x, s, d, ctx.kind, w.shape[2], ctx.wscale) if (need[1] and not skip_w) else None
        gs = _chan_dot(gx, x) / s if need[2] else None
        gd = _chan_dot(gy, y) / d if need[3] else None
        return (gx if need[0] else None), gw, gs, gd, None, None


class _Dgrad(Function):
    @staticmethod
    def forward(ctx, gy, w, s, d, kind, wscale):       # s (.) dgrad(d (.) gy, wscale w), shaped like the convolution's input
        ctx.kind, ctx.wscale = kind, wscale
        keep_cache(ctx)
        if s is not None and _rgb_ok(kind, w.shape[0], w.shape[1], gy, d):
            gx = _lib.rgb_dgrad(gy, w.reshape(3, w.shape[1]), s.contiguous(), w.shape[1], wscale)
        else:
            gx = _dgrad_raw(gy, w, kind, isc=_dense(d), osc=_dense(s), wscale=wscale)
        ctx.save_for_backward(gy, w, s, d, None if s is None else gx)    # (gx: for dP/ds only)
        return gx

    @staticmethod
    def backward(ctx, ggx):
        gy, w, s, d, gx = ctx.saved_tensors
        need = ctx.needs_input_grad
        with cache_of(ctx):
            y2 = _Fwd.apply(ggx, w, s, d, ctx.kind, ctx.wscale) if (need[0] or need[3]) else None
            gw = _Wgrad.apply(gy, ggx, s, d, ctx.kind, w.shape[2], ctx.wscale) if need[1] else None
        gs = _chan_dot(ggx, gx) / s if need[2] else None
        gd = _chan_dot(gy, y2) / d if need[3] else None
        return (y2 if need[0] else None), gw, gs, gd, None, None


class _Wgrad(Function):
    @staticmethod
    def forward(ctx, gy, x, s, d, kind, ksize, wscale):    # wscale * sum_b d_b s_b (correlation slab of sample b)  [Co,Ci,k,k]
        ctx.kind, ctx.wscale = kind, wscale
        keep_cache(ctx)
        ctx.save_for_backward(gy, x, s, d)
        if s is None and d is None:       # nothing per sample is derived from the slabs: samples may share one (the group plan)
            return _wgrad_plain(gy, x, kind, ksize, wscale)
        Co, Ci = gy.shape[1], x.shape[1]
        gyc, xc = gy.contiguous(), x.contiguous()
        if s is not None and _rgb_ok(kind, Co, Ci, x, d):
            slabs = _lib.rgb_wgrad_slabs(gyc, xc)
        else:
            slabs = _wgrad_raw(gyc, xc, kind)
        gw, _, _ = _lib.wgrad_reduce(slabs, slabs[0, 0], wscale, _dense(s), _dense(d), want_w=True)
        return gw.reshape(Co, Ci, ksize, ksize)

    @staticmethod
    def backward(ctx, ggw):
        gy, x, s, d = ctx.saved_tensors
        need = ctx.needs_input_grad
        with cache_of(ctx):
            y2 = _Fwd.apply(x, ggw, s, d, ctx.kind, ctx.wscale) if (need[0] or need[3]) else None
            gx = _Dgrad.apply(gy, ggw, s, d, ctx.kind, ctx.wscale) if (need[1] or need[2]) else None
        gs = _chan_dot(gx, x) / s if need[2] else None
        gd = _chan_dot(gy, y2) / d if need[3] else None
        return (y2 if need[0] else None), (gx if need[1] else None), gs, gd, None, None, None


def _closed_ok(x):
    return x.is_cuda and x.dtype == torch.float32


USE_CLOSED_MODCONV = True      # False: the chan_scale -> conv_core -> chan_scale composite of rounds 2-3 (A/B measurements)


def conv_core(x, w, kind='3x3', wscale=1.0):
    """Plain convolution y = conv(x, wscale * w) (w [Co,Ci,k,k]), differentiable to any order: the closed family without scales."""
    return _Fwd.apply(x, w, None, None, kind, float(wscale))


def modconv_closed(x, w, isc, osc, kind='3x3', wscale=1.0):
    """osc (.) conv(isc (.) x, wscale * w), differentiable to any order with the scales inside the convolution kernels"""
    return _Fwd.apply(x, w, _nonzero(isc), _nonzero(osc), kind, float(wscale))


def _composite(x, w, isc, osc, bias, act, kind, wscale=1.0):
    """The same function as the fused kernel, built from any-order differentiable pieces (the equalised-lr constant rides
    in the weight packing of the family: no `w * wscale` pass, no scaling pass for its gradient)."""
    if USE_CLOSED_MODCONV and isc is not None and kind in ('3x3', 'up', '1x1') and _closed_ok(x):
        y = modconv_closed(x, w, isc, osc, kind, wscale)
        if act:
            return fused_leaky_relu(y, bias, 0.2, _act_gain(act))
        return y if bias is None else y + bias[None, :, None, None]
    if isc is not None:
        x = chan_scale(x, isc)
    y = conv_core(x, w, kind, wscale)
    if osc is not None:
        y = chan_scale(y, osc)
    if act:
        return fused_leaky_relu(y, bias, 0.2, _act_gain(act))
    if bias is not None:
        y = y + bias[None, :, None, None]
    return y


def _modconv_bwd(g, x, w, isc, osc, kind, wscale, need, wp_bwd=None, rgb=False, wsq=None):
    """First-order backward of the modulated convolution y = osc (.) conv(isc (.) x, wscale w) from g = dL/dy (contiguous) ->
    (gx, gw, gisc, gosc): ONE data-gradient convolution (wp_bwd: its packed weights and kind as the forward planned them; rgb: the
    ToRGB streaming kernels), ONE correlation pass into per-sample slabs, the slab reducer.  need: flags for (x, w, isc, osc).
    wsq (te_demod_fwd_f32's squares): osc is the demodulation coefficient of (w, isc) computed inside the node, so its gradient is
    chained into gw / gisc in place and gosc comes back None.  Shared by _ModConvFused and op/styled_rgb.py::_ModConvRGB."""
    gx = gw = gisc = gosc = None
    if need[0] and rgb:
        gx = _lib.rgb_dgrad(g, w.reshape(w.shape[0], w.shape[1]), isc, x.shape[1], wscale)
    elif need[0]:
        gx = _dgrad_raw(g, w, kind, isc=osc, osc=isc, wscale=wscale, wp=wp_bwd)
    if need[1] or (need[2] and isc is not None) or (need[3] and osc is not None):
        slabs = _lib.rgb_wgrad_slabs(g, x) if rgb else _wgrad_raw(g, x, kind)
        if kind == 'down' and isc is None and osc is None:        # the discriminator's convolutions
            gw = _slab_sum(slabs, kind).reshape(w.shape) if need[1] else None
            if gw is not None and wscale != 1.0:
                gw = gw * wscale
            return gx, gw, None, None
        if kind == 'down':       # modulated (ModulatedConv2d(downsample=True)): slabs come as [B,S,Ci,Co,taps]
            slabs = slabs.sum(dim=1).transpose(1, 2).contiguous().unsqueeze(1)
        w3 = w.reshape(w.shape[0], w.shape[1], -1)
        dm = wsq is not None
        gw, gisc, gosc = _lib.wgrad_reduce(slabs, w3, wscale, isc, osc,
                                           want_w=need[1], want_isc=need[2] and isc is not None,
                                           want_osc=(need[3] or dm) and osc is not None)
        if dm:       # chain through d = demod(w, isc): its dW / d style are added to gw / gisc in place
            if gw is not None or gisc is not None:
                _lib.demod_bwd(gosc, osc, w3, wsq, isc, wscale, into=(gw, gisc))
            gosc = None
        if gw is not None:
            gw = gw.reshape(w.shape)
    return gx, gw, gisc, gosc


class _ModConvFused(Function):
    @staticmethod
    def forward(ctx, x, w, isc, osc, bias, act, kind, wscale, demod_eps):
        # demod_eps != None: osc is the demodulation coefficient of (w, isc), computed here (te_demod_fwd_f32) and
        # differentiated here (its dW / d style are accumulated into the convolution's own in the backward)
        ctx.act, ctx.kind, ctx.wscale = act, kind, wscale
        ctx.demod = ctx.wp_bwd = None
        keep_cache(ctx)
        if demod_eps is not None:
            w3 = w.reshape(w.shape[0], w.shape[1], -1)
            osc, wsq = _lib.demod_fwd(w3, isc, wscale, demod_eps)
            ctx.demod = (demod_eps, wsq)
        ctx.rgb = _rgb_ok(kind, w.shape[0], w.shape[1], x, osc, act)
        # from-RGB stem (1x1 FROM 3 channels, unmodulated: the discriminator's first layer, :815): write-bound, the same
        # streaming kernels with the operands' roles exchanged instead of a 3-of-16-channels MFMA stage
        ctx.stem = (not ctx.rgb and kind == '1x1' and w.shape[1] == 3 and isc is None and osc is None
                    and _lib.rgb_supported(3, w.shape[0], x.shape[2] * x.shape[3]))
        if ctx.rgb:
            out = _lib.rgb_fwd(x, w.reshape(w.shape[0], w.shape[1]), isc, bias, wscale)
        elif ctx.stem:
            out = _lib.rgb_expand(x, w.reshape(w.shape[0], 3).t(), bias, _act_code(act), wscale)
        elif ctx.needs_input_grad[0]:       # a backward will want dx: pack the data-gradient layout in the same launch (+ its kind)
            out, ctx.wp_bwd = _fwd_raw(x, w, kind, isc, osc, bias, _act_code(act), wscale, with_bwd_pack=True)
        else:
            out = _fwd_raw(x, w, kind, isc, osc, bias, _act_code(act), wscale)
        ctx.save_for_backward(x, w, isc, osc, bias, out if act else None)      # (ToRGB has no activation)
        return out

    @staticmethod
    def backward(ctx, g):
        with cache_of(ctx):
            return _ModConvFused._backward(ctx, g)

    @staticmethod
    def _backward(ctx, g):
        x, w, isc, osc, bias, out = ctx.saved_tensors
        act, kind, wscale = ctx.act, ctx.kind, ctx.wscale
        need = ctx.needs_input_grad
        if torch.is_grad_enabled():
            # double backward requested: differentiate the composite built from the closed family (op/recorded.py)
            dm = ctx.demod is not None           # osc is then a function of (w, isc) inside this node, rebuilt from their aliases

            def build(x, w, isc, osc, bias):
                return _composite(x, w, isc, demod(w, isc, wscale, ctx.demod[0]) if dm else osc, bias, act, kind, wscale)
            nd = (need[0], need[1] and not weights_skipped()) + need[2:5]      # (built outside second_order(): default token)
            return tuple(recorded_backward(build, (x, w, isc, None if dm else osc, bias), nd, g)) + (None,) * 4
        g = g.contiguous()
        g_bias = None
        if act:
            g, g_bias = _lib.bias_act_bwd(g, out, 0.2, _act_gain(act), want_bias=bias is not None)
        elif bias is not None and need[4]:
            g_bias = g.sum(dim=(0, 2, 3))
        if ctx.stem:
            gx = _lib.rgb_fwd(g, w.reshape(w.shape[0], 3).t().contiguous(), None, None, wscale) if need[0] else None
            gw = None
            if need[1]:
                gw = _lib.rgb_wgrad_slabs(x, g).sum(dim=(0, 1)).reshape(3, w.shape[0]).t().reshape(w.shape)
                gw = gw * wscale if wscale != 1.0 else gw
            return gx, gw, None, None, g_bias, None, None, None, None
        wsq = ctx.demod[1] if ctx.demod is not None else None
        gx, gw, gisc, gosc = _modconv_bwd(g, x, w, isc, osc, kind, wscale, need[:4], ctx.wp_bwd, ctx.rgb, wsq)
        return gx, gw, gisc, gosc, g_bias, None, None, None, None


def modconv(x, w, isc=None, osc=None, bias=None, act=False, kind='3x3', wscale=1.0, demod_eps=None):
    """out = [lrelu*sqrt2]( osc[b,co] * conv(isc[b,ci] * x, wscale * w) + bias[co] )  — fused kernels.
    `act`: False, True (gain sqrt(2), the reference's FusedLeakyReLU) or the gain itself (sqrt(2) or 1.0).
    `demod_eps` (instead of `osc`): osc = rsqrt(sum (wscale w isc)^2 + eps), the StyleGAN2 demodulation
    (model_spatial_query.py:300-304), evaluated and differentiated inside the same autograd node.
    `wscale` is the equalised-lr constant: the parameter is consumed as stored, its gradient comes back scaled."""
    if demod_eps is not None and (osc is not None or isc is None or isc.shape[0] > 64 or w.shape[1] > 8192):
        if osc is not None or isc is None:
            raise RuntimeError('modconv: demod_eps needs isc and excludes an explicit osc')
        osc, demod_eps = demod(w, isc, float(wscale), demod_eps), None      # shapes the demod kernels do not cover
    if _STATE.second_order and torch.is_grad_enabled():
        if demod_eps is not None:
            osc = demod(w, isc, float(wscale), demod_eps)
        return _composite(x, w, isc, osc, bias, act, kind, float(wscale))
    isc = isc.contiguous() if isc is not None else None
    osc = osc.contiguous() if osc is not None else None
    if _CACHES.frozen_on and not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w, isc, osc, bias))):
        return _modconv_frozen(x, w, isc, osc, bias, act, kind, float(wscale), demod_eps)
    return _ModConvFused.apply(x, w, isc, osc, bias, act, kind, float(wscale), demod_eps)


# `modconv.USE_SPLIT_BF16 = flag` goes through set_split_bf16 (reads stay plain global lookups)
import sys as _sys
import types as _types


class _ModconvModule(_types.ModuleType):
    @property
    def USE_SPLIT_BF16(self):
        return self.__dict__['USE_SPLIT_BF16']

    @USE_SPLIT_BF16.setter
    def USE_SPLIT_BF16(self, on):
        set_split_bf16(on)


_sys.modules[__name__].__class__ = _ModconvModule

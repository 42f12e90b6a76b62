"""ctypes binding of libte_hip.so (C ABI: include/te_hip.h) + thin tensor-level wrappers.

The product path has NO fallback: if the shared object is missing, was built for another
architecture, or a tensor is not a contiguous fp32 CUDA(HIP) tensor, these wrappers raise.
PyTorch is used here only for device memory and the current HIP stream.

Every entry point is declared once, in include/te_hip.h: lib() reads the ctypes prototypes from the header (_abi.parse), so
there is no table to keep in step.  A new entry point needs its prototype in the header and one wrapper here that hands its
arguments to _launch('te_name', ...), decorated with @_op (which gives it its roctx range under TE_ROCTX=1).
"""
import ctypes as C
import os

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libte_hip.so')
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'te_hip.h')
_lib = _protos = None

CONV_3X3, CONV_T2, CONV_S2, CONV_1X1, CONV_3X3W, CONV_3X3W6, CONV_S2S6, CONV_T2S6, CONV_1X1S6 = 0, 1, 2, 3, 4, 5, 6, 7, 8
(PACK_FWD, PACK_DGRAD, PACK_SWAP, PACK_WFWD, PACK_WDGRAD, PACK_W6FWD, PACK_W6DGRAD, PACK_S6FWD, PACK_S6SWAP, PACK_T6FWD,
 PACK_T6SWAP, PACK_P6FWD, PACK_P6DGRAD) = range(13)


def _header_text():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f'{HEADER_PATH} is missing: the bindings of libte_hip.so are read from it')
    with open(HEADER_PATH) as f:
        return f.read()


def _prototypes():
    """(once) ({name: (restype, argtypes)} in header order, TE_ABI_VERSION) of include/te_hip.h"""
    global _protos
    if _protos is None:
        text = _header_text()
        _protos = _abi.parse(text), _abi.abi_version(text)
    return _protos


def __getattr__(name):
    if name == 'EXPORTS':           # the entry points' names in header order (read at first use)
        return tuple(_prototypes()[0])
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def lib():
    """Load (once) and return the CDLL.  Raises RuntimeError if the extension is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'{LIB_PATH} is missing: build it with `python -m transeditor_amd.build` '
                               '(there is no CPU / PyTorch fallback for the TransEditor hot path)')
        protos, version = _prototypes()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in protos.items():
            if not hasattr(L, name):
                raise RuntimeError(f'{LIB_PATH} does not export {name}')
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        if L.te_arch() != b'gfx950':
            raise RuntimeError('libte_hip.so was not built for gfx950')
        if L.te_version() != version:
            raise RuntimeError(f'{LIB_PATH} has ABI version {L.te_version()} but include/te_hip.h declares {version}: '
                               'a stale library, rebuild it with `python -m transeditor_amd.build`')
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f'{what} failed (code {rc}): {lib().te_last_error_string().decode()}')


def _launch(name, *args):
    """enqueue entry point `name` with `args` on the current stream; a failure raises in that same name"""
    rc = getattr(_lib or lib(), name)(*args, _stream())
    if rc:                          # (the one extra Python call per launch is paid for by skipping lib() and _check on success)
        _check(rc, name)


_OPS = []


def _op(fn):
    """marks a tensor-level wrapper that launches: TE_ROCTX=1 runs each of them inside a roctx range (end of this module)"""
    _OPS.append(fn)
    return fn


_cur_dev = getattr(torch._C, '_cuda_getDevice', torch.cuda.current_device)


def _on_current_device(t):
    """The kernels are enqueued on the CURRENT device's current stream (what the reference's ops do,
    fused_bias_act_kernel.cu:90, upfirdn2d_kernel.cu:192).  Unlike the reference, a tensor that lives on another GPU is
    refused instead of being read through a foreign pointer on the wrong stream."""
    if t.device.index != _cur_dev():          # (a CUDA tensor exists, so the runtime is initialised)
        raise RuntimeError(f'te_hip: tensor on {t.device} but the current device is cuda:{torch.cuda.current_device()}; '
                           f'call torch.cuda.set_device (one process per GPU) or wrap the call in torch.cuda.device(...)')


def _ptr(t, dtype=torch.float32, dense=True):
    """device pointer of t (None: NULL) after the one check every operand gets: on the current GPU, of `dtype`, and contiguous
    unless the entry point addresses it through explicit strides (dense=False)"""
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == dtype and (t.is_contiguous() or not dense)):
        name = 'fp32' if dtype == torch.float32 else dtype
        raise RuntimeError(f'te_hip: expected {"a contiguous" if dense else "an"} {name} tensor on the GPU, got {t.dtype} {t.device} '
                           + (f'contiguous={t.is_contiguous()} ' if dense else '') + '(no CPU path exists)')
    _on_current_device(t)
    return t.data_ptr()


_ptr_as = _ptr                  # (t, dtype): an operand that is not fp32


def _raw(t):
    """device pointer of a tensor addressed through explicit strides (no contiguity requirement)"""
    return _ptr(t, dense=False)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _aligned16(t):
    """t, or a fresh (16-byte aligned) copy of it when its data is not: a contiguous view at an offset into its storage keeps
    that offset through .contiguous()"""
    if t is None or t.data_ptr() % 16 == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


# --------------------------------------------------------------------------------------------- K1
_OTHER = {torch.float16: 'f16', torch.float64: 'f64'}       # K1 / K2 also exist in the reference's other two dispatch types


def _dispatch(x):
    """(entry-point suffix, operand dtype) of K1 / K2 for x; anything but half and double goes to the fp32 entry, whose operand
    check refuses what is not fp32"""
    return (_OTHER[x.dtype], x.dtype) if x.dtype in _OTHER else ('f32', torch.float32)


def _inner(shape):
    """prod(shape[2:]): the elements per channel of [B,C,...]"""
    n = 1
    for d in shape[2:]:
        n *= d
    return n


@_op
def bias_act(x, b, ref, act, grad, alpha, scale):
    """out = act(x + b[channel]) * scale; channel = dim 1 (step_b = prod(shape[2:]))."""
    x = x.contiguous()
    sfx, dt = _dispatch(x)
    out = torch.empty_like(x)
    _launch('te_bias_act_' + sfx, _ptr(out, dt), _ptr(x, dt), _ptr(b, dt), _ptr(ref, dt), act, grad, alpha, scale, x.numel(),
            _inner(x.shape), b.numel() if b is not None else 1)
    return out


def _bias_grad_buffers(want_bias, outer, Cn, inner, device):
    """(gb, workspace): the bias gradient is WRITTEN by a fixed-order second pass over per-block partials (no atomics, so no
    zero fill and bit-reproducible); it owns its storage (it becomes a parameter's .grad)."""
    if not want_bias:
        return None, None
    n = lib().te_bias_act_bwd_ws_floats(outer, Cn, inner)
    return (torch.empty(Cn, device=device, dtype=torch.float32),
            torch.empty(n, device=device, dtype=torch.float32) if n > 0 else None)


@_op
def bias_act_bwd(g, ref, alpha, scale, want_bias=True):
    g = g.contiguous()
    if g.dtype in _OTHER:       # the reference's two steps (fused_act.py:18-38): the kernel in grad mode, then the bias sum
        gi = bias_act(g, None, ref, 3, 1, alpha, scale)
        return gi, (gi.sum(dim=[0] + list(range(2, gi.ndim))) if want_bias else None)
    gi = torch.empty_like(g)
    Cn, inner = g.shape[1], _inner(g.shape)
    gb, ws = _bias_grad_buffers(want_bias, g.shape[0], Cn, inner, g.device)
    _launch('te_bias_act_bwd_f32', _ptr(gi), _ptr(gb), _ptr(ws), _ptr(g), _ptr(ref), alpha, scale, g.shape[0], Cn, inner)
    return gi, gb


def bias_act_bwd_rgb_supported(shape):
    return bool(lib().te_bias_act_bwd_rgb_supported(shape[0], shape[1], _inner(shape)))


@_op
def bias_act_bwd_rgb(g, ref, grgb, wrgb, srgb, wscale, alpha, scale, want_bias=True):
    """activation gradient with a ToRGB data gradient folded in (see te_hip.h); g may be None.  -> (gi, gb | None)
    The kernel reads g, ref and grgb with 16-byte accesses and the ABI refuses misaligned ones: an operand whose data is not
    16-byte aligned (an upstream gradient that is a view at an offset into its storage) is handed over as an aligned copy."""
    ref, grgb = _aligned16(ref.contiguous()), _aligned16(grgb.contiguous())
    g = _aligned16(g.contiguous()) if g is not None else None
    gi = torch.empty_like(ref)
    Cn, inner = ref.shape[1], _inner(ref.shape)
    gb, ws = _bias_grad_buffers(want_bias, ref.shape[0], Cn, inner, ref.device)
    _launch('te_bias_act_bwd_rgb_f32', _ptr(gi), _ptr(gb), _ptr(ws), _ptr(g), _ptr(ref), _ptr(grgb), _ptr(wrgb.contiguous()),
            _ptr(srgb.contiguous()) if srgb is not None else None, wscale, alpha, scale, ref.shape[0], Cn, inner)
    return gi, gb


# --------------------------------------------------------------------------------------------- K2
@_op
def upfirdn2d_raw(x, k, up, down, pad, bias=None, act=0, alpha=0.2, scale=1.0):
    """x [B,C,H,W] -> [B,C,H',W'];  pad = (px0, px1, py0, py1);  up/down = (x, y)."""
    x = x.contiguous()
    B, Cn, H, W = x.shape
    kh, kw = k.shape
    px0, px1, py0, py1 = pad
    oh = (H * up[1] + py0 + py1 - kh) // down[1] + 1
    ow = (W * up[0] + px0 + px1 - kw) // down[0] + 1
    if oh <= 0 or ow <= 0:
        raise RuntimeError(f'upfirdn2d: empty output {oh}x{ow}')
    out = torch.empty(B, Cn, oh, ow, device=x.device, dtype=x.dtype)
    sfx, dt = _dispatch(x)
    if sfx != 'f32':
        if bias is not None or act:
            raise RuntimeError('upfirdn2d: the fused bias / activation epilogue exists in fp32 only')
        k = k.to(dt)                # (the taps in the tensors' own type; the fp32 entry takes fp32 taps only)
    args = [_ptr(out, dt), _ptr(x, dt), _ptr(k.contiguous(), dt), B * Cn, H, W, 1, kh, kw, up[0], up[1], down[0], down[1],
            px0, px1, py0, py1]
    if sfx == 'f32':
        args += [_ptr(bias), bias.numel() if bias is not None else 1, act, alpha, scale]
    _launch('te_upfirdn2d_' + sfx, *args)
    return out


@_op
def blur_actgrad(g, ref, k_flipped, pad, alpha, scale):
    """backward of blur + bias + lrelu in one pass: returns (gx, gbias).  g / ref [B,C,H,W]; pad = (px0, px1, py0, py1)."""
    g, ref = g.contiguous(), ref.contiguous()
    B, Cn, H, W = g.shape
    kh, kw = k_flipped.shape
    px0, px1, py0, py1 = pad
    tiles = lib().te_blur_actgrad_tiles(H, W, kh, kw, px0, px1, py0, py1)
    if tiles <= 0:
        raise RuntimeError(f'te_blur_actgrad_tiles failed ({tiles})')
    gx = torch.empty(B, Cn, H + py0 + py1 - kh + 1, W + px0 + px1 - kw + 1, device=g.device, dtype=g.dtype)
    partial = torch.empty(B, Cn, tiles, device=g.device, dtype=g.dtype)
    _launch('te_blur_actgrad_f32', _ptr(gx), _ptr(partial), _ptr(g), _ptr(ref), _ptr(k_flipped.contiguous()), B * Cn, H, W, kh, kw, px0,
            px1, py0, py1, alpha, scale)
    return gx, partial.sum(dim=(0, 2))


@_op
def blur_gradact(g, ref, k_flipped, pad, alpha, scale):
    """backward of 'bias + lrelu -> blur' in one pass: (upfirdn2d(g, k_flipped, pad) * slope(ref), gbias).  ref is shaped
    like the result."""
    g, ref = g.contiguous(), ref.contiguous()
    B, Cn, H, W = g.shape
    kh, kw = k_flipped.shape
    px0, px1, py0, py1 = pad
    oh, ow = H + py0 + py1 - kh + 1, W + px0 + px1 - kw + 1
    if tuple(ref.shape) != (B, Cn, oh, ow):
        raise RuntimeError(f'blur_gradact: ref {tuple(ref.shape)} is not the shape of the adjoint blur output {(B, Cn, oh, ow)}')
    tiles = lib().te_blur_actgrad_tiles(H, W, kh, kw, px0, px1, py0, py1)
    if tiles <= 0:
        raise RuntimeError(f'te_blur_actgrad_tiles failed ({tiles})')
    gx = torch.empty(B, Cn, oh, ow, device=g.device, dtype=g.dtype)
    partial = torch.empty(B, Cn, tiles, device=g.device, dtype=g.dtype)
    _launch('te_blur_gradact_f32', _ptr(gx), _ptr(partial), _ptr(g), _ptr(ref), _ptr(k_flipped.contiguous()), B * Cn, H, W, kh, kw, px0,
            px1, py0, py1, alpha, scale)
    return gx, partial.sum(dim=(0, 2))


FIR_KERNELS = ('direct', 'blur44', 'tile_up2', 'tile_down2', 'tile_ag')                     # TE_FIR_* (te_hip.h)
FIR_FORM = ('kernel', 'mode', 'D', 'ext', 'ext_x', 'ext_y', 'tile_h', 'tile_w', 'tiles_x', 'tiles_y', 'zgroups', 'grid_x', 'threads')   # te_fir_form
FIR_OPS = {'upfirdn2d': 0, 'blur_actgrad': 1, 'blur_gradact': 2}


def fir_form(op, major, in_h, in_w, pad, kh=4, kw=4, up=(1, 1), down=(1, 1), minor=1):
    """the plan of the te_upfirdn2d_f32 / te_blur_actgrad_f32 / te_blur_gradact_f32 launch (op: a key of FIR_OPS) over `major` planes
    of in_h x in_w with pad = (px0, px1, py0, py1) and up / down = (x, y) (host only): a dict of FIR_FORM with 'kernel' as a name of
    FIR_KERNELS; the negative TE_ERR_* code where the launch refuses"""
    buf = (C.c_int * len(FIR_FORM))()
    rc = lib().te_fir_form(FIR_OPS[op], major, in_h, in_w, minor, kh, kw, up[0], up[1], down[0], down[1], *pad, buf)
    if rc:
        return rc
    f = dict(zip(FIR_FORM, buf))
    f['kernel'] = FIR_KERNELS[f['kernel']]
    return f


# --------------------------------------------------------------------------------------------- F1
@_op
def conv_pack(w, kind_pack, wscale=1.0):
    """w [Co,Ci,k,k] (model layout) -> packed Wp[tap][Kp][Mp]."""
    w = w.contiguous()
    Co, Ci, ks, _ = w.shape
    n = lib().te_conv_packed_numel(kind_pack, Co, Ci, ks)
    wp = torch.empty(n, device=w.device, dtype=w.dtype)
    _launch('te_conv_pack_weights_f32', _ptr(wp), _ptr(w), wscale, kind_pack, Co, Ci, ks)
    return wp


@_op
def conv_pack2(w, kind_a, kind_b, wscale=1.0):
    """both packed layouts of w in one launch -> (wp_a, wp_b)"""
    w = w.contiguous()
    Co, Ci, ks, _ = w.shape
    wa = torch.empty(lib().te_conv_packed_numel(kind_a, Co, Ci, ks), device=w.device, dtype=w.dtype)
    wb = torch.empty(lib().te_conv_packed_numel(kind_b, Co, Ci, ks), device=w.device, dtype=w.dtype)
    _launch('te_conv_pack_weights2_f32', _ptr(wa), kind_a, _ptr(wb), kind_b, _ptr(w), wscale, Co, Ci, ks)
    return wa, wb


@_op
def conv_pack_multi(jobs):
    """jobs: [(wp, w, kind_pack, wscale)] with w [Co,Ci,k,k] dense and wp an already allocated packed buffer of the right
    size: every layout is (re)written in one launch per 64 jobs."""
    n = len(jobs)
    if not n:
        return
    for wp, w, _, _ in jobs:
        if not (w.is_contiguous() and wp.is_contiguous()):
            raise RuntimeError('te_hip: conv_pack_multi needs dense weights and buffers')
    arr = lambda ty, vals: (ty * n)(*vals)
    _launch('te_conv_pack_weights_multi_f32', n, arr(C.c_void_p, [_ptr(j[0]) for j in jobs]), arr(C.c_void_p, [_ptr(j[1]) for j in jobs]),
            arr(C.c_float, [float(j[3]) for j in jobs]), arr(C.c_int, [int(j[2]) for j in jobs]),
            arr(C.c_int, [j[1].shape[0] for j in jobs]), arr(C.c_int, [j[1].shape[1] for j in jobs]),
            arr(C.c_int, [j[1].shape[2] for j in jobs]))


def wino_ok(B, K, M, H, W):
    """does TE_CONV_3X3W (1-D Winograd F(2,3): 2/3 of the MFMAs of the direct 3x3 kernel) cover this problem?"""
    return bool(lib().te_conv_wino_supported(B, K, M, H, W))


def s2s6_ok(B, K, M, H, W):
    """does TE_CONV_S2S6 (the stride-2 convolution on the bf16 matrix pipe, three-piece split) cover this problem?  H, W = output size"""
    return bool(lib().te_conv_s2s6_supported(B, K, M, H, W))


def t2s6_ok(B, K, M, H, W):
    """does TE_CONV_T2S6 (the transposed stride-2 convolution on the bf16 matrix pipe) cover this problem?  H, W = input (low-res) size"""
    return bool(lib().te_conv_t2s6_supported(B, K, M, H, W))


def p1s6_ok(B, K, M, H, W):
    """does TE_CONV_1X1S6 (the 1x1 convolution on the bf16 matrix pipe) cover this problem?"""
    return bool(lib().te_conv_p1s6_supported(B, K, M, H, W))


def wino6_form(form=-1):
    """test and tool hook: kernel form of TE_CONV_3X3W6 - 2 = two-image (default; M % 128 == 0 and a block per CU, else ping-pong),
    3 = two-image wherever M % 128 == 0, 1 = ping-pong (bit-identical results); returns the previous value (any other value: query only)"""
    return int(lib().te_conv_wino6_form(form))


def wino6_tiles_per_block(n=-1):
    """test and tool hook: tiles a block of the two-image form of TE_CONV_3X3W6 walks - 0 = automatic (default), 1 = one tile per block,
    n >= 2 = runs of at most n tiles (bit-identical results); returns the previous value (anything but 0 .. 4096: query only)"""
    return int(lib().te_conv_wino6_tiles_per_block(n))


def s2s6_form(form=-1):
    """test and tool hook: kernel form of TE_CONV_S2S6 - 1 = two-image (default; M % 128 == 0 and a block per CU, else ping-pong),
    2 = two-image wherever M % 128 == 0, 0 = ping-pong (bit-identical results); returns the previous value (-1: query only)"""
    return int(lib().te_conv_s2s6_form(form))


def t2s6_form(form=-1):
    """test and tool hook: kernel form of TE_CONV_T2S6, as s2s6_form"""
    return int(lib().te_conv_t2s6_form(form))


def wino6_ok(B, K, M, H, W):
    """does TE_CONV_3X3W6 (the Winograd form on the bf16 matrix pipe, three-piece split, fp32-equivalent) cover this problem?"""
    return bool(lib().te_conv_wino6_supported(B, K, M, H, W))


def conv_out_shape(kind, B, M, H, W):
    if kind in (CONV_T2, CONV_T2S6):
        return (B, M, 2 * H + 1, 2 * W + 1)
    return (B, M, H, W)


CONV_FORM_HEAD = ('tc', 'fast', 'ms', 'multi_sample', 'occ', 'ksplit', 'nreg', 'ntiles', 'nbody', 'mblocks', 'grid_x')      # te_conv_form (te_hip.h)
CONV_FORM_REGION = ('TW', 'TH', 'NS', 'NSv', 'tiles_x', 'tiles_y', 'tapmask', 'TH0')
CONV_EPI = {'none': 0, 'res': 1, 'mask': 2, 'both': 3}


def conv_form(kind, B, K, M, H, W, has_isc=False, epi='none', with_ws=True):
    """the form of the fp32 direct kernel that conv() launches for this problem (host only): a dict of CONV_FORM_HEAD plus 'regions', a list of
    nreg dicts of CONV_FORM_REGION; the negative TE_ERR_* code where the launch refuses the combination"""
    buf = (C.c_int * (len(CONV_FORM_HEAD) + 3 * len(CONV_FORM_REGION)))()
    rc = lib().te_conv_form(kind, B, K, M, H, W, int(has_isc), CONV_EPI[epi], int(with_ws), buf)
    if rc:
        return rc
    v, h, r = list(buf), len(CONV_FORM_HEAD), len(CONV_FORM_REGION)
    form = dict(zip(CONV_FORM_HEAD, v[:h]))
    form['regions'] = [dict(zip(CONV_FORM_REGION, v[h + i * r:h + (i + 1) * r])) for i in range(form['nreg'])]
    return form


CONV_SPLIT_FORM = ('two_image', 'pair16', 'mblocks', 'ntiles', 'blocks', 'idle', 'tpb', 'lists', 'lds', 'edge_ct', 'edge_line_tiles', 'edge_blocks',
                   'scratch', 'isc')      # te_conv_split_form (te_hip.h)


def conv_split_form(kind, B, K, M, H, W, has_isc=False, with_scratch=True):
    """the plan of the conv() launch of a split-bf16 kind (CONV_3X3W6, CONV_S2S6, CONV_T2S6, CONV_1X1S6) under the current form hooks
    (host only): a dict of CONV_SPLIT_FORM; the negative TE_ERR_* code where the launch refuses.  conv() always hands CONV_T2S6 its
    column scratch: with_scratch=True is what it launches."""
    buf = (C.c_int * len(CONV_SPLIT_FORM))()
    rc = lib().te_conv_split_form(kind, B, K, M, H, W, int(has_isc), int(with_scratch), buf)
    return rc if rc else dict(zip(CONV_SPLIT_FORM, buf))


@_op
def conv(x, wp, kind, M, H, W, isc=None, osc=None, bias=None, act=0, res=None, mask_ref=None, mask_gain=1.0, split=True):
    """H, W = LOW-resolution size (see te_hip.h).  x [B,K,Hin,Win].  split=False: no split-K workspace is handed over (what
    te_conv_f32 launches: the channel loop is not split).  res: residual added after the activation; mask_ref:
    leaky-ReLU gradient mask (saved output of the layer this data gradient lands on) applied last.  The kinds that read
    residual / mask (and TE_CONV_1X1S6 its input) with 16-byte accesses get aligned copies of misaligned operands."""
    x = x.contiguous()
    if kind == CONV_1X1S6:
        x = _aligned16(x)
    res = _aligned16(res.contiguous()) if res is not None else None
    mask_ref = _aligned16(mask_ref.contiguous()) if mask_ref is not None else None
    B, K = x.shape[0], x.shape[1]
    out = torch.empty(conv_out_shape(kind, B, M, H, W), device=x.device, dtype=x.dtype)
    if res is not None and tuple(res.shape) != tuple(out.shape):
        raise RuntimeError(f'te_hip: residual {tuple(res.shape)} does not match the convolution output {tuple(out.shape)}')
    if mask_ref is not None and tuple(mask_ref.shape) != tuple(out.shape):
        raise RuntimeError(f'te_hip: mask reference {tuple(mask_ref.shape)} does not match the convolution output {tuple(out.shape)}')
    S = lib().te_conv_splitk_count(kind, B, K, M, H, W)
    if S < 1:
        raise RuntimeError(f'te_conv_splitk_count failed ({S})')
    # small images split the channel loop over the grid: per-split slabs + fixed-order sum (deterministic, graph-capturable)
    ws = torch.empty((S,) + tuple(out.shape), device=x.device, dtype=x.dtype) if S > 1 and split else None
    if kind == CONV_T2S6:          # scratch for the last input column (body kernel -> edge kernel; te_hip.h)
        ws = torch.empty(B * K * H, device=x.device, dtype=x.dtype)
    _launch('te_conv_res_f32', _ptr(out), _ptr(ws), _ptr(x), _ptr(wp), _ptr(isc), _ptr(osc), _ptr(bias), _ptr(res), _ptr(mask_ref),
            mask_gain, act, kind, B, K, M, H, W)
    return out


@_op
def wgrad_slabs(g, x, kind, H, W, group=False, S=None, NB=None, out=None):
    """correlation slabs [B, S, Co, Ci, taps]; group=True (PLAIN gradient only - nothing per sample is derived from the slabs):
    [B / NB, S, Co, Ci, taps] with NB samples per slab where the plan finds that worthwhile (small images, big weights).
    S= / NB= (tests): the caller's chunk count and group size instead of the planners' - te_wgrad_f32 with S when NB is None,
    te_wgrad_group_f32 with S and NB otherwise (S is required then); slabs [B / NB, S, Co, Ci, taps], written into `out` when given
    (a contiguous tensor of that shape, e.g. a view inside a guarded buffer)."""
    g, x = g.contiguous(), x.contiguous()
    B, Co, Ci = g.shape[0], g.shape[1], x.shape[1]
    taps = 1 if kind == CONV_1X1 else 9
    if S is not None or NB is not None:
        if S is None or S < 1 or (NB is not None and (NB < 1 or B % NB)):
            raise RuntimeError(f'te_hip: wgrad_slabs needs S >= 1 and a group size that divides the batch (S={S}, NB={NB}, B={B})')
        shape = (B // (NB or 1), S, Co, Ci, taps)
        if out is not None and (tuple(out.shape) != shape or not out.is_contiguous() or out.dtype != g.dtype or out.device != g.device):
            raise RuntimeError(f'te_hip: wgrad_slabs out= must be a contiguous {shape} tensor like g')
        slabs = out if out is not None else torch.empty(shape, device=g.device, dtype=g.dtype)
        if NB is None:
            _launch('te_wgrad_f32', _ptr(slabs), _ptr(g), _ptr(x), kind, B, Co, Ci, H, W, S)
        else:
            _launch('te_wgrad_group_f32', _ptr(slabs), _ptr(g), _ptr(x), kind, B, Co, Ci, H, W, S, NB)
        return slabs
    if out is not None:
        raise RuntimeError('te_hip: wgrad_slabs out= needs an explicit S')
    if group:
        nb, sc = C.c_int(0), C.c_int(0)
        _check(lib().te_wgrad_group_plan(kind, B, Co, Ci, H, W, C.byref(nb), C.byref(sc)), 'te_wgrad_group_plan')
        if nb.value > 1:
            slabs = torch.empty(B // nb.value, sc.value, Co, Ci, taps, device=g.device, dtype=g.dtype)
            _launch('te_wgrad_group_f32', _ptr(slabs), _ptr(g), _ptr(x), kind, B, Co, Ci, H, W, sc.value, nb.value)
            return slabs
    S = lib().te_wgrad_slab_count(kind, B, Co, Ci, H, W)
    if S <= 0:
        raise RuntimeError(f'te_wgrad_slab_count failed ({S})')
    slabs = torch.empty(B, S, Co, Ci, taps, device=g.device, dtype=g.dtype)
    _launch('te_wgrad_f32', _ptr(slabs), _ptr(g), _ptr(x), kind, B, Co, Ci, H, W, S)
    return slabs


def wgrad_t2_wide(on=-1):
    """test and tool hook: form of the split transposed-kind weight-gradient kernel - 1 = 64 x 128 channels per block where
    Ci % 128 == 0 (default), 0 = 64 x 64 (bit-identical slabs); returns the previous value (-1: query only)"""
    return int(lib().te_wgrad_t2_wide(on))


def wgrad_split(on=-1):
    """switch of the split-bf16 weight-gradient kernels (csrc/wgrad6.hip), initialised from TE_SPLIT_BF16 and written by
    op/modconv.set_split_bf16: 0 / 1 sets it, returns the previous value (-1: query only).  The slab plan (wgrad_slabs) follows it, so
    the weight gradient is fp32-equivalent but not bit-identical across its values."""
    return int(lib().te_wgrad_split_bf16(on))


def wgrad_split_ok(kind, Co, Ci, H, W):
    """does the split-bf16 weight-gradient kernel cover this problem?  (taken only while wgrad_split() is on)"""
    return bool(lib().te_wgrad_split_supported(kind, Co, Ci, H, W))


WGRAD6_FORMS = ('fp32', 'w6', 'w6pair', 't2wide', 't2narrow', 't2masked', 'p1')      # te_wgrad6_form codes (te_hip.h)


def wgrad6_form(kind, B, Co, Ci, H, W, NB=1):
    """name of the kernel wgrad_slabs runs for this problem (16-byte aligned operands; NB samples per slab), see WGRAD6_FORMS"""
    return WGRAD6_FORMS[lib().te_wgrad6_form(kind, B, Co, Ci, H, W, NB)]


WGRAD_FORM = ('form6', 'nwp', 'wino', 'vec', 'db', 'TW', 'TH', 'tiles_x', 'tiles_y', 'grid_x', 'grid_y', 'grid_z', 'lds')      # te_wgrad_form (te_hip.h)


def wgrad_form(kind, B, Co, Ci, H, W, S, NB=1, g_mod16=0, x_mod16=0):
    """the plan of the wgrad_slabs launch with S chunks and NB samples per slab (host only): a dict of WGRAD_FORM - 'form6' is the
    te_wgrad6_form code of the kernel that runs (0: the fp32 kernel, which the other fields describe; they are zeros otherwise);
    the negative TE_ERR_* code where the launch refuses"""
    buf = (C.c_int * len(WGRAD_FORM))()
    rc = lib().te_wgrad_form(kind, B, Co, Ci, H, W, S, NB, g_mod16, x_mod16, buf)
    return rc if rc else dict(zip(WGRAD_FORM, buf))


def wgrad_pair_form(kind, Co, Ci, H, W):
    """does the weight-gradient kernel take the pair (Winograd F(3,2)) form for this problem?  (FLOP accounting only)"""
    return bool(lib().te_wgrad_pair_form(kind, Co, Ci, H, W))


@_op
def wgrad_reduce(slabs, w, wscale=1.0, isc=None, osc=None, want_w=True, want_isc=False, want_osc=False):
    B, S, Co, Ci, taps = slabs.shape
    dev, dt = slabs.device, slabs.dtype
    # all three outputs are WRITTEN (shares of different blocks meet in the workspace, summed in a fixed order: no atomics)
    gw = torch.empty(Co, Ci, taps, device=dev, dtype=dt) if want_w else None
    gisc = torch.empty(B, Ci, device=dev, dtype=dt) if want_isc else None
    gosc = torch.empty(B, Co, device=dev, dtype=dt) if want_osc else None
    n = lib().te_wgrad_reduce_ws_floats(B, S, Co, Ci, taps, int(want_w), int(want_isc), int(want_osc))
    if n < 0:
        raise RuntimeError(f'te_wgrad_reduce_ws_floats failed ({n})')
    ws = torch.empty(n, device=dev, dtype=dt) if n > 0 else None
    _launch('te_wgrad_reduce_f32', _ptr(gw), _ptr(gisc), _ptr(gosc), _ptr(ws), _ptr(slabs), _ptr(w.contiguous()), wscale, _ptr(isc),
            _ptr(osc), B, S, Co, Ci, taps)
    return gw, gisc, gosc


# --------------------------------------------------------------------------------------------- M3
def rgb_supported(M, K, HW):
    return bool(lib().te_rgb_supported(M, K, HW))


@_op
def rgb_fwd(x, w, isc, bias, wscale=1.0):
    """ToRGB forward [B,K,H,W] -> [B,3,H,W].  The kernel reads x with 16-byte accesses: a misaligned x goes in as an aligned copy."""
    x = _aligned16(x.contiguous())
    B, K, H, W = x.shape
    out = torch.empty(B, 3, H, W, device=x.device, dtype=x.dtype)
    _launch('te_rgb_fwd_f32', _ptr(out), _ptr(x), _ptr(w.contiguous()), _ptr(isc), _ptr(bias), wscale, B, K, H * W)
    return out


@_op
def rgb_dgrad(g, w, isc, K, wscale=1.0):
    """ToRGB data gradient [B,3,H,W] -> [B,K,H,W].  The kernel reads g with 16-byte accesses: a misaligned g goes in as an aligned
    copy."""
    g = _aligned16(g.contiguous())
    B, _, H, W = g.shape
    gx = torch.empty(B, K, H, W, device=g.device, dtype=g.dtype)
    _launch('te_rgb_dgrad_f32', _ptr(gx), _ptr(g), _ptr(w.contiguous()), _ptr(isc), wscale, B, K, H * W)
    return gx


@_op
def rgb_wgrad_sum_slabs(g3, x):
    """slabs [B,S,4,K]: rows 0-2 = sum_p g3[b,o,p] x[b,k,p], row 3 = sum_p x[b,k,p]"""
    g3, x = g3.contiguous(), x.contiguous()
    B, K, H, W = x.shape
    S = lib().te_rgb_wgrad_slab_count(B, K, H * W)
    slabs = torch.empty(B, S, 4, K, device=x.device, dtype=x.dtype)
    _launch('te_rgb_wgrad_sum_f32', _ptr(slabs), _ptr(g3), _ptr(x), B, K, H * W, S)
    return slabs


@_op
def rgb_expand(x3, w3k, bias, act, wscale=1.0):
    """from-RGB stem: x3 [B,3,H,W], w3k [3,K] -> act(wscale * sum_o w3k[o,k] x3[b,o] + bias[k])  [B,K,H,W].  The kernel reads x3
    with 16-byte accesses: a misaligned x3 goes in as an aligned copy."""
    x3 = _aligned16(x3.contiguous())
    B, _, H, W = x3.shape
    K = w3k.shape[1]
    out = torch.empty(B, K, H, W, device=x3.device, dtype=x3.dtype)
    _launch('te_rgb_expand_f32', _ptr(out), _ptr(x3), _ptr(w3k.contiguous()), _ptr(bias), act, wscale, B, K, H * W)
    return out


@_op
def rgb_wgrad_slabs(g, x):
    """correlation slabs [B,S,3,K,1] of the ToRGB weight gradient.  Operands go in as they come: the kernel itself stages a
    misaligned x through its scalar path (the same LDS tile, bit-identical slabs) and reads g element by element."""
    g, x = g.contiguous(), x.contiguous()
    B, K, H, W = x.shape
    S = lib().te_rgb_wgrad_slab_count(B, K, H * W)
    slabs = torch.empty(B, S, 3, K, 1, device=x.device, dtype=x.dtype)
    _launch('te_rgb_wgrad_f32', _ptr(slabs), _ptr(g), _ptr(x), B, K, H * W, S)
    return slabs


# --------------------------------------------------------------------------------------------- G2/A2
@_op
def small_gemm(I, J, K, a, sai, sak, b, sbk, sbj, bias=None, residual=None, alpha=1.0, beta=1.0, act=0, want_pre=False,
               rowsum_scale=None, out=None):
    """C[I,J] = act(alpha * A B + beta * bias) + residual with strided operands (see te_hip.h); a / b are the base
    tensors (contiguous storage, addressed through the element strides).  Returns (C, pre | None, rowsum | None);
    rowsum_scale != None asks for rowsum[i] = rowsum_scale * sum_k A(i,k).  out: the caller's (C, pre, rowsum) to write
    into (a test's views inside guard bands), each None where it is not wanted."""
    if out is not None:
        c, pre, rs = out
    else:
        c = torch.empty(I, J, device=a.device, dtype=a.dtype)
        pre = torch.empty_like(c) if want_pre else None
        rs = torch.empty(I, device=a.device, dtype=a.dtype) if rowsum_scale is not None else None
    # a / b are addressed through explicit strides: only device / dtype are checked
    _launch('te_small_gemm_f32', _ptr(c), _ptr(pre), _raw(a), _raw(b), _ptr(bias), _ptr(residual), _ptr(rs),
            rowsum_scale if rowsum_scale is not None else 0.0, I, J, K, sai, sak, sbk, sbj, alpha, beta, act)
    return c, pre, rs


@_op
def small_gemm_splitk(I, J, K, S, a, sai, sak, b, sbk, sbj, bias=None, residual=None, alpha=1.0, beta=1.0, act=0, want_pre=False,
                      out=None):
    """small_gemm for wide reductions: K in S chunks over the grid, fixed-order second pass (see te_hip.h).  out: the caller's
    (C, pre | None, workspace [S, I, J]) to write into."""
    if out is not None:
        c, pre, ws = out
    else:
        c = torch.empty(I, J, device=a.device, dtype=a.dtype)
        pre = torch.empty_like(c) if want_pre else None
        ws = torch.empty(S, I, J, device=a.device, dtype=a.dtype)
    _launch('te_small_gemm_splitk_f32', _ptr(c), _ptr(pre), _ptr(ws), S, _raw(a), _raw(b), _ptr(bias), _ptr(residual), I, J, K, sai, sak,
            sbk, sbj, alpha, beta, act)
    return c, pre


def small_gemm_form(I, J, K, nz, sai, sak, sbk, sbj, za=0, zb=0, b_tab=None, a_mod16=0, b_mod16=0, splitk=False):
    """(nw, av, bv, grid x, y, z) that the small_gemm launches plan for these arguments (host only; splitk: nz is S, the chunk plan);
    the negative TE_ERR_* code where they refuse"""
    buf = (C.c_int * 6)()
    bt = (C.c_int64 * max(len(b_tab), min(nz, 16)))(*b_tab) if b_tab is not None else None
    rc = lib().te_small_gemm_form(I, J, K, nz, sai, sak, sbk, sbj, za, zb, bt, a_mod16, b_mod16, int(splitk), buf)
    return rc if rc else tuple(buf)


@_op
def minibatch_stddev_fwd(x, group, eps, chunks=1):
    """x [B, C, H, W] -> y [B, C + 1, H, W] (input copied, stddev channel appended); `chunks` > 1: the batch is `chunks`
    independent minibatches laid end to end (one launch each on its slice)"""
    x = x.contiguous()
    B, Cn, H, W = x.shape
    y = torch.empty(B, Cn + 1, H, W, device=x.device, dtype=x.dtype)
    Bc = B // chunks
    for c in range(chunks):
        _launch('te_minibatch_stddev_fwd_f32', _ptr(y[c * Bc:(c + 1) * Bc]), _ptr(x[c * Bc:(c + 1) * Bc]), Bc, group, Cn, H * W, eps)
    return y


@_op
def minibatch_stddev_bwd(gy, x, group, eps, chunks=1):
    gy = gy.contiguous()
    B, Cn, H, W = x.shape
    gx = torch.empty_like(x)
    Bc = B // chunks
    for c in range(chunks):
        sl = slice(c * Bc, (c + 1) * Bc)
        _launch('te_minibatch_stddev_bwd_f32', _ptr(gx[sl]), _ptr(gy[sl]), _ptr(x[sl]), Bc, group, Cn, H * W, eps)
    return gx


@_op
def small_gemm_batched(c, a, b, bias, nz, za, zc, I, J, K, sai, sak, sbk, sbj, sci, scj, zb=0, zbias=0, b_tab=None,
                       bias_tab=None, alpha=1.0, beta=1.0, act=0):
    """nz GEMMs in one launch (see te_hip.h); c is written in place through (zc, sci, scj).  b_tab / bias_tab: lists of
    element offsets relative to b / bias for separately allocated per-z operands."""
    bt = (C.c_int64 * nz)(*b_tab) if b_tab is not None else None
    bit = (C.c_int64 * nz)(*bias_tab) if bias_tab is not None else None
    _launch('te_small_gemm_batched_f32', _raw(c), _raw(a), _raw(b), _raw(bias), nz, za, zc, zb, zbias, bt, bit, I, J, K, sai, sak, sbk, sbj,
            sci, scj, alpha, beta, act)
    return c


def layer_norm_supported(R, N):
    return bool(lib().te_layer_norm_supported(R, N))


@_op
def layer_norm_fwd(x2, eps):
    """x2 [R, N] contiguous -> (y [R, N], stats [R, 2])"""
    R, N = x2.shape
    y = torch.empty_like(x2)
    stats = torch.empty(R, 2, device=x2.device, dtype=x2.dtype)
    _launch('te_layer_norm_fwd_f32', _ptr(y), _ptr(stats), _ptr(x2), R, N, eps)
    return y, stats


@_op
def layer_norm_bwd(g2, y2, stats):
    R, N = y2.shape
    gx = torch.empty_like(y2)
    _launch('te_layer_norm_bwd_f32', _ptr(gx), _ptr(g2), _ptr(y2), _ptr(stats), R, N)
    return gx


def pixel_norm_supported(B, D, Cn):
    return bool(lib().te_pixel_norm_supported(B, D, Cn))


@_op
def pixel_norm_fwd(x, eps):
    """x [B, D, C] contiguous -> (y, r [B, C])"""
    B, D, Cn = x.shape
    y = torch.empty_like(x)
    r = torch.empty(B, Cn, device=x.device, dtype=x.dtype)
    _launch('te_pixel_norm_fwd_f32', _ptr(y), _ptr(r), _ptr(x), B, D, Cn, eps)
    return y, r


@_op
def pixel_norm_bwd(g, y, r):
    B, D, Cn = y.shape
    gx = torch.empty_like(y)
    _launch('te_pixel_norm_bwd_f32', _ptr(gx), _ptr(g), _ptr(y), _ptr(r), B, D, Cn)
    return gx


# --------------------------------------------------------------------------------------------- M1
@_op
def demod_fwd(w, s, wscale, eps):
    """w [Co,Ci,T] raw weights, s [B,Ci] -> (d [B,Co], wsq [Co,Ci])"""
    Co, Ci, T = w.shape
    B = s.shape[0]
    d = torch.empty(B, Co, device=w.device, dtype=w.dtype)
    wsq = torch.empty(Co, Ci, device=w.device, dtype=w.dtype)
    _launch('te_demod_fwd_f32', _ptr(d), _ptr(wsq), _ptr(w), _ptr(s), wscale, eps, B, Co, Ci, T)
    return d, wsq


@_op
def demod_from_wsq(wsq, s, eps):
    """d [B,Co] from a cached wsq [Co,Ci] (frozen weights: the 9-tap squares are not recomputed)"""
    Co, Ci = wsq.shape
    B = s.shape[0]
    d = torch.empty(B, Co, device=wsq.device, dtype=wsq.dtype)
    _launch('te_demod_fwd_f32', _ptr(d), None, _ptr(wsq), _ptr(s), 1.0, eps, B, Co, Ci, 0)
    return d


@_op
def demod_bwd(gd, d, w, wsq, s, wscale, want_w=True, want_s=True, into=None):
    """into = (gw, gs): accumulate into these existing gradients (either may be None) instead of allocating new ones."""
    Co, Ci, T = w.shape
    B = s.shape[0]
    if into is not None:
        gw, gs = into
    else:
        gw = torch.empty_like(w) if want_w else None
        gs = torch.empty_like(s) if want_s else None
    _launch('te_demod_bwd_f32', _ptr(gw), _ptr(gs), _ptr(gd.contiguous()), _ptr(d), _ptr(w), _ptr(wsq), _ptr(s), wscale, B, Co, Ci, T,
            1 if into is not None else 0)
    return gw, gs


# --------------------------------------------------------------------------------------------- F2
@_op
def attn_fwd(q, k, v, scale, groups):
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    N, M, Cn = q.shape
    L = k.shape[1]
    D = Cn // groups
    o = torch.empty_like(q)
    sim = torch.empty(N, groups, M, L, device=q.device, dtype=q.dtype)
    _launch('te_attn_fwd_f32', _ptr(o), _ptr(sim), _ptr(q), _ptr(k), _ptr(v), scale, N, groups, M, L, D)
    return o, sim


@_op
def attn_bwd(go, gsim, q, k, v, sim, scale, groups):
    N, M, Cn = q.shape
    L = k.shape[1]
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    _launch('te_attn_bwd_f32', _ptr(gq), _ptr(gk), _ptr(gv), _ptr(go.contiguous()), _ptr(gsim.contiguous()) if gsim is not None else None,
            _ptr(q), _ptr(k), _ptr(v), _ptr(sim), scale, N, groups, M, L, Cn // groups)
    return gq, gk, gv


# --------------------------------------------------------------------------------------------- T2
@_op
def mt_adam(table, chunks, n_tensors, n_chunks, chunk_elems, lr, beta1, beta2, eps, step):
    """table: int64 device tensor [5, n]; chunks: int32 device tensor [2, n_chunks] (see te_hip.h)"""
    _on_current_device(table)
    _launch('te_mt_adam_f32', table.data_ptr(), chunks.data_ptr(), n_tensors, n_chunks, chunk_elems, lr, beta1, beta2, eps, step)


@_op
def mt_ema(table, chunks, n_tensors, n_chunks, chunk_elems, decay):
    _on_current_device(table)
    _launch('te_mt_ema_f32', table.data_ptr(), chunks.data_ptr(), n_tensors, n_chunks, chunk_elems, float(decay))


@_op
def mt_ranger(table, work, n_tensors, n_work, tile_elems, step_lr, decay, beta1, beta2, eps, alpha, rectified, lookahead):
    """table: int64 device tensor [7, n]; work: int32 device tensor [3, n_work] of whole-row groups (see te_hip.h)"""
    _on_current_device(table)
    _launch('te_mt_ranger_f32', table.data_ptr(), work.data_ptr(), n_tensors, n_work, tile_elems, float(step_lr), float(decay),
            float(beta1), float(beta2), float(eps), float(alpha), int(bool(rectified)), int(bool(lookahead)))


# --------------------------------------------------------------------------------------------- channel scale / dot
@_op
def chan_scale(x, s):
    """x [B,C,...] * s[B,C] broadcast over the trailing dims"""
    x, s = x.contiguous(), s.contiguous()
    rows = x.shape[0] * x.shape[1]
    out = torch.empty_like(x)
    _launch('te_chan_scale_f32', _ptr(out), _ptr(x), _ptr(s), rows, x.numel() // max(rows, 1))
    return out


@_op
def chan_dot(a, b):
    """sum over the trailing dims of a * b -> [B,C]"""
    a, b = a.contiguous(), b.contiguous()
    rows = a.shape[0] * a.shape[1]
    out = torch.empty(a.shape[0], a.shape[1], device=a.device, dtype=a.dtype)
    _launch('te_chan_dot_f32', _ptr(out), _ptr(a), _ptr(b), rows, a.numel() // max(rows, 1))
    return out


# --------------------------------------------------------------------------------------------- L1 LPIPS-VGG pieces
@_op
def lpips_stem_fwd(x, w, b):
    """ScalingLayer -> conv1_1 -> bias -> ReLU: x [N,3,H,W] -> [N,64,H,W]"""
    x = x.contiguous()
    N, _, H, W = x.shape
    out = torch.empty(N, 64, H, W, device=x.device, dtype=x.dtype)
    _launch('te_lpips_stem_fwd_f32', _ptr(out), _ptr(x), _ptr(w), _ptr(b), N, H, W)
    return out


@_op
def lpips_stem_dgrad(g, y1, w):
    """data gradient of the stem w.r.t. the UNSCALED input (relu1_1 mask from its output y1)"""
    g = g.contiguous()
    N, _, H, W = g.shape
    gx = torch.empty(N, 3, H, W, device=g.device, dtype=g.dtype)
    _launch('te_lpips_stem_dgrad_f32', _ptr(gx), _ptr(g), _ptr(y1), _ptr(w), N, H, W)
    return gx


@_op
def maxpool2_fwd(x):
    x = x.contiguous()
    N, Cn, H, W = x.shape
    out = torch.empty(N, Cn, H // 2, W // 2, device=x.device, dtype=x.dtype)
    _launch('te_maxpool2_fwd_f32', _ptr(out), _ptr(x), N * Cn, H, W)
    return out


@_op
def maxpool2_bwd(g, x):
    g = g.contiguous()
    N, Cn, H, W = x.shape
    gx = torch.empty_like(x)
    _launch('te_maxpool2_bwd_f32', _ptr(gx), _ptr(g), _ptr(x), N * Cn, H, W)
    return gx


@_op
def lpips_normalize(x):
    x = x.contiguous()
    out = torch.empty_like(x)
    _launch('te_lpips_normalize_f32', _ptr(out), _ptr(x), x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
    return out


@_op
def lpips_head_fwd(f, t_hat, w):
    """per-block partial sums [N, blocks] of one layer's head (t_hat: normalised target features, batch N or 1)"""
    f = f.contiguous()
    N, Cn, H, W = f.shape
    nb = lib().te_lpips_head_blocks(H * W)
    partial = torch.empty(N, nb, device=f.device, dtype=f.dtype)
    _launch('te_lpips_head_fwd_f32', _ptr(partial), _ptr(f), _ptr(t_hat), _ptr(w), N, t_hat.shape[0], Cn, H * W)
    return partial


@_op
def lpips_dist(partials, hws):
    """d[N] = sum over layers (in order) of the spatial means"""
    L, N = len(partials), partials[0].shape[0]
    d = torch.empty(N, device=partials[0].device, dtype=torch.float32)
    ptrs = (C.c_void_p * L)(*[_ptr(p) for p in partials])
    hw = (C.c_int64 * L)(*hws)
    _launch('te_lpips_dist_f32', _ptr(d), ptrs, hw, L, N)
    return d


@_op
def lpips_head_bwd(gd, f, t_hat, w, gin=None, relu_mask=True):
    f = f.contiguous()
    N, Cn, H, W = f.shape
    gf = torch.empty_like(f)
    _launch('te_lpips_head_bwd_f32', _ptr(gf), _ptr(gin.contiguous()) if gin is not None else None, _ptr(gd.contiguous()), _ptr(f),
            _ptr(t_hat), _ptr(w), N, t_hat.shape[0], Cn, H * W, 1 if relu_mask else 0)
    return gf


@_op
def lpips_pair_head_fwd(f, w):
    """per-block partial sums [N, blocks] of one layer's head for an interleaved batch f [2N,C,H,W] (images 2n, 2n+1 are a pair)"""
    if f.shape[0] % 2:
        raise RuntimeError(f'te_hip: the paired LPIPS head needs an even batch, got {f.shape[0]}')
    f = f.contiguous()
    N, Cn, H, W = f.shape[0] // 2, f.shape[1], f.shape[2], f.shape[3]
    nb = lib().te_lpips_head_blocks(H * W)
    partial = torch.empty(N, nb, device=f.device, dtype=f.dtype)
    _launch('te_lpips_pair_head_fwd_f32', _ptr(partial), _ptr(f), _ptr(w), N, Cn, H * W)
    return partial


@_op
def crop_resize_bilinear(img, y0, x0, hc, wc, h, w):
    """window [y0:y0+hc, x0:x0+wc] of img [B,3,H,W], bilinear (align_corners=False) to [B,3,h,w]; hc / h and wc / w integers"""
    img = img.contiguous()
    B, Cn, H, W = img.shape
    if Cn != 3:
        raise RuntimeError(f'te_hip: crop_resize_bilinear expects [B,3,H,W] images, got {tuple(img.shape)}')
    out = torch.empty(B, 3, h, w, device=img.device, dtype=img.dtype)
    _launch('te_crop_resize_bilinear_f32', _ptr(out), _ptr(img), B, H, W, y0, x0, hc, wc, h, w)
    return out


# --------------------------------------------------------------------------------------------- L2 noise regulariser
def _noise_list(maps):
    n = len(maps)
    if n == 0:
        raise RuntimeError('te_hip: the noise regulariser needs at least one noise map')
    B = maps[0].shape[0]
    for m in maps:
        if m.ndim != 4 or m.shape[0] != B or m.shape[1] != 1 or m.shape[2] != m.shape[3]:
            raise RuntimeError(f'te_hip: noise maps must be [B,1,s,s] with one B, got {tuple(m.shape)}')
    ptrs = (C.c_void_p * n)(*[_ptr(m) for m in maps])
    sizes = (C.c_int * n)(*[m.shape[2] for m in maps])
    return ptrs, sizes, n, B


@_op
def noise_reg_fwd(maps):
    """-> (loss [1], workspace for noise_reg_bwd)"""
    ptrs, sizes, n, B = _noise_list(maps)
    nws = lib().te_noise_reg_ws_floats(sizes, n, B)
    if nws < 0:
        raise RuntimeError(f'te_noise_reg_ws_floats failed ({nws})')
    loss = torch.empty(1, device=maps[0].device, dtype=torch.float32)
    ws = torch.empty(nws, device=maps[0].device, dtype=torch.float32)
    _launch('te_noise_reg_fwd_f32', _ptr(loss), _ptr(ws), ptrs, sizes, n, B)
    return loss, ws


@_op
def noise_reg_bwd(gloss, ws, maps):
    ptrs, sizes, n, B = _noise_list(maps)
    grads = [torch.empty_like(m) for m in maps]
    gptrs = (C.c_void_p * n)(*[_ptr(g) for g in grads])
    tws = torch.empty_like(ws)
    _launch('te_noise_reg_bwd_f32', gptrs, _ptr(tws), _ptr(gloss.reshape(1).contiguous()), _ptr(ws), ptrs, sizes, n, B)
    return grads


@_op
def noise_normalize_(maps):
    ptrs, sizes, n, B = _noise_list(maps)
    _launch('te_noise_normalize_f32', ptrs, sizes, n, B)


# --------------------------------------------------------------------------------------------- M1 PRDC
def _features(t, what):
    if t.ndim != 2:
        raise RuntimeError(f'te_hip: {what} expects [N,D] features, got {tuple(t.shape)}')
    _ptr(t)
    return t.shape


def _prdc_ws(N, M, D, k, device):
    nb = lib().te_prdc_ws_bytes(N, M, D, k)
    if nb < 0:
        raise RuntimeError(f'te_prdc_ws_bytes failed ({nb}) for N={N}, M={M}, D={D}, k={k}: 1 <= k <= 15 and at least k + 1 rows per set')
    return torch.empty(nb // 4, device=device, dtype=torch.float32)


@_op
def row_sqnorm(x):
    """[N,D] -> the squared row norms [N]"""
    N, D = _features(x, 'row_sqnorm')
    out = torch.empty(N, device=x.device, dtype=torch.float32)
    _launch('te_row_sqnorm_f32', _ptr(out), _ptr(x), N, D)
    return out


@_op
def prdc_knn(x, nx, k):
    """squared distance of every row of x [N,D] to its k-th nearest other row (element k of the sorted row, diagonal 0) -> [N]"""
    N, D = _features(x, 'prdc_knn')
    if nx.shape != (N,):
        raise RuntimeError(f'te_hip: prdc_knn expects {N} row norms, got {tuple(nx.shape)}')
    ws = _prdc_ws(N, N, D, k, x.device)
    r2 = torch.empty(N, device=x.device, dtype=torch.float32)
    _launch('te_prdc_knn_f32', _ptr(r2), _ptr(x), _ptr(nx), N, D, k, _ptr(ws))
    return r2


@_op
def prdc_counts(x, nx, rr2, y, ny, rf2):
    """real x [N,D], fake y [M,D], their row norms and squared radii -> (col_count [M] int32, row_any [N] int32, row_min [N])"""
    N, D = _features(x, 'prdc_counts')
    M, Dy = _features(y, 'prdc_counts')
    if Dy != D or nx.shape != (N,) or rr2.shape != (N,) or ny.shape != (M,) or rf2.shape != (M,):
        raise RuntimeError(f'te_hip: prdc_counts: inconsistent shapes x {tuple(x.shape)}, y {tuple(y.shape)}, nx {tuple(nx.shape)}, '
                           f'rr2 {tuple(rr2.shape)}, ny {tuple(ny.shape)}, rf2 {tuple(rf2.shape)}')
    ws = _prdc_ws(N, M, D, 1, x.device)
    col_count = torch.empty(M, device=x.device, dtype=torch.int32)
    row_any = torch.empty(N, device=x.device, dtype=torch.int32)
    row_min = torch.empty(N, device=x.device, dtype=torch.float32)
    _launch('te_prdc_counts_f32', _ptr_as(col_count, torch.int32), _ptr_as(row_any, torch.int32), _ptr(row_min), _ptr(x), _ptr(nx),
            _ptr(rr2), _ptr(y), _ptr(ny), _ptr(rf2), N, M, D, _ptr(ws))
    return col_count, row_any, row_min


# --------------------------------------------------------------------------------------------- M2 VGG16 fc7 features
@_op
def vgg_stem_fwd(x, w, b):
    """conv1_1 -> bias -> ReLU on the raw input (no ScalingLayer): x [N,3,H,W] -> [N,64,H,W]"""
    x = x.contiguous()
    N, _, H, W = x.shape
    out = torch.empty(N, 64, H, W, device=x.device, dtype=x.dtype)
    _launch('te_vgg_stem_fwd_f32', _ptr(out), _ptr(x), _ptr(w), _ptr(b), N, H, W)
    return out


@_op
def adaptive_avgpool(x, OH=7, OW=7):
    """torch's adaptive_avg_pool2d: x [N,C,H,W] -> [N,C,OH,OW] (contiguous: .view(N, -1) is the flattened layout)"""
    x = x.contiguous()
    N, Cn, H, W = x.shape
    out = torch.empty(N, Cn, OH, OW, device=x.device, dtype=x.dtype)
    _launch('te_adaptive_avgpool_f32', _ptr(out), _ptr(x), N * Cn, H, W, OH, OW)
    return out


def fc_stream_splits(J, K):
    """the number of K chunks te_fc_stream_f32 uses for a [J,K] weight (no batch size enters)"""
    S = lib().te_fc_stream_splits(J, K)
    if S < 0:
        raise RuntimeError(f'te_fc_stream_splits failed ({S}) for J={J}, K={K}: J >= 1, K a positive multiple of 4')
    return S


@_op
def fc_stream(a, w, bias, act=0):
    """act(a @ w.T + bias): a [I,K], w [J,K] (torch Linear layout), bias [J] -> [I,J]; act 0 none, 1 ReLU.  The ABI refuses bad shapes
    and misaligned operands; nothing is launched then."""
    if a.ndim != 2 or w.ndim != 2 or bias.ndim != 1 or a.shape[1] != w.shape[1] or bias.shape[0] != w.shape[0]:
        raise RuntimeError(f'te_hip: fc_stream: inconsistent shapes a {tuple(a.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}')
    (I, K), J = a.shape, w.shape[0]
    nb = lib().te_fc_stream_ws_bytes(I, J, K)
    c = torch.empty(I, J, device=a.device, dtype=a.dtype)
    ws = torch.empty(max(nb, 4) // 4, device=a.device, dtype=a.dtype)        # (nb < 0: the call below names what is wrong)
    _launch('te_fc_stream_f32', _ptr(c), _ptr(ws), _ptr(a), _ptr(w), _ptr(bias), I, J, K, act)
    return c


# --------------------------------------------------------------------------------------------- M3 FID feature moments
def fid_moments_ws_bytes(N, D):
    nb = lib().te_fid_moments_ws_bytes(N, D)
    if nb < 0:
        raise RuntimeError(f'te_fid_moments_ws_bytes failed ({nb}) for N={N}, D={D}: N >= 1 and 1 <= D <= 8192')
    return nb


@_op
def fid_moments(S, s, x, accumulate):
    """S [D,D] fp64 (upper triangle) and s [D] fp64 (+)= the second and first moments of the rows of x [N,D] fp32; in place"""
    N, D = _features(x, 'fid_moments')
    if S.shape != (D, D) or s.shape != (D,):
        raise RuntimeError(f'te_hip: fid_moments: x {tuple(x.shape)} needs S [{D},{D}] and s [{D}], got {tuple(S.shape)} and {tuple(s.shape)}')
    nb = fid_moments_ws_bytes(N, D)
    ws = torch.empty(nb // 8, device=x.device, dtype=torch.float64) if nb else None
    _launch('te_fid_moments_f64', _ptr_as(S, torch.float64), _ptr_as(s, torch.float64), _ptr_as(ws, torch.float64), _ptr(x), N, D,
            1 if accumulate else 0)


@_op
def fid_finalize(S, s, n):
    """the moments of n samples -> (mean [D], cov [D,D]) fp64 on the device: np.mean / np.cov(rowvar=False)"""
    if S.ndim != 2 or S.shape[0] != S.shape[1] or s.shape != (S.shape[0],):
        raise RuntimeError(f'te_hip: fid_finalize expects S [D,D] and s [D], got {tuple(S.shape)} and {tuple(s.shape)}')
    D = S.shape[0]
    mean = torch.empty(D, device=S.device, dtype=torch.float64)
    cov = torch.empty(D, D, device=S.device, dtype=torch.float64)
    _launch('te_fid_finalize_f64', _ptr_as(mean, torch.float64), _ptr_as(cov, torch.float64), _ptr_as(S, torch.float64),
            _ptr_as(s, torch.float64), int(n), D)
    return mean, cov


# --------------------------------------------------------------------------------------------- E1 linear SVM of an editing boundary
def _labels(y, n, what):
    """n labels +1 / -1 on the HOST (a numpy array, a CPU tensor or a sequence) -> a contiguous int8 ctypes array"""
    import numpy as np
    if torch.is_tensor(y):
        if y.is_cuda:
            raise RuntimeError(f'te_hip: {what}: the labels are a host array (the ABI validates them before it launches), got {y.device}')
        y = y.numpy()
    y = np.ascontiguousarray(y, dtype=np.int8)
    if y.shape != (n,):
        raise RuntimeError(f'te_hip: {what} expects {n} labels, got {tuple(y.shape)}')
    return y


@_op
def gram(x):
    """x [n,D] -> K = x x^T [n,n], bitwise symmetric"""
    n, D = _features(x, 'gram')
    K = torch.empty(n, n, device=x.device, dtype=torch.float32)
    _launch('te_gram_f32', _ptr(K), _ptr(x), n, D)
    return K


@_op
def svm_smo(K, y, C_=1.0, eps=1e-3, max_iter=1_000_000):
    """the C-SVC dual on the Gram matrix K [n,n] with HOST labels y (+1 / -1) -> (alpha [n] fp64, rho [1] fp64, info [2] int32 =
    (iterations, converged)), all on the device; nothing synchronises"""
    if K.ndim != 2 or K.shape[0] != K.shape[1]:
        raise RuntimeError(f'te_hip: svm_smo expects a square Gram matrix, got {tuple(K.shape)}')
    n = K.shape[0]
    y = _labels(y, n, 'svm_smo')
    alpha = torch.empty(n, device=K.device, dtype=torch.float64)
    rho = torch.empty(1, device=K.device, dtype=torch.float64)
    info = torch.empty(2, device=K.device, dtype=torch.int32)
    _launch('te_svm_smo_f64', _ptr_as(alpha, torch.float64), _ptr_as(rho, torch.float64), _ptr_as(info, torch.int32), _ptr(K),
            y.ctypes.data, n, float(C_), float(eps), int(max_iter))
    return alpha, rho, info


@_op
def svm_coef(x, alpha, y):
    """w [D] = sum_i alpha_i y_i x[i,:] (fp64 accumulation, one rounding): x [n,D] fp32, alpha [n] fp64, HOST labels y"""
    n, D = _features(x, 'svm_coef')
    if alpha.shape != (n,):
        raise RuntimeError(f'te_hip: svm_coef expects {n} alphas, got {tuple(alpha.shape)}')
    y = _labels(y, n, 'svm_coef')
    w = torch.empty(D, device=x.device, dtype=torch.float32)
    _launch('te_svm_coef_f32', _ptr(w), _ptr(x), _ptr_as(alpha, torch.float64), y.ctypes.data, n, D)
    return w


# --------------------------------------------------------------------------------------------- M4 Inception-v3 pool3 features
POOL3_MAX_S2, POOL3_MAX_S1, POOL3_AVG_S1 = 0, 1, 2


def conv2d_out_hw(H, W, kh, kw, stride=1, pad=(0, 0)):
    return (H + 2 * pad[0] - kh) // stride + 1, (W + 2 * pad[1] - kw) // stride + 1


def _slice_out(out, c0, B, Cn, Ho, Wo, like, what):
    """the [B,Ctot,Ho,Wo] tensor a slice [c0, c0 + Cn) is written into: a new [B,Cn,Ho,Wo] one where none is given"""
    if out is None:
        if c0 != 0:
            raise RuntimeError(f'te_hip: {what}: c0 = {c0} needs the output tensor it indexes')
        return torch.empty(B, Cn, Ho, Wo, device=like.device, dtype=like.dtype)
    if out.ndim != 4 or out.shape[0] != B or tuple(out.shape[2:]) != (Ho, Wo):
        raise RuntimeError(f'te_hip: {what}: the output must be [{B},Ctot,{Ho},{Wo}], got {tuple(out.shape)}')
    return out


def _conv2d_geometry(who, x, w, bias, stride, pad, out=None, c0=0, also=None, more=''):
    """the x / w / bias check of the ops on the conv2d loop (`also`: what else the op needs to hold, `more`: its part of the message) ->
    (B, Ci, Co, H, W, kh, kw, stride, py, px) as the ABI takes them, the output tensor (_slice_out) and (Ho, Wo), which the ABI refuses
    where they are not positive"""
    if x.ndim != 4 or w.ndim != 4 or bias.ndim != 1 or x.shape[1] != w.shape[1] or bias.shape[0] != w.shape[0] or (also and not also()):
        raise RuntimeError(f'te_hip: {who}: inconsistent shapes x {tuple(x.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}{more}')
    (B, Ci, H, W), (Co, _, kh, kw) = x.shape, w.shape
    Ho, Wo = conv2d_out_hw(H, W, kh, kw, stride, pad)
    return (B, Ci, Co, H, W, kh, kw, stride, pad[0], pad[1]), _slice_out(out, c0, B, Co, max(Ho, 0), max(Wo, 0), x, who), (Ho, Wo)


@_op
def conv2d(x, w, bias, stride=1, pad=(0, 0), act=0, out=None, c0=0):
    """act(conv2d(x, w, stride, pad) + bias) written into channels [c0, c0 + Co) of `out` [B,Ctot,Ho,Wo] (a new [B,Co,Ho,Wo] tensor
    where out is None): x [B,Ci,H,W], w [Co,Ci,kh,kw], bias [Co]; act 0 none, 1 ReLU.  The ABI refuses what it does not cover (a
    stride above 2, a kernel above 7 x 7, padding >= the kernel, an empty output, a slice past Ctot); nothing is launched then.
    Returns out."""
    geo, out, _ = _conv2d_geometry('conv2d', x, w, bias, stride, pad, out, c0)
    _launch('te_conv2d_f32', _ptr(out), _ptr(x), _ptr(w), _ptr(bias), *geo, out.shape[1], c0, act)
    return out


@_op
def pool3(x, mode, out=None, c0=0):
    """3 x 3 pooling of x [B,C,H,W] into channels [c0, c0 + C) of `out`: POOL3_MAX_S2 (max, stride 2, no padding), POOL3_MAX_S1 (max,
    stride 1, pad 1) or POOL3_AVG_S1 (average, stride 1, pad 1, over the taps inside the image).  Returns out."""
    if x.ndim != 4:
        raise RuntimeError(f'te_hip: pool3 expects [B,C,H,W], got {tuple(x.shape)}')
    B, Cn, H, W = x.shape
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == POOL3_MAX_S2 else (H, W)
    out = _slice_out(out, c0, B, Cn, max(Ho, 0), max(Wo, 0), x, 'pool3')
    _launch('te_pool3_f32', _ptr(out), _ptr(x), B, Cn, H, W, mode, out.shape[1], c0)
    return out


@_op
def resize_bilinear(x, OH, OW):
    """F.interpolate(x, (OH, OW), mode='bilinear', align_corners=False) of x [B,C,H,W]"""
    if x.ndim != 4:
        raise RuntimeError(f'te_hip: resize_bilinear expects [B,C,H,W], got {tuple(x.shape)}')
    x = x.contiguous()
    B, Cn, H, W = x.shape
    out = torch.empty(B, Cn, OH, OW, device=x.device, dtype=x.dtype)
    _launch('te_resize_bilinear_f32', _ptr(out), _ptr(x), B * Cn, H, W, OH, OW)
    return out


# --------------------------------------------------------------------------------------------- M5 DEX age / gender scorer
CLS_EXPECTATION, CLS_FIRST = 0, 1


@_op
def dex_stem_fwd(img, w, b, crop):
    """RGB [-1, 1] -> BGR byte levels -> centre crop -> conv1_1 -> bias -> ReLU: img [N,3,H,W] -> [N,64,crop,crop].  The ABI refuses a
    crop that does not fit or is not centred (an odd H - crop or W - crop); nothing is launched then."""
    img = img.contiguous()
    N, _, H, W = img.shape
    out = torch.empty(N, 64, max(crop, 0), max(crop, 0), device=img.device, dtype=img.dtype)
    _launch('te_dex_stem_fwd_f32', _ptr(out), _ptr(img), _ptr(w), _ptr(b), N, H, W, crop)
    return out


@_op
def cls_score(a, w, bias, mode, want_prob=False):
    """p = softmax(a @ w.T + bias) over the classes: a [I,K], w [C,K] (torch Linear layout), bias [C] -> score [I] = sum_c (c + 1) p_c
    (CLS_EXPECTATION) or p_0 (CLS_FIRST); want_prob: -> (score, p [I,C]).  The ABI refuses C > 1024, K % 4 != 0 and misaligned
    operands; nothing is launched then."""
    if a.ndim != 2 or w.ndim != 2 or bias.ndim != 1 or a.shape[1] != w.shape[1] or bias.shape[0] != w.shape[0]:
        raise RuntimeError(f'te_hip: cls_score: inconsistent shapes a {tuple(a.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}')
    (I, K), Cn = a.shape, w.shape[0]
    score = torch.empty(I, device=a.device, dtype=a.dtype)
    prob = torch.empty(I, Cn, device=a.device, dtype=a.dtype) if want_prob else None
    _launch('te_cls_score_f32', _ptr(score), _ptr(prob), _ptr(a), _ptr(w), _ptr(bias), I, Cn, K, mode)
    return (score, prob) if want_prob else score


# --------------------------------------------------------------------------------------------- M6 CelebA-HQ attribute classifier
@_op
def attr_stem_fwd(img, w, b, R, preprocessed=False):
    """RGB [-1, 1] -> BGR byte levels (preprocessed: img already is) -> f x f box mean, f = S / R -> 1x1 convolution -> bias ->
    leaky ReLU 0.2: img [N,3,S,S], w [C0,3] (scaled), b [C0] -> [N,C0,R,R].  The ABI refuses an S that is no multiple of R and
    C0 > 1024; nothing is launched then."""
    if img.ndim != 4 or img.shape[1] != 3 or img.shape[2] != img.shape[3] or w.ndim != 2 or w.shape[1] != 3 or b.shape != (w.shape[0],):
        raise RuntimeError(f'te_hip: attr_stem_fwd: inconsistent shapes img {tuple(img.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}')
    img = img.contiguous()
    N, S, C0 = img.shape[0], img.shape[2], w.shape[0]
    out = torch.empty(N, C0, max(R, 0), max(R, 0), device=img.device, dtype=img.dtype)
    _launch('te_attr_stem_fwd_f32', _ptr(out), _ptr(img), _ptr(w), _ptr(b), N, S, R, C0, 1 if preprocessed else 0)
    return out


@_op
def avgpool2_act(x, slope=1.0):
    """2 x 2 average pool, then v > 0 ? v : slope * v (slope 1: the plain pool): x [N,C,H,W] -> [N,C,H/2,W/2]"""
    if x.ndim != 4:
        raise RuntimeError(f'te_hip: avgpool2_act expects [N,C,H,W], got {tuple(x.shape)}')
    x = x.contiguous()
    N, Cn, H, W = x.shape
    out = torch.empty(N, Cn, H // 2, W // 2, device=x.device, dtype=x.dtype)
    _launch('te_avgpool2_act_f32', _ptr(out), _ptr(x), N * Cn, H, W, slope)
    return out


@_op
def attr_score(a, w, bias, slope=0.2, want_logit=True, want_score=True):
    """logit = bias + act(a) @ w, score = 1 / (1 + exp(2 logit)): a [I,K] (dense0's output before its activation), w [K] (scaled),
    bias [1] -> (logit [I] or None, score [I] or None).  The ABI refuses K % 4 != 0 and misaligned operands; nothing is launched
    then."""
    if a.ndim != 2 or w.ndim != 1 or a.shape[1] != w.shape[0] or bias.shape != (1,):
        raise RuntimeError(f'te_hip: attr_score: inconsistent shapes a {tuple(a.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}')
    I, K = a.shape
    logit = torch.empty(I, device=a.device, dtype=a.dtype) if want_logit else None
    score = torch.empty(I, device=a.device, dtype=a.dtype) if want_score else None
    _launch('te_attr_score_f32', _ptr(logit), _ptr(score), _ptr(a), _ptr(w), _ptr(bias), I, K, slope)
    return logit, score


# --------------------------------------------------------------------------------------------- M7 ResNet-18 pose classifier
@_op
def conv2d_res(x, w, bias, res, stride=1, pad=(0, 0), act=1):
    """act((conv2d(x, w, stride, pad) + bias) + res), the end of a ResNet BasicBlock: x [B,Ci,H,W], w [Co,Ci,kh,kw], bias [Co],
    res [B,Co,Ho,Wo] -> a new [B,Co,Ho,Wo] tensor, bitwise relu(conv2d(act=0) + res).  The ABI refuses what te_conv2d_f32 refuses;
    nothing is launched then."""
    geo, out, (Ho, Wo) = _conv2d_geometry('conv2d_res', x, w, bias, stride, pad)
    if tuple(res.shape) != (*out.shape[:2], Ho, Wo):
        raise RuntimeError(f'te_hip: conv2d_res: the residual must be [{out.shape[0]},{out.shape[1]},{Ho},{Wo}], got {tuple(res.shape)}')
    _launch('te_conv2d_res_f32', _ptr(out), _ptr(x), _ptr(w), _ptr(bias), _ptr(res), *geo, act)
    return out


@_op
def pose_stem_fwd(img, w, b, crop, preprocessed=False):
    """RGB [-1, 1] -> BGR byte levels (preprocessed: img already is) -> centre crop -> 7x7 stride-2 pad-3 convolution -> bias -> ReLU:
    img [N,3,H,W], w [Co,3,7,7], b [Co] -> [N,Co,Hc,Hc], Hc = (crop - 1) // 2 + 1.  The ABI refuses a crop that does not fit or is not
    centred (an odd H - crop or W - crop); nothing is launched then."""
    if img.ndim != 4 or img.shape[1] != 3 or w.ndim != 4 or tuple(w.shape[1:]) != (3, 7, 7) or b.shape != (w.shape[0],):
        raise RuntimeError(f'te_hip: pose_stem_fwd: inconsistent shapes img {tuple(img.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}')
    img = img.contiguous()
    (N, _, H, W), Co = img.shape, w.shape[0]
    Hc = (max(crop, 1) - 1) // 2 + 1
    out = torch.empty(N, Co, Hc, Hc, device=img.device, dtype=img.dtype)
    _launch('te_pose_stem_fwd_f32', _ptr(out), _ptr(img), _ptr(w), _ptr(b), N, H, W, crop, Co, 1 if preprocessed else 0)
    return out


@_op
def maxpool3s2p1(x):
    """nn.MaxPool2d(3, 2, 1): x [N,C,H,W] -> [N,C,(H - 1) // 2 + 1,(W - 1) // 2 + 1]; the padding never wins, a NaN propagates"""
    if x.ndim != 4:
        raise RuntimeError(f'te_hip: maxpool3s2p1 expects [N,C,H,W], got {tuple(x.shape)}')
    x = x.contiguous()
    N, Cn, H, W = x.shape
    out = torch.empty(N, Cn, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device=x.device, dtype=x.dtype)
    _launch('te_maxpool3s2p1_f32', _ptr(out), _ptr(x), N * Cn, H, W)
    return out


# --------------------------------------------------------------------------------------------- M8 AlexNet LPIPS (diversity score)
@_op
def alex_stem_fwd(img, w, b):
    """(x - mu) / sigma -> 11x11 stride-4 pad-2 convolution -> bias -> ReLU: img [N,3,H,W], w [Co,3,11,11], b [Co] ->
    [N,Co,(H - 7) // 4 + 1,(W - 7) // 4 + 1].  The ABI refuses an image below 7 px; nothing is launched then."""
    if img.ndim != 4 or img.shape[1] != 3 or w.ndim != 4 or tuple(w.shape[1:]) != (3, 11, 11) or b.shape != (w.shape[0],):
        raise RuntimeError(f'te_hip: alex_stem_fwd: inconsistent shapes img {tuple(img.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}')
    img = img.contiguous()
    (N, _, H, W), Co = img.shape, w.shape[0]
    Ho, Wo = conv2d_out_hw(H, W, 11, 11, 4, (2, 2))
    out = torch.empty(N, Co, max(Ho, 0), max(Wo, 0), device=img.device, dtype=img.dtype)
    _launch('te_alex_stem_fwd_f32', _ptr(out), _ptr(img), _ptr(w), _ptr(b), N, H, W, Co)
    return out


@_op
def lpips_unit(f, out=None):
    """f * rsqrt(sum_c f^2 + 1e-10) of f [N,C,H,W] (or [N,C,HW]); out=f normalises in place"""
    if f.ndim not in (3, 4):
        raise RuntimeError(f'te_hip: lpips_unit expects [N,C,H,W] or [N,C,HW], got {tuple(f.shape)}')
    if out is None:
        out = torch.empty_like(f)
    _launch('te_lpips_unit_f32', _ptr(out), _ptr(f), f.shape[0], f.shape[1], f[0, 0].numel())
    return out


@_op
def lpips_allpairs_fwd(fh, w):
    """one layer's per-block partials of the all-pairs head for normalised taps fh [N,C,H,W] (or [N,C,HW]) and the head w [C]: a flat
    workspace of te_lpips_allpairs_ws_floats(N, C, HW) floats that lpips_allpairs_dist reads"""
    if fh.ndim not in (3, 4) or w.ndim != 1 or w.shape[0] != fh.shape[1]:
        raise RuntimeError(f'te_hip: lpips_allpairs_fwd: inconsistent shapes fh {tuple(fh.shape)}, w {tuple(w.shape)}')
    N, Cn, HW = fh.shape[0], fh.shape[1], fh[0, 0].numel()
    n = lib().te_lpips_allpairs_ws_floats(N, Cn, HW)
    if n < 0:
        raise RuntimeError(f'te_hip: lpips_allpairs_fwd: a group of {N} taps of {HW} pixels is outside the limits (1 <= N < 65536)')
    partial = torch.empty(n, device=fh.device, dtype=fh.dtype)
    _launch('te_lpips_allpairs_fwd_f32', _ptr(partial), _ptr(fh), _ptr(w), N, Cn, HW)
    return partial


@_op
def lpips_allpairs_dist(partials, shapes, N):
    """D [N,N] = sum over the layers (in order) of the pairs' spatial means; shapes: each layer's (C, HW), as its partials were made"""
    L = len(partials)
    D = torch.empty(N, N, device=partials[0].device, dtype=torch.float32)
    ptrs = (C.c_void_p * L)(*[_ptr(p) for p in partials])
    cs = (C.c_int * L)(*[s[0] for s in shapes])
    hw = (C.c_int64 * L)(*[s[1] for s in shapes])
    for p, (Cn, HW) in zip(partials, shapes):
        if p.numel() != lib().te_lpips_allpairs_ws_floats(N, Cn, HW):
            raise RuntimeError(f'te_hip: lpips_allpairs_dist: {p.numel()} partials are not those of a group of {N} taps [{Cn},{HW}]')
    _launch('te_lpips_allpairs_dist_f32', _ptr(D), ptrs, cs, hw, L, N)
    return D


# --------------------------------------------------------------------------------------------- M9 ArcFace IR-SE50 identity network
def _conv2d_prelu(who, keep, x, w, bias, slope, in_scale, in_shift, stride, pad):
    geo, out, _ = _conv2d_geometry(
        who, x, w, bias, stride, pad,
        also=lambda: slope.shape == (w.shape[0],) and all(t is None or t.shape == (x.shape[1],) for t in (in_scale, in_shift)),
        more=f', slope {tuple(slope.shape)}, affine {[None if t is None else tuple(t.shape) for t in (in_scale, in_shift)]}')
    pre = [torch.empty_like(out)] if keep else []
    _launch(f'te_{who}_f32', _ptr(out), *map(_ptr, pre), _ptr(x), _ptr(w), _ptr(bias), _ptr(slope), _ptr(in_scale), _ptr(in_shift), *geo)
    return (out, *pre) if keep else out


@_op
def conv2d_prelu(x, w, bias, slope, in_scale=None, in_shift=None, stride=1, pad=(0, 0)):
    """prelu(conv2d(v, w, stride, pad) + bias, slope) with v = in_scale[c] * x + in_shift[c] inside the image and 0 in the padding (both
    None: v = x): x [B,Ci,H,W], w [Co,Ci,kh,kw], bias, slope [Co], in_scale, in_shift [Ci] -> a new [B,Co,Ho,Wo] tensor.  The ABI
    refuses what te_conv2d_f32 refuses and an affine given by half; nothing is launched then."""
    return _conv2d_prelu('conv2d_prelu', False, x, w, bias, slope, in_scale, in_shift, stride, pad)


def _id_stem(who, keep, img, w, b, slope, box, pool):
    if img.ndim != 4 or img.shape[1] != 3 or w.ndim != 4 or tuple(w.shape[1:]) != (3, 3, 3) or b.shape != (w.shape[0],) \
            or slope.shape != (w.shape[0],):
        raise RuntimeError(f'te_hip: {who}: inconsistent shapes img {tuple(img.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}, '
                           f'slope {tuple(slope.shape)}')
    img = img.contiguous()
    (N, _, H, W), Co = img.shape, w.shape[0]
    y0, y1, x0, x1 = box
    out = torch.empty(N, Co, max(pool, 0), max(pool, 0), device=img.device, dtype=img.dtype)
    pre = [torch.empty_like(out)] if keep else []
    _launch(f'te_{who}_f32', _ptr(out), *map(_ptr, pre), _ptr(img), _ptr(w), _ptr(b), _ptr(slope), N, H, W, y0, y1, x0, x1, pool, Co)
    return (out, *pre) if keep else out


@_op
def id_stem_fwd(img, w, b, slope, box, pool):
    """the window box = (y0, y1, x0, x1) of img [N,3,H,W] -> adaptive average to pool x pool -> 3x3 pad-1 convolution -> bias -> PReLU:
    w [Co,3,3,3], b, slope [Co] -> [N,Co,pool,pool].  The ABI refuses an empty window and one outside the image; nothing is launched
    then."""
    return _id_stem('id_stem_fwd', False, img, w, b, slope, box, pool)


@_op
def se_excite(pooled, w1, w2):
    """sigmoid(relu(pooled @ w1.T) @ w2.T): pooled [B,C], w1 [R,C], w2 [C,R] -> the gates [B,C]"""
    if pooled.ndim != 2 or w1.ndim != 2 or w2.ndim != 2 or w1.shape[1] != pooled.shape[1] or tuple(w2.shape) != (w1.shape[1], w1.shape[0]):
        raise RuntimeError(f'te_hip: se_excite: inconsistent shapes pooled {tuple(pooled.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}')
    (B, Cn), R = pooled.shape, w1.shape[0]
    gate = torch.empty(B, Cn, device=pooled.device, dtype=pooled.dtype)
    _launch('te_se_excite_f32', _ptr(gate), _ptr(pooled), _ptr(w1), _ptr(w2), B, Cn, R)
    return gate


@_op
def se_scale_add(res, gate, sc, stride=1):
    """res * gate[:, :, None, None] + sc[:, :, ::stride, ::stride] (gate None: res + sc[...]): res [B,C,Ho,Wo], gate [B,C],
    sc [B,C,Hs,Ws] -> a new [B,C,Ho,Wo] tensor.  The ABI refuses a shortcut whose size does not match; nothing is launched then."""
    if res.ndim != 4 or sc.ndim != 4 or tuple(sc.shape[:2]) != tuple(res.shape[:2]) or gate is not None and tuple(gate.shape) != tuple(res.shape[:2]):
        raise RuntimeError(f'te_hip: se_scale_add: inconsistent shapes res {tuple(res.shape)}, gate '
                           f'{None if gate is None else tuple(gate.shape)}, sc {tuple(sc.shape)}')
    (B, Cn, Ho, Wo), (Hs, Ws) = res.shape, sc.shape[2:]
    out = torch.empty_like(res)
    _launch('te_se_scale_add_f32', _ptr(out), _ptr(res), _ptr(gate), _ptr(sc), B, Cn, Ho, Wo, Hs, Ws, stride)
    return out


@_op
def rows_unit(a):
    """a / ||a||_2 per row of a [I,D] (the norm's square summed in fp64); a zero row gives NaN"""
    if a.ndim != 2:
        raise RuntimeError(f'te_hip: rows_unit expects [I,D], got {tuple(a.shape)}')
    out = torch.empty_like(a)
    _launch('te_rows_unit_f32', _ptr(out), _ptr(a), a.shape[0], a.shape[1])
    return out


@_op
def rows_dot(a, b):
    """sum_d a[i,d] * b[i,d] of a, b [I,D] -> [I]"""
    if a.ndim != 2 or tuple(a.shape) != tuple(b.shape):
        raise RuntimeError(f'te_hip: rows_dot expects two [I,D] tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}')
    out = torch.empty(a.shape[0], device=a.device, dtype=a.dtype)
    _launch('te_rows_dot_f32', _ptr(out), _ptr(a), _ptr(b), a.shape[0], a.shape[1])
    return out


# --------------------------------------------------------------------------------------------- M9b the identity network's backward pass
@_op
def conv2d_prelu_keep(x, w, bias, slope, in_scale=None, in_shift=None, stride=1, pad=(0, 0)):
    """conv2d_prelu that also returns the pre-activation: -> (out, pre), out bitwise conv2d_prelu's, out = prelu(pre, slope)"""
    return _conv2d_prelu('conv2d_prelu_keep', True, x, w, bias, slope, in_scale, in_shift, stride, pad)


@_op
def id_stem_keep(img, w, b, slope, box, pool):
    """id_stem_fwd that also returns the pre-activation: -> (out, pre)"""
    return _id_stem('id_stem_keep', True, img, w, b, slope, box, pool)


def dgrad_phases(k, stride, pad):
    """per output parity r < stride of one axis: (k0, n), the taps k0, k0 + stride, ... (n of them) of a kernel of size k that reach the
    rows y = stride * yy + r of the data gradient (y = stride * oy - pad + tap)"""
    out = []
    for r in range(stride):
        k0 = (r + pad) % stride
        out.append((k0, (k - k0 + stride - 1) // stride if k0 < k else 0))
    return out


def dgrad_weight(w, stride=1, pad=(0, 0)):
    """w [Co,Ci,kh,kw] -> the flat weight conv2d_dgrad reads (made once per layer: the network is frozen): for each output phase
    (ry, rx), ry-major, the block [Ci, Co, ny, nx] of the taps that reach it, flipped (te_hip.h, te_conv2d_dgrad_f32).  Stride 1 is the
    one block [Ci, Co*kh*kw].  Plain torch: runs on whatever device w is on."""
    blocks = []
    for k0y, ny in dgrad_phases(w.shape[2], stride, pad[0]):
        for k0x, nx in dgrad_phases(w.shape[3], stride, pad[1]):
            sub = w[:, :, k0y::stride, k0x::stride]
            assert tuple(sub.shape[2:]) == (ny, nx)
            blocks.append(sub.flip(2, 3).transpose(0, 1).reshape(-1))
    return torch.cat(blocks).contiguous()


@_op
def conv2d_dgrad(g, wt, x_shape, kernel, stride=1, pad=(0, 0), pre=None, slope=None, in_scale=None, add=None, add_stride=1):
    """the data gradient of conv2d / conv2d_prelu: g [B,Co,Ho,Wo], wt = dgrad_weight(w, stride, pad), x_shape = (B, Ci, H, W) of the
    forward's input, kernel = (kh, kw) -> gx [B,Ci,H,W].  pre [B,Ci,H,W] with slope [Ci]: gx = acc * PReLU'(pre).  Else
    gx = in_scale[ci] * acc + add[:, :, y / add_stride, x / add_stride] (where add_stride divides y and x), each term optional."""
    B, Ci, H, W = x_shape
    kh, kw = kernel
    if g.ndim != 4 or g.shape[0] != B or wt.ndim != 1 or (pre is not None and tuple(pre.shape) != (B, Ci, H, W)) \
            or any(t is not None and tuple(t.shape) != (Ci,) for t in (slope, in_scale)) \
            or tuple(g.shape[2:]) != conv2d_out_hw(H, W, kh, kw, stride, pad) \
            or wt.numel() != Ci * g.shape[1] * sum(a[1] for a in dgrad_phases(kh, stride, pad[0])) * sum(a[1] for a in dgrad_phases(kw, stride, pad[1])) \
            or (add is not None and tuple(add.shape) != (B, Ci, (H - 1) // max(add_stride, 1) + 1, (W - 1) // max(add_stride, 1) + 1)):
        raise RuntimeError(f'te_hip: conv2d_dgrad: inconsistent shapes g {tuple(g.shape)}, wt {tuple(wt.shape)}, x {tuple(x_shape)}, a {kh} x {kw} '
                           f'kernel, stride {stride}, pad {tuple(pad)}, pre {None if pre is None else tuple(pre.shape)}, add '
                           f'{None if add is None else tuple(add.shape)} read with stride {add_stride}')
    gx = torch.empty(B, Ci, H, W, device=g.device, dtype=g.dtype)
    _launch('te_conv2d_dgrad_f32', _ptr(gx), _ptr(g), _ptr(wt), _ptr(pre), _ptr(slope), _ptr(in_scale), _ptr(add), B, Ci, g.shape[1], H, W,
            kh, kw, stride, pad[0], pad[1], add_stride)
    return gx


@_op
def se_bwd(gout, r, gate, pooled, w1, w2):
    """the gradient of r in out = r * gate + shortcut with gate = se_excite(pooled, w1, w2), pooled = the plane means of r:
    gout, r [B,C,Ho,Wo], gate, pooled [B,C], w1 [R,C], w2 [C,R] -> gr [B,C,Ho,Wo]"""
    if gout.ndim != 4 or gout.shape != r.shape or tuple(gate.shape) != tuple(gout.shape[:2]) or gate.shape != pooled.shape or w1.ndim != 2 \
            or w1.shape[1] != gate.shape[1] or tuple(w2.shape) != (w1.shape[1], w1.shape[0]):
        raise RuntimeError(f'te_hip: se_bwd: inconsistent shapes gout {tuple(gout.shape)}, r {tuple(r.shape)}, gate {tuple(gate.shape)}, pooled '
                           f'{tuple(pooled.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}')
    B, Cn, Ho, Wo = gout.shape
    gr = torch.empty_like(gout)
    ws = torch.empty(2 * B * Cn, device=gout.device, dtype=gout.dtype)
    _launch('te_se_bwd_f32', _ptr(gr), _ptr(ws), _ptr(gout), _ptr(r), _ptr(gate), _ptr(pooled), _ptr(w1), _ptr(w2), B, Cn, w1.shape[0], Ho, Wo)
    return gr


@_op
def id_stem_bwd(g, wt, pre, slope, img_shape, box, pool):
    """the adjoint of id_stem_fwd: g, pre [N,Co,pool,pool], wt = dgrad_weight(the stem weight, 1, (1, 1)), slope [Co], img_shape = (N, 3, H, W)
    -> the image's gradient [N,3,H,W], exactly 0 outside the box"""
    N, _, H, W = img_shape
    if g.ndim != 4 or g.shape != pre.shape or g.shape[0] != N or tuple(g.shape[2:]) != (pool, pool) or slope.shape != (g.shape[1],) \
            or wt.shape != (27 * g.shape[1],) or img_shape[1] != 3:
        raise RuntimeError(f'te_hip: id_stem_bwd: inconsistent shapes g {tuple(g.shape)}, pre {tuple(pre.shape)}, wt {tuple(wt.shape)}, slope '
                           f'{tuple(slope.shape)}, image {tuple(img_shape)}, pool {pool}')
    y0, y1, x0, x1 = box
    gimg = torch.empty(N, 3, H, W, device=g.device, dtype=g.dtype)
    ws = torch.empty(N * 3 * pool * pool, device=g.device, dtype=g.dtype)
    _launch('te_id_stem_bwd_f32', _ptr(gimg), _ptr(ws), _ptr(g), _ptr(wt), _ptr(pre), _ptr(slope), N, H, W, y0, y1, x0, x1, pool, g.shape[1])
    return gimg


@_op
def rows_unit_bwd(ge, e, a):
    """l2_norm backwards: e = rows_unit(a), ge the gradient of e -> the gradient of a, (ge - e <e, ge>) / ||a||, per row of [I,D]"""
    if a.ndim != 2 or tuple(ge.shape) != tuple(a.shape) or tuple(e.shape) != tuple(a.shape):
        raise RuntimeError(f'te_hip: rows_unit_bwd expects three [I,D] tensors of one shape, got {tuple(ge.shape)}, {tuple(e.shape)}, {tuple(a.shape)}')
    ga = torch.empty_like(a)
    _launch('te_rows_unit_bwd_f32', _ptr(ga), _ptr(ge), _ptr(e), _ptr(a), a.shape[0], a.shape[1])
    return ga


# --------------------------------------------------------------------------------------------- M8b AlexNet LPIPS as a loss
@_op
def pool3s2_max_bwd(g, x):
    """MaxPool2d(3, 2) backwards (the adjoint of pool3 with POOL3_MAX_S2): x [B,C,H,W] the pool's input, g [B,C,Ho,Wo] -> gx [B,C,H,W],
    every element written; torch's tie rule (the first of equal maxima takes the gradient)"""
    if x.ndim != 4 or g.ndim != 4 or tuple(g.shape) != (x.shape[0], x.shape[1], max((x.shape[2] - 3) // 2 + 1, 0), max((x.shape[3] - 3) // 2 + 1, 0)):
        raise RuntimeError(f'te_hip: pool3s2_max_bwd: inconsistent shapes g {tuple(g.shape)}, x {tuple(x.shape)}')
    B, Cn, H, W = x.shape
    gx = torch.empty_like(x, memory_format=torch.contiguous_format)
    _launch('te_pool3s2_max_bwd_f32', _ptr(gx), _ptr(g), _ptr(x), B * Cn, H, W)
    return gx


ALEX_STEM_ROW_TAPS = tuple((2 + r) % 4 for r in range(4))          # k0 of the output rows y = 4 yy + r: (2, 3, 0, 1)


def alex_stem_dgrad_weight(w):
    """w [Co,3,11,11] -> the flat weight alex_stem_dgrad reads (made once: the network is frozen): for each row phase ry < 4 the block
    [Co, ny, 11, 3] of the kernel rows k0 + 4 jy that reach the rows y = 4 yy + ry (te_hip.h, te_alex_stem_dgrad_f32).  Plain torch:
    runs on whatever device w is on."""
    if w.ndim != 4 or tuple(w.shape[1:]) != (3, 11, 11):
        raise RuntimeError(f'te_hip: alex_stem_dgrad_weight expects [Co,3,11,11], got {tuple(w.shape)}')
    return torch.cat([w[:, :, k0::4, :].permute(0, 2, 3, 1).reshape(-1) for k0 in ALEX_STEM_ROW_TAPS]).contiguous()


@_op
def alex_stem_dgrad(g, wt, img_shape):
    """the adjoint of alex_stem_fwd without its ReLU: g [N,Co,Ho,Wo] (already masked), wt = alex_stem_dgrad_weight(w), img_shape =
    (N, 3, H, W) -> the UNSCALED image's gradient [N,3,H,W]"""
    N, _, H, W = img_shape
    if g.ndim != 4 or g.shape[0] != N or img_shape[1] != 3 or tuple(g.shape[2:]) != conv2d_out_hw(H, W, 11, 11, 4, (2, 2)) \
            or wt.shape != (363 * g.shape[1],):
        raise RuntimeError(f'te_hip: alex_stem_dgrad: inconsistent shapes g {tuple(g.shape)}, wt {tuple(wt.shape)}, image {tuple(img_shape)}')
    gimg = torch.empty(N, 3, H, W, device=g.device, dtype=g.dtype)
    _launch('te_alex_stem_dgrad_f32', _ptr(gimg), _ptr(g), _ptr(wt), N, H, W, g.shape[1])
    return gimg


# --------------------------------------------------------------------------------------------- M10 dual-space pSp encoder
def conv2d_heads_splits(Ci, kh, kw, Ho, Wo):
    """the number of k ranges te_conv2d_heads_f32 runs for this (Ci * kh * kw, Ho * Wo); 1 is the unsplit route (no batch or head count enters)"""
    S = lib().te_conv2d_heads_splits(Ci, kh, kw, Ho, Wo)
    if S < 0:
        raise RuntimeError(f'te_conv2d_heads_splits failed ({S}) for Ci={Ci}, a {kh} x {kw} kernel and a {Ho} x {Wo} plane')
    return S


@_op
def conv2d_heads(x, w, bias, stride=1, pad=(0, 0), shared=False, slope=0.01, out=None, c0=0, splits=0):
    """G convolutions of one shape in one launch, with bias and leaky ReLU: w [G,Cg,Ci,kh,kw], bias [G*Cg]; x [B,Ci,H,W] (shared: every head
    reads it) or [B,G*Ci,H,W] (head g reads its own Ci channels); written into channels [c0, c0 + G*Cg) of `out` [B,Ctot,Ho,Wo] (a new
    [B,G*Cg,Ho,Wo] tensor where out is None).  splits 0: the ABI's rule; n >= 1: n ranges of k (1 is the unsplit route).  The ABI refuses
    what te_conv2d_f32 refuses and a Cg that is no multiple of 64; nothing is launched then.  Returns out."""
    if x.ndim != 4 or w.ndim != 5 or bias.ndim != 1 or bias.shape[0] != w.shape[0] * w.shape[1] \
            or x.shape[1] != w.shape[2] * (1 if shared else w.shape[0]):
        raise RuntimeError(f'te_hip: conv2d_heads: inconsistent shapes x {tuple(x.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}, '
                           f'shared={bool(shared)}')
    (B, _, H, W), (G, Cg, Ci, kh, kw) = x.shape, w.shape
    Ho, Wo = conv2d_out_hw(H, W, kh, kw, stride, pad)
    out = _slice_out(out, c0, B, G * Cg, max(Ho, 0), max(Wo, 0), x, 'conv2d_heads')
    S = splits if splits else (conv2d_heads_splits(Ci, kh, kw, Ho, Wo) if Ho > 0 and Wo > 0 else 1)
    ws = torch.empty(S * B * G * Cg * Ho * Wo, device=x.device, dtype=x.dtype) if S > 1 else None
    _launch('te_conv2d_heads_f32', _ptr(out), _ptr(ws), 0 if ws is None else ws.numel() * 4, _ptr(x), _ptr(w), _ptr(bias), B, G, Ci, Cg, H, W,
            kh, kw, stride, pad[0], pad[1], out.shape[1], c0, 1 if shared else 0, float(slope), splits)
    return out


@_op
def upsample_add(x, y):
    """F.interpolate(x, size=y.shape[2:], mode='bilinear', align_corners=True) + y: x [B,C,h,w], y [B,C,H,W] -> a new [B,C,H,W] tensor"""
    if x.ndim != 4 or y.ndim != 4 or tuple(x.shape[:2]) != tuple(y.shape[:2]):
        raise RuntimeError(f'te_hip: upsample_add expects x [B,C,h,w] and y [B,C,H,W], got {tuple(x.shape)} and {tuple(y.shape)}')
    x, y = x.contiguous(), y.contiguous()
    (B, Cn, h, w), (H, W) = x.shape, y.shape[2:]
    out = torch.empty_like(y)
    _launch('te_upsample_add_f32', _ptr(out), _ptr(x), _ptr(y), B * Cn, h, w, H, W)
    return out


@_op
def psp_codes(lat, A, bz, Np, z_avg=None, p_avg=None):
    """the heads' latents lat [B,Ns+Np,D] (styles first) -> (z [B,D,T], p [B,D,Np]): z = adjust_style over the head axis (A [T,Ns], bz [T],
    scale folded in) + z_avg [D,T], p = the spatial latents + p_avg [D,Np]; either average may be None"""
    if lat.ndim != 3 or A.ndim != 2 or bz.shape != (A.shape[0],) or lat.shape[1] != A.shape[1] + Np \
            or z_avg is not None and tuple(z_avg.shape) != (lat.shape[2], A.shape[0]) \
            or p_avg is not None and tuple(p_avg.shape) != (lat.shape[2], Np):
        raise RuntimeError(f'te_hip: psp_codes: inconsistent shapes lat {tuple(lat.shape)}, A {tuple(A.shape)}, bz {tuple(bz.shape)}, Np {Np}, '
                           f'averages {[None if t is None else tuple(t.shape) for t in (z_avg, p_avg)]}')
    (B, _, D), (T, Ns) = lat.shape, A.shape
    z = torch.empty(B, D, T, device=lat.device, dtype=lat.dtype)
    p = torch.empty(B, D, Np, device=lat.device, dtype=lat.dtype)
    _launch('te_psp_codes_f32', _ptr(z), _ptr(p), _ptr(lat), _ptr(A), _ptr(bz), _ptr(z_avg), _ptr(p_avg), B, Ns, Np, D, T)
    return z, p


# --------------------------------------------------------------------------------------------- M10b training the encoder's heads
def heads_dgrad_weight(w, stride=1, pad=(0, 0)):
    """w [G,Cg,Ci,kh,kw] -> the flat weight conv2d_heads_dgrad reads: dgrad_weight's phases, each holding the heads' blocks [Ci,Cg,ny,nx]
    one behind the other.  Made once per step (the weights change); plain torch on whatever device w is on."""
    if w.ndim != 5:
        raise RuntimeError(f'te_hip: heads_dgrad_weight expects [G,Cg,Ci,kh,kw], got {tuple(w.shape)}')
    blocks = []
    for k0y, ny in dgrad_phases(w.shape[3], stride, pad[0]):
        for k0x, nx in dgrad_phases(w.shape[4], stride, pad[1]):
            blocks.append(w[:, :, :, k0y::stride, k0x::stride].flip(3, 4).transpose(1, 2).reshape(-1))
    return torch.cat(blocks).contiguous()


def _grad_slice(who, g, c0, Cn, B, Ho, Wo):
    """the check of a gradient read as the channel slice [c0, c0 + Cn) of g [B,Ctot,Ho,Wo]"""
    if g.ndim != 4 or g.shape[0] != B or tuple(g.shape[2:]) != (Ho, Wo) or c0 < 0 or c0 + Cn > g.shape[1]:
        raise RuntimeError(f'te_hip: {who}: g must be [{B},Ctot,{Ho},{Wo}] with channels [{c0}, {c0} + {Cn}) inside it, got {tuple(g.shape)}')


@_op
def conv2d_heads_dgrad(g, wt, x_shape, G, kernel, stride=1, pad=(0, 0), act=None, slope=0.01, c0=0):
    """the data gradient of conv2d_heads(shared=False): g the channels [c0, c0 + G*Cg) of [B,Ctot,Ho,Wo], wt = heads_dgrad_weight(w, stride,
    pad), x_shape = (B, G*Ci, H, W) of the forward's input, kernel = (kh, kw) -> gx [B,G*Ci,H,W], multiplied by the leaky ReLU' of the layer
    it enters where that layer's kept output act [B,G*Ci,H,W] is given (act > 0 ? 1 : slope).  The ABI refuses a Ci that is no multiple of
    64 and a slope that is not positive; nothing is launched then."""
    B, Cx, H, W = x_shape
    kh, kw = kernel
    taps = sum(a[1] for a in dgrad_phases(kh, stride, pad[0])) * sum(a[1] for a in dgrad_phases(kw, stride, pad[1]))
    if G < 1 or Cx % G or wt.ndim != 1 or wt.numel() % (Cx * max(taps, 1)) or (act is not None and tuple(act.shape) != (B, Cx, H, W)):
        raise RuntimeError(f'te_hip: conv2d_heads_dgrad: inconsistent shapes wt {tuple(wt.shape)}, x {tuple(x_shape)}, {G} heads, a {kh} x {kw} '
                           f'kernel, stride {stride}, pad {tuple(pad)}, act {None if act is None else tuple(act.shape)}')
    Cg = wt.numel() // (Cx * taps)
    _grad_slice('conv2d_heads_dgrad', g, c0, G * Cg, B, *conv2d_out_hw(H, W, kh, kw, stride, pad))
    gx = torch.empty(B, Cx, H, W, device=g.device, dtype=g.dtype)
    _launch('te_conv2d_heads_dgrad_f32', _ptr(gx), _ptr(g), _ptr(wt), _ptr(act), B, G, Cx // G, Cg, H, W, kh, kw, stride, pad[0], pad[1],
            g.shape[1], c0, float(slope))
    return gx


def conv2d_heads_wgrad_splits(Cg, Ci, kh, kw, B, Ho, Wo):
    """the number of ranges of r = (b, oy, ox) te_conv2d_heads_wgrad_f32 runs for (M = Cg, N = Ci * kh * kw, R = B * Ho * Wo); 1 is the
    unsplit route (no head count enters)"""
    S = lib().te_conv2d_heads_wgrad_splits(Cg, Ci, kh, kw, B, Ho, Wo)
    if S < 0:
        raise RuntimeError(f'te_conv2d_heads_wgrad_splits failed ({S}) for Cg={Cg}, Ci={Ci}, a {kh} x {kw} kernel, B={B} and a {Ho} x {Wo} plane')
    return S


@_op
def conv2d_heads_wgrad(g, x, w_shape, stride=1, pad=(0, 0), shared=False, c0=0, splits=0):
    """the weight and bias gradient of conv2d_heads (and, with G = 1, of conv2d): g the channels [c0, c0 + G*Cg) of [B,Ctot,Ho,Wo], already
    multiplied by the activation's derivative; x the forward's input, [B,Ci,H,W] (shared) or [B,G*Ci,H,W]; w_shape = (G, Cg, Ci, kh, kw)
    -> (gw [G,Cg,Ci,kh,kw], gb [G*Cg]).  splits 0: the ABI's rule; n >= 1: n ranges of the reduction (1 is the unsplit route)."""
    if len(w_shape) != 5 or x.ndim != 4 or x.shape[1] != w_shape[2] * (1 if shared else w_shape[0]):
        raise RuntimeError(f'te_hip: conv2d_heads_wgrad: inconsistent shapes x {tuple(x.shape)}, w {tuple(w_shape)}, shared={bool(shared)}')
    (B, _, H, W), (G, Cg, Ci, kh, kw) = x.shape, w_shape
    Ho, Wo = conv2d_out_hw(H, W, kh, kw, stride, pad)
    _grad_slice('conv2d_heads_wgrad', g, c0, G * Cg, B, Ho, Wo)
    gw = torch.empty(G, Cg, Ci, kh, kw, device=g.device, dtype=g.dtype)
    gb = torch.empty(G * Cg, device=g.device, dtype=g.dtype)
    S = splits if splits else (conv2d_heads_wgrad_splits(Cg, Ci, kh, kw, B, Ho, Wo) if Ho > 0 and Wo > 0 and Cg % 64 == 0 else 1)
    ws = torch.empty(S * gw.numel(), device=g.device, dtype=g.dtype) if S > 1 else None
    _launch('te_conv2d_heads_wgrad_f32', _ptr(gw), _ptr(gb), _ptr(ws), 0 if ws is None else ws.numel() * 4, _ptr(g), _ptr(x), B, G, Ci, Cg, H, W,
            kh, kw, stride, pad[0], pad[1], g.shape[1], c0, 1 if shared else 0, splits)
    return gw, gb


@_op
def upsample_add_bwd(g, x_shape, add=None):
    """the adjoint of upsample_add with respect to x: g [B,C,H,W], x_shape = (B, C, h, w) -> gx [B,C,h,w] (+ add [B,C,h,w] where given);
    the gradient of y is g itself"""
    if g.ndim != 4 or len(x_shape) != 4 or tuple(g.shape[:2]) != tuple(x_shape[:2]) or (add is not None and tuple(add.shape) != tuple(x_shape)):
        raise RuntimeError(f'te_hip: upsample_add_bwd expects g [B,C,H,W] and x_shape (B, C, h, w), got {tuple(g.shape)}, {tuple(x_shape)} and add '
                           f'{None if add is None else tuple(add.shape)}')
    B, Cn, h, w = x_shape
    gx = torch.empty(B, Cn, h, w, device=g.device, dtype=g.dtype)
    _launch('te_upsample_add_bwd_f32', _ptr(gx), _ptr(g), _ptr(add), B * Cn, h, w, g.shape[2], g.shape[3])
    return gx


@_op
def psp_codes_bwd(gz, gp, lat, A):
    """the adjoint of psp_codes: gz [B,D,T], gp [B,D,Np], lat [B,Ns+Np,D], A [T,Ns] (folded) -> (glat [B,Ns+Np,D], gA [T,Ns] for the FOLDED
    A, gbz [T])"""
    if gz.ndim != 3 or gp.ndim != 3 or lat.ndim != 3 or A.ndim != 2 or gz.shape[2] != A.shape[0] or tuple(gz.shape[:2]) != tuple(gp.shape[:2]) \
            or tuple(lat.shape) != (gz.shape[0], A.shape[1] + gp.shape[2], gz.shape[1]):
        raise RuntimeError(f'te_hip: psp_codes_bwd: inconsistent shapes gz {tuple(gz.shape)}, gp {tuple(gp.shape)}, lat {tuple(lat.shape)}, '
                           f'A {tuple(A.shape)}')
    (B, D, T), Np, Ns = gz.shape, gp.shape[2], A.shape[1]
    glat = torch.empty_like(lat, memory_format=torch.contiguous_format)
    gA = torch.empty(T, Ns, device=gz.device, dtype=gz.dtype)
    gbz = torch.empty(T, device=gz.device, dtype=gz.dtype)
    _launch('te_psp_codes_bwd_f32', _ptr(glat), _ptr(gA), _ptr(gbz), _ptr(gz), _ptr(gp), _ptr(lat), _ptr(A), B, Ns, Np, D, T)
    return glat, gA, gbz


# --------------------------------------------------------------------------------------------- roctx ranges (SURVEY §5 tracing)
# TE_ROCTX=1: every wrapper marked @_op above runs inside a roctx range "te:<op> <shape of its first tensor>", so a
# `rocprofv3 --kernel-trace --marker-trace` timeline attributes kernels to operators instead of showing template names only
# (torch.cuda.nvtx is backed by roctx on ROCm builds).  Off by default: two extra calls per launch.
def _install_roctx():
    import functools
    import torch.cuda.nvtx as nvtx

    def wrap(fn):
        name = fn.__name__

        @functools.wraps(fn)
        def run(*a, **k):
            t = next((x for x in a if torch.is_tensor(x)), None)
            nvtx.range_push(f'te:{name} {tuple(t.shape)}' if t is not None else f'te:{name}')
            try:
                return fn(*a, **k)
            finally:
                nvtx.range_pop()
        return run
    for i, fn in enumerate(_OPS):           # the registry then holds what the module exposes
        _OPS[i] = globals()[fn.__name__] = wrap(fn)


ROCTX = os.environ.get('TE_ROCTX') == '1'
if ROCTX:
    _install_roctx()

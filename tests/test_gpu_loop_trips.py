"""The kernels that loop inside a block - the FIR plane walks and the capped grids of tests/loop_trips.py - past their first trip,
against fp64 references built from stock torch ops on the GPU.  Each test re-asserts its entry's trips through the library's
queries before it compares numbers, so a changed launch constant cannot silently move a case back to one trip.

Bounds are elementwise and come from the arithmetic, u = unit round-off of the kernel's number format (2^-24 fp32, 2^-11 fp16
stores, 2^-53 fp64):
* a FIR output of T taps with bias b and leaky-ReLU gain g: (T + 2) u (|k| * |x| + |b|) g + u |y|.  (T products and T - 1 adds
  give at most T u (|k| * |x|), the bias add u (|k| * |x| + |b|); the slope and the gain are one rounding each, 2 u |y|, of which one
  is folded into the first term because |y| <= g (|k| * |x| + |b|).)  The activation-gradient prologue adds one rounding to
  every staged value (inside T + 2), the epilogue form one to the output (the u |y|).
* a sum of L terms (bias gradients, scale gradients, weight gradients): (L + 1) u sum |terms| - L - 1 additions in any order and
  one rounding per term.  Where the terms are FIR outputs (the epilogue form's bias gradient) their own bounds are added.
* elementwise kernels: one rounding per operation, (1 + u)^n - 1 relative; fp16 adds the store's 2^-11 |y| and half a subnormal
  step, 2^-25.  The fp64 kernels are compared with a reference of their own precision, so its round-off counts too: twice the bound.
* the convolution cases: the bars of tests/test_gpu_conv_routes.py.
Elements whose fp64 pre-activation lies within the bound of 0 are left out of a leaky-ReLU comparison (the slope may differ there);
at most 0.1 % of a case (tests/fp64_check.py: KINK_CAP).  For the forward and dx cases of the plane walks a plane's bits must not depend on the launch: the first
zgroups planes and the last plane of the big launch equal launches that hold only those planes.

`max err / bound` and the left-out share per case are printed at the end of the module.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_routes as cr
import fp64_check
import loop_trips as lt
from conftest import rel_err
from fir_restated import fir64, fir_bound as _fir_bound, slope64
from fp64_check import A32, ALPHA, S32, SCALE, U, U32, where64
from transeditor_amd import _lib
from transeditor_amd.op.chanscale import chan_scale
from transeditor_amd.op.fir_act import blur_bias_act
from transeditor_amd.op.linear import linear_fused
from transeditor_amd.op.upfirdn2d import upfirdn2d

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CONV_TOL = 1e-5                                                          # tests/test_gpu_conv_routes.py: FWD_TOL
RESULTS = []
IDS = lambda e: e.name
_report = fp64_check.report_fixture('max err / bound per case (tests/test_gpu_loop_trips.py):', RESULTS)


def _randn(shape, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV, dtype=torch.float32).to(dtype)


def _within(entry, what, got, ref, bound, keep=None):
    """the elementwise check of tests/fp64_check.py, recorded for this module's report"""
    fp64_check.within(entry.name, what, got, ref, bound, keep, results=RESULTS)


def _rel(entry, what, got, ref, bar):
    e = rel_err(got, ref)
    RESULTS.append((entry.name, what, e / bar, 0.0))
    print(f'{entry.name} {what}: rel err {e:.2e} (bar {bar:.0e})')
    assert e <= bar, f'{entry.name} {what}: rel err {e:.3e} > {bar:.1e}'


# ------------------------------------------------------------------------------------------------ references
def taps2d(taps, dtype=torch.float32, gain=1.0):
    k = torch.tensor(taps, dtype=torch.float64)
    k = torch.outer(k, k)
    return (k / k.sum() * gain).to(dtype).to(DEV)          # (1,3,3,1) / 64 and (1,2,1) / 16 are exact in every format here


def _pad4(p):
    return (p[0], p[1], p[0], p[1])


def _planes(t, lo, hi):
    """planes lo .. hi of a [B, C, H, W] tensor as a [1, hi - lo, H, W] tensor of its own"""
    return t.reshape(1, -1, *t.shape[2:])[:, lo:hi].clone()


# ------------------------------------------------------------------------------------------------ FIR plane walks
FWD_ACT = [e for e in lt.PLANE_WALKS if e.op == 'blur_bias_act']
PLAIN = [e for e in lt.PLANE_WALKS if e.op == 'upfirdn2d']
ACTGRAD = [e for e in lt.PLANE_WALKS if e.op == 'blur_actgrad']
GRADACT = [e for e in lt.PLANE_WALKS if e.op == 'blur_gradact']


@pytest.mark.parametrize('entry', FWD_ACT, ids=IDS)
def test_blur_bias_act_forward(entry):
    """blur44 MODE 0 with the bias of a later plane (mj % size_b) and the leaky ReLU riding on trips 2 and 3"""
    lt.check(entry)
    planes, zgroups, _ = lt.fir_plan(entry)
    B, Cn, H, W = entry.shape
    pad = entry.args['pad']
    x, b, k = _randn(entry.shape, 1), _randn((Cn,), 2), taps2d(lt.BLUR)
    with torch.no_grad():
        y = blur_bias_act(x, k, b, pad)
        x64, k64, b64 = x.double(), k.double(), b.double()[None, :, None, None]
        pre = fir64(x64, k64, pad=_pad4(pad)) + b64
        gain = where64(pre > 0, S32, A32 * S32)
        y64 = pre * gain
        mag = fir64(x64.abs(), k64, pad=_pad4(pad)) + b64.abs()
        keep = pre.abs() > (16 + 2) * U32 * mag                      # off the kink by more than the pre-activation's own bound
        _within(entry, 'y', y, y64, _fir_bound(mag, y64, 16, gain), keep)
        # a plane's bits do not depend on the launch (bias per plane of the sub-launch = b[plane % C])
        bp = b.repeat(-(-planes // Cn))[:planes]
        first = blur_bias_act(_planes(x, 0, zgroups), k, bp[:zgroups].clone(), pad)
        assert torch.equal(_planes(y, 0, zgroups), first)
        last = blur_bias_act(_planes(x, planes - 1, planes), k, bp[planes - 1:].clone(), pad)
        assert torch.equal(_planes(y, planes - 1, planes), last)


@pytest.mark.parametrize('entry', PLAIN, ids=IDS)
def test_upfirdn2d_both_directions(entry):
    """plain upfirdn2d through the plane-walking kernels and its adjoint (the same op with up / down swapped, at the same plane count)"""
    lt.check(entry)
    planes, zgroups, _ = lt.fir_plan(entry)
    a = entry.args
    up, down, pad = a['up'], a['down'], a['pad']
    k = taps2d(lt.BLUR, gain=up * up)
    x = _randn(entry.shape, 3).requires_grad_(True)
    y = upfirdn2d(x, k, up=up, down=down, pad=pad)
    g = _randn(tuple(y.shape), 4)
    gx, = torch.autograd.grad(y, x, g)
    x64, k64 = x.detach().double().requires_grad_(True), k.double()
    y64 = fir64(x64, k64, up, down, _pad4(pad))
    gx64, = torch.autograd.grad(y64, x64, g.double())
    ax = x.detach().double().abs().requires_grad_(True)
    mag = fir64(ax, k64, up, down, _pad4(pad))
    gmag, = torch.autograd.grad(mag, ax, g.double().abs())           # |k| (adjoint) |g|
    T, Tadj = 16 // (up * up), 16 // (down * down)                   # taps that meet a sample (zero insertion skips the others)
    with torch.no_grad():
        _within(entry, 'y', y.detach(), y64.detach(), _fir_bound(mag.detach(), y64.detach(), T))
        _within(entry, 'dx', gx, gx64, _fir_bound(gmag, gx64, Tadj))
        xd = x.detach()
        for lo, hi in ((0, zgroups), (planes - 1, planes)):
            assert torch.equal(_planes(y.detach(), lo, hi), upfirdn2d(_planes(xd, lo, hi), k, up=up, down=down, pad=pad))
        # the adjoint launch has its own plane groups
        gz = lt._plan(_lib.lib().te_upfirdn2d_plan, planes, y.shape[2], y.shape[3], 1, 4, 4, down, down, up, up,
                      *_adjoint_pads(entry, y.shape[2:]))[0]
        assert 0 < gz < planes
        for lo, hi in ((0, gz), (planes - 1, planes)):
            xs = _planes(xd, lo, hi).requires_grad_(True)
            with torch.enable_grad():
                ys = upfirdn2d(xs, k, up=up, down=down, pad=pad)
                gs, = torch.autograd.grad(ys, xs, _planes(g, lo, hi))
            assert torch.equal(_planes(gx, lo, hi), gs)


def _adjoint_pads(entry, out_hw):
    from transeditor_amd.op.upfirdn2d import _geometry
    a = entry.args
    _, g_pad = _geometry(entry.shape[2:], (4, 4), (a['up'],) * 2, (a['down'],) * 2, _pad4(a['pad']))
    return g_pad


def _actgrad_ref(entry, g, ref, k):
    """fp64 staged values s = g * slope(ref), their FIR and |k| * |s|"""
    s = g.double() * slope64(ref)
    gp = entry.args['gpad']
    return s, fir64(s, k.double(), pad=gp), fir64(s.abs(), k.double(), pad=gp)


@pytest.mark.parametrize('entry', ACTGRAD, ids=IDS)
def test_blur_actgrad(entry):
    """te_blur_actgrad_f32 (blur44 MODE 1; fir_tile_kernel<1,1,4,4,AG> for rows of 3): dx and the bias gradient from
    partial[mj * tiles + tile] of later planes"""
    lt.check(entry)
    planes, zgroups, _ = lt.fir_plan(entry)
    B, Cn, H, W = entry.shape
    gp = entry.args['gpad']
    g, ref, k = _randn(entry.shape, 5), _randn(entry.shape, 6), taps2d(lt.BLUR)
    with torch.no_grad():
        gx, gb = _lib.blur_actgrad(g, ref, k, gp, ALPHA, SCALE)
        s, gx64, mag = _actgrad_ref(entry, g, ref, k)
        _within(entry, 'dx', gx, gx64, _fir_bound(mag, gx64, 16))
        L = B * H * W
        _within(entry, 'dbias', gb, s.sum(dim=(0, 2, 3)), (L + 1) * U32 * s.abs().sum(dim=(0, 2, 3)))
        for lo, hi in ((0, zgroups), (planes - 1, planes)):
            sub, _ = _lib.blur_actgrad(_planes(g, lo, hi), _planes(ref, lo, hi), k, gp, ALPHA, SCALE)
            assert torch.equal(_planes(gx, lo, hi), sub)


@pytest.mark.parametrize('entry', GRADACT, ids=IDS)
def test_blur_gradact(entry):
    """te_blur_gradact_f32 (blur44 MODE 2): dx and the bias gradient"""
    lt.check(entry)
    planes, zgroups, _ = lt.fir_plan(entry)
    B, Cn, H, W = entry.shape
    gp = entry.args['gpad']
    oh, ow = lt.fir_out_hw(entry)
    g, ref, k = _randn(entry.shape, 7), _randn((B, Cn, oh, ow), 8), taps2d(lt.BLUR)
    with torch.no_grad():
        gx, gb = _lib.blur_gradact(g, ref, k, gp, ALPHA, SCALE)
        c = slope64(ref)
        gx64 = fir64(g.double(), k.double(), pad=gp) * c
        mag = fir64(g.double().abs(), k.double(), pad=gp)
        bound = _fir_bound(mag, gx64, 16, c)
        _within(entry, 'dx', gx, gx64, bound)
        L = B * oh * ow
        _within(entry, 'dbias', gb, gx64.sum(dim=(0, 2, 3)), (L + 1) * U32 * gx64.abs().sum(dim=(0, 2, 3)) + bound.sum(dim=(0, 2, 3)))
        for lo, hi in ((0, zgroups), (planes - 1, planes)):
            sub, _ = _lib.blur_gradact(_planes(g, lo, hi), _planes(ref, lo, hi), k, gp, ALPHA, SCALE)
            assert torch.equal(_planes(gx, lo, hi), sub)


# ------------------------------------------------------------------------------------------------ capped grids
def _dtype(entry):
    return getattr(torch, entry.args['dtype'])


@pytest.mark.parametrize('entry', [e for e in lt.CAPPED if e.op == 'fir_direct'], ids=IDS)
def test_fir_direct(entry):
    lt.check(entry)
    dt = _dtype(entry)
    x, k = _randn(entry.shape, 9, dt), taps2d(entry.args['taps'], dt)
    pad = _pad4(entry.args['pad'])
    with torch.no_grad():
        y = _lib.upfirdn2d_raw(x, k, (1, 1), (1, 1), pad)
        y64 = fir64(x.double(), k.double(), pad=pad)
        mag = fir64(x.double().abs(), k.double(), pad=pad)
        acc = U32 if dt == torch.float16 else U[dt]                  # half accumulates in fp32 and rounds once at the store
        bound = (k.numel() + 2) * acc * mag + U[dt] * y64.abs() + (2.0 ** -25 if dt == torch.float16 else 0.0)
        if dt == torch.float64:
            bound = 2 * bound                                        # the fp64 reference has the same round-off as the kernel
        _within(entry, 'y', y, y64, bound)


@pytest.mark.parametrize('entry', [e for e in lt.CAPPED if e.op == 'chan_scale'], ids=IDS)
def test_chan_scale_and_adjoints(entry):
    lt.check(entry)
    B, Cn, H, W = entry.shape
    x = _randn(entry.shape, 10).requires_grad_(True)
    s = (1 + 0.3 * _randn((B, Cn), 11)).requires_grad_(True)
    assert x.data_ptr() % 16 == 0
    y = chan_scale(x, s)
    g = _randn(entry.shape, 12)
    gx, gs = torch.autograd.grad(y, (x, s), g)                       # chan_scale again, and te_chan_dot_f32
    with torch.no_grad():
        x64, s64, g64 = x.double(), s.double()[:, :, None, None], g.double()
        _within(entry, 'y', y, x64 * s64, U32 * (x64 * s64).abs())
        _within(entry, 'dx', gx, g64 * s64, U32 * (g64 * s64).abs())
        _within(entry, 'ds', gs, (g64 * x64).sum(dim=(2, 3)), (H * W + 1) * U32 * (g64 * x64).abs().sum(dim=(2, 3)))


BIAS_ACT = [(e, m) for e in lt.CAPPED if e.op == 'bias_act' for m in ('forward', 'grad', 'gradgrad', 'grad2')]


@pytest.mark.parametrize('entry,mode', BIAS_ACT, ids=lambda v: v if isinstance(v, str) else v.name)
def test_bias_act_elementwise(entry, mode):
    """forward act(x + b) * scale; 'grad' = the slope mask of a saved output on g; 'gradgrad' = the same mask on ggi + ggb[c] (what
    the op's double backward runs); 'grad2' = the second derivative, identically zero"""
    lt.check(entry)
    dt = _dtype(entry)
    x = _randn(entry.shape, 13, dt)
    b = _randn((entry.shape[1],), 14, dt) if mode in ('forward', 'gradgrad') else None
    ref = None if mode == 'forward' else _randn(entry.shape, 15, dt)
    grad = {'forward': 0, 'grad': 1, 'gradgrad': 1, 'grad2': 2}[mode]
    with torch.no_grad():
        y = _lib.bias_act(x, b, ref, 3, grad, ALPHA, SCALE)
        if mode == 'grad2':
            assert torch.equal(y, torch.zeros_like(y))
            return
        # the float arguments become scalar_t (fp16: through a half), the arithmetic is fp32 for half and T for the other two
        al, sc = (float(torch.tensor(v, dtype=torch.float32).to(dt)) for v in (ALPHA, SCALE))
        v64 = x.double() + (b.double()[None, :, None, None] if b is not None else 0.0)
        mask = (v64 if mode == 'forward' else ref.double()) > 0      # (a correctly rounded sum keeps the sign of the exact one: no kink)
        y64 = torch.where(mask, v64, v64 * al) * sc
        acc = U32 if dt == torch.float16 else U[dt]
        bound = ((1 + acc) ** 3 - 1) * y64.abs()                     # add, slope, gain
        if dt == torch.float16:
            bound = bound + U[dt] * y64.abs() + 2.0 ** -25
        if dt == torch.float64:
            bound = 2 * bound                                        # the fp64 reference has the same round-off as the kernel
        _within(entry, mode, y, y64, bound)


def _conv_case(entry, seed):
    B, K, M, H, W = entry.shape
    ws = 0.7
    x = _randn((B, K, H, W), seed).requires_grad_(True)
    w = _randn((M, K, 3, 3), seed + 1) / math.sqrt(K * 9)
    gy = _randn((B, M, H, W), seed + 2)
    sw = {k: v for k, v in entry.args.items() if k in cr.DEFAULT_SWITCHES}
    with cr.switches(**sw) as mc:
        y = mc.conv_core(x, w, '3x3', ws)
        gx, = torch.autograd.grad(y, x, gy)
    x64 = x.detach().double().requires_grad_(True)
    y64 = F.conv2d(x64, w.double() * ws, padding=1)
    gx64, = torch.autograd.grad(y64, x64, gy.double())
    _rel(entry, 'y', y, y64, CONV_TOL)
    _rel(entry, 'dx', gx, gx64, CONV_TOL)


def test_conv_finalize_past_its_cap():
    """the split-K epilogue strides over 655 360 outputs, forward and data gradient"""
    entry = lt.BY_NAME['conv_finalize']
    lt.check(entry)
    _conv_case(entry, 20)


@pytest.mark.parametrize('entry', [e for e in lt.CAPPED if e.op == 'pack'], ids=IDS)
def test_pack_tile_walk_through_the_convolution(entry):
    """288 tiles of 32 x 32 on 256 blocks: the packed layouts are checked through the convolution that reads them"""
    lt.check(entry)
    _conv_case(entry, 30)


def test_splitk_finish_past_its_cap():
    """the weight gradient [512, 520] of a linear layer over 2055 rows: split-K over 2048 rows (the finishing kernel strides), the
    last 7 rows through the single-pass kernel with the first part as its residual"""
    entry = lt.BY_NAME['splitk_finish']
    lt.check(entry)
    R, K, N = entry.shape
    x, gy = _randn((R, K), 40), _randn((R, N), 41)
    w = (_randn((N, K), 42) / math.sqrt(K)).requires_grad_(True)
    y = linear_fused(x, w)
    gw, = torch.autograd.grad(y, w, gy)
    with torch.no_grad():
        _within(entry, 'dW', gw, gy.double().t() @ x.double(), (R + 1) * U32 * (gy.double().abs().t() @ x.double().abs()))

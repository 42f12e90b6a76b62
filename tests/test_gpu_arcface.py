"""The ArcFace IR-SE50 identity network (transeditor_amd.arcface, csrc/irse.hip on the main loop of csrc/conv2d_body.h) against
te_conv2d_f32, fp64 torch and the plain-torch restatement (tests/arcface_restated.py): the convolution with a batch norm in front of its
zero padding and PReLU behind it, the stem with the crop and the adaptive average in its gather, squeeze-and-excitation, the gated
residual sum, the row kernels, the whole network on small geometries and on the true one (IR-SE50 at 256 px, against what the
reference's own Backbone returns: tests/golden/arcface_ref.npz), and the plumbing around it (feature_sweeps, the input checks)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import arcface_restated as R
from conftest import load_golden, rel_l2
from fp64_check import SENTINEL, U32 as EPS, within

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ------------------------------------------------------------------------------------------- 1. batch norm -> padded convolution -> PReLU
# (B, Ci, Co, H, W, k, s, pad)
PRELU_CASES = [(3, 8, 72, 7, 7, 3, 1, 1),               # a ragged channel block (72 = 64 + 8), 147 pixels: a tile that spans images
               (2, 3, 64, 9, 11, 3, 1, 1),              # K = 27: the unaligned weight path
               (2, 16, 40, 9, 9, 3, 2, 1),              # stride 2
               (1, 4, 64, 256, 256, 3, 1, 1)]           # 512 workgroups of 128 pixels: the wide tile (kWideGridMin)
_IDS = dict(ids=lambda c: 'x'.join(map(str, c)))


def _prelu_case(case, shift=0.3):
    """x, w ~ N(0, 1), bias ~ N(0, 1), slopes 0.25 + 0.3 N(0, 1) (a fifth negative), in_scale uniform in [0.5, 1.5] with every third
    one negated, in_shift ~ shift * N(0, 1)"""
    B, Ci, Co, H, W, k, s, pad = case
    g = torch.Generator().manual_seed(sum(p * v for p, v in zip((3, 5, 7, 11, 13, 17, 19, 23), case)))
    x, w = torch.randn(B, Ci, H, W, generator=g), torch.randn(Co, Ci, k, k, generator=g)
    b, slope = torch.randn(Co, generator=g), 0.25 + 0.3 * torch.randn(Co, generator=g)
    a = (torch.rand(Ci, generator=g) + 0.5) * torch.where(torch.arange(Ci) % 3 == 2, -1.0, 1.0)
    return dict(x=x, w=w, b=b, slope=slope, a=a, t=shift * torch.randn(Ci, generator=g))


def _prelu_ref(d, case, dtype, affine=True):
    """the contract restated: the affine INSIDE the image, zeros around it, convolution, bias, PReLU -> (out, the bound's magnitude)"""
    *_, k, s, pad = case
    x, w, b, slope, a, t = (d[n].to(dtype) for n in ('x', 'w', 'b', 'slope', 'a', 't'))
    v = x * a.view(1, -1, 1, 1) + t.view(1, -1, 1, 1) if affine else x
    out = F.prelu(F.conv2d(F.pad(v, (pad,) * 4), w, b, s), slope)
    mag = F.conv2d(F.pad(x.abs() * a.abs().view(1, -1, 1, 1) + t.abs().view(1, -1, 1, 1), (pad,) * 4), w.abs(), b.abs(), s)
    return out, mag


@pytest.fixture(scope='module')
def prelu_refs():
    """per case: the inputs, the fp64 result with the affine, the elementwise bound and torch's own fp32 on the CPU.  Computed once,
    shared and never modified.  Bound: max(1, |slope_m|) (K + 5) 2^-24 (|w| * (|a||x| + |b|) + |bias|) + 2^-24 |out64|: K products and
    K additions of the fma chain, the gather's fma, the bias, a spare, scaled by the slope; then the slope product's own rounding."""
    out = {}
    for case in PRELU_CASES:
        B, Ci, Co, H, W, k, s, pad = case
        d = _prelu_case(case)
        K = Ci * k * k
        o64, mag = _prelu_ref(d, case, torch.float64)
        bound = d['slope'].double().abs().clamp(min=1).view(1, -1, 1, 1) * (K + 5) * EPS * mag + EPS * o64.abs()
        out[case] = dict(d, o64=o64, bound=bound, cpu32=_prelu_ref(d, case, torch.float32)[0], K=K)
    return out


def _run_prelu(d, case, affine=True, **over):
    from transeditor_amd import _lib
    *_, k, s, pad = case
    t = {n: over.get(n, d[n]).to(DEV) for n in ('x', 'w', 'b', 'slope', 'a', 't')}
    return _lib.conv2d_prelu(t['x'], t['w'], t['b'], t['slope'], t['a'] if affine else None, t['t'] if affine else None, s, (pad, pad))


@pytest.mark.parametrize('case', PRELU_CASES, **_IDS)
def test_conv2d_prelu_without_the_affine_is_conv2d(prelu_refs, case):
    """the accumulators are te_conv2d_f32's: bitwise prelu(te_conv2d_f32(act = 0)), torch doing the PReLU"""
    from transeditor_amd import _lib
    *_, k, s, pad = case
    d = prelu_refs[case]
    out = _run_prelu(d, case, affine=False)
    plain = _lib.conv2d(d['x'].to(DEV), d['w'].to(DEV), d['b'].to(DEV), s, (pad, pad), act=0)
    assert out.shape == d['o64'].shape and out.dtype == torch.float32 and out.is_contiguous()
    assert torch.equal(out, F.prelu(plain, d['slope'].to(DEV)))
    assert 0.2 < float((plain < 0).float().mean()) < 0.8                        # both branches are live


@pytest.mark.parametrize('case', PRELU_CASES, **_IDS)
def test_conv2d_prelu_with_the_affine_against_fp64(prelu_refs, case):
    """elementwise, no element left out (PReLU is Lipschitz: nothing near 0 needs excusing); torch's own fp32 on the CPU meets the
    same bound"""
    d = prelu_refs[case]
    within(f'conv2d_prelu {case}', f'K={d["K"]}', _run_prelu(d, case), d['o64'], d['bound'], yardstick=(d['cpu32'], 0.0))


def test_conv2d_prelu_shift_is_not_a_bias():
    """With in_shift of order 10 the result agrees with fp64 everywhere, and at the border it is NOT what folding the shift into the
    bias gives (bias'[m] = bias[m] + sum_{c,ky,kx} w[m,c,ky,kx] shift[c]): the padded taps do not carry the shift.  A border element
    misses 3 or 5 of its 9 taps, i.e. 24 or 40 terms w * shift of size 10: a difference of some tens (a quarter of that where the
    slope applies), against 1000 x the bound of about 3.  Asserted: at EVERY border pixel some channel differs by more than
    1000 x the bound, more than half of all border elements do, and no interior element differs at all beyond the bound."""
    case = PRELU_CASES[0]
    B, Ci, Co, H, W, k, s, pad = case
    d = _prelu_case(case, shift=10.0)
    o64, mag = _prelu_ref(d, case, torch.float64)
    bound = d['slope'].double().abs().clamp(min=1).view(1, -1, 1, 1) * (Ci * k * k + 5) * EPS * mag + EPS * o64.abs()
    out = _run_prelu(d, case).double().cpu()
    within(f'conv2d_prelu {case} shift 10', 'y', out, o64, bound)
    w64, a64 = d['w'].double(), d['a'].double()
    folded_bias = d['b'].double() + (w64 * d['t'].double().view(1, -1, 1, 1)).sum((1, 2, 3))
    folded = F.prelu(F.conv2d(d['x'].double() * a64.view(1, -1, 1, 1), w64, folded_bias, s, pad), d['slope'].double())
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    diff = (out - folded).abs() / bound
    print(f'shift folded into the bias: border diff / bound min-over-pixels of max-over-channels {float(diff[:, :, border].amax(1).min()):.0f}, '
          f'share of border elements above 1000: {float((diff[:, :, border] > 1000).double().mean()):.3f}; interior max {float(diff[:, :, ~border].max()):.3f}')
    assert bool((diff[:, :, border].amax(1) > 1000).all())
    assert float((diff[:, :, border] > 1000).double().mean()) > 0.5
    assert bool((diff[:, :, ~border] <= 2).all())                               # (each of the two within its bound of fp64)


@pytest.mark.parametrize('affine', [False, True])
def test_conv2d_prelu_nan_and_batch(prelu_refs, affine):
    case = PRELU_CASES[0]
    B, Ci, Co, H, W, *_ = case
    d = prelu_refs[case]
    full = _run_prelu(d, case, affine)
    # the first image of a batch equals a batch of one (its 49 pixels share a tile with the second image's); two runs agree
    assert torch.equal(full[:1], _run_prelu(d, case, affine, x=d['x'][:1].contiguous()))
    assert torch.equal(full, _run_prelu(d, case, affine))
    # a NaN pixel reaches exactly the outputs whose 3 x 3 window holds it, on every channel (no weight is exactly 0)
    bad = d['x'].clone()
    bad[1, 5, 0, 3] = float('nan')
    got = _run_prelu(d, case, affine, x=bad)
    hit = torch.zeros_like(got, dtype=torch.bool)
    hit[1, :, 0:2, 2:5] = True
    assert torch.equal(got.isnan(), hit) and torch.equal(got[~hit], full[~hit])


def test_conv2d_prelu_refusals():
    from transeditor_amd import _lib
    L = _lib.lib()
    x, w, b = torch.zeros(2, 3, 9, 9, device=DEV), torch.zeros(4, 3 * 8 * 8, device=DEV), torch.zeros(4, device=DEV)
    sl, a, t = torch.zeros(4, device=DEV), torch.ones(3, device=DEV), torch.zeros(3, device=DEV)
    out = torch.full((2, 4, 9, 9), SENTINEL, device=DEV)
    st = _lib._stream()

    def call(o=out, xx=x, ww=w, bb=b, ss=sl, aa=a, tt=t, B=2, Ci=3, Co=4, H=9, W=9, kh=3, kw=3, s=1, py=1, px=1):
        ptr = lambda v: None if v is None else v.data_ptr()
        return L.te_conv2d_prelu_f32(ptr(o), ptr(xx), ptr(ww), ptr(bb), ptr(ss), ptr(aa), ptr(tt), B, Ci, Co, H, W, kh, kw, s, py, px, st)
    assert call(s=3) == -3 and call(s=0) == -3
    assert call(kh=8, py=0) == -3 and call(kw=0) == -3
    assert call(py=3) == -2 and call(px=3) == -2 and call(py=-1) == -2
    assert call(H=2, kh=3, py=0) == -2 and call(W=1, kw=5, px=1) == -2                        # Ho < 1, Wo < 1
    assert call(o=None) == -1 and call(xx=None) == -1 and call(ww=None) == -1 and call(bb=None) == -1
    assert call(ss=None) == -1 and b'NULL' in L.te_last_error_string()                         # the slope is not optional
    assert call(aa=None) == -1 and b'both' in L.te_last_error_string() and call(tt=None) == -1  # the affine is given whole or not at all
    assert call(B=0) == -2 and call(Ci=0) == -2 and call(Co=0) == -2
    with pytest.raises(RuntimeError, match='stride must be 1 or 2'):
        _lib.conv2d_prelu(x, w[:, :27].reshape(4, 3, 3, 3).contiguous(), b, sl, a, t, 3, (1, 1))
    with pytest.raises(RuntimeError, match='inconsistent shapes'):
        _lib.conv2d_prelu(x, w[:, :27].reshape(4, 3, 3, 3).contiguous(), b, sl[:3], a, t, 1, (1, 1))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                                     # nothing was launched
    assert call() == 0 and call(aa=None, tt=None) == 0                                       # ... and valid arguments run
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ---------------------------------------------------------------------------------------------------------- 2. the stem
# (S, box, Pn, N, Co)
STEM_CASES = [(64, (9, 56, 8, 55), 28, 2, 24),          # 47 -> 28: windows of 2 and 3 rows
              (47, (3, 44, 5, 40), 24, 3, 16),          # unequal sides: 41 x 35 -> 24 x 24, windows of 2 and 3
              (256, R.BOX, R.POOL, 1, 64)]              # the true geometry: 188 -> 112, the wide tile


def _stem_weights(Co, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Co, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5, torch.randn(Co, generator=g) * 0.3, 0.25 + 0.3 * torch.randn(Co, generator=g)


@pytest.mark.parametrize('S,box,Pn,N,Co', STEM_CASES)
def test_stem_is_conv2d_prelu_on_the_pooled_crop(S, box, Pn, N, Co):
    """the contract: bitwise te_conv2d_prelu_f32(te_adaptive_avgpool_f32(the contiguous crop), NULL, NULL, ...) - whatever lies outside
    the window"""
    from transeditor_amd import _lib
    w, b, slope = (t.to(DEV) for t in _stem_weights(Co, S + Pn))
    x = R.images(S + 1, N, S)
    y0, y1, x0, x1 = box
    crop = x[:, :, y0:y1, x0:x1].contiguous().to(DEV)
    pooled = _lib.adaptive_avgpool(crop, Pn, Pn)
    want = _lib.conv2d_prelu(pooled, w, b, slope, None, None, 1, (1, 1))
    y = _lib.id_stem_fwd(x.to(DEV), w, b, slope, box, Pn)
    assert y.shape == (N, Co, Pn, Pn) and y.dtype == torch.float32 and y.is_contiguous()
    assert torch.equal(y, want)
    assert 0.2 < float((y > 0).float().mean()) < 0.8                            # (not a comparison of zeros; both PReLU branches)
    far = torch.full_like(x, 1e30)
    far[:, :, y0:y1, x0:x1] = x[:, :, y0:y1, x0:x1]
    assert torch.equal(_lib.id_stem_fwd(far.to(DEV), w, b, slope, box, Pn), want)


def test_stem_against_fp64():
    """rel_l2 < 1e-6 against the restated crop, pool, convolution and PReLU in fp64: the bar of test_gpu_pose.py::test_stem_against_fp64
    for a short chain (a window of at most 9 pixels, a 27-term fp32 chain)"""
    from transeditor_amd import _lib
    S, box, Pn, N, Co = STEM_CASES[0]
    w, b, slope = _stem_weights(Co, 7)
    x = R.images(11, N, S)
    y = _lib.id_stem_fwd(x.to(DEV), w.to(DEV), b.to(DEV), slope.to(DEV), box, Pn)
    ref = F.prelu(F.conv2d(R.extract(x, box, Pn, torch.float64), w.double(), b.double(), 1, 1), slope.double())
    e = rel_l2(y, ref)
    print(f'id stem N={N} {S} px box {box} -> {Pn}: rel_l2 {e:.3e}')
    assert e < 1e-6


def test_stem_refusals():
    from transeditor_amd import _lib
    L = _lib.lib()
    w, b, slope = (t.to(DEV) for t in _stem_weights(8, 3))
    x = torch.zeros(1, 3, 40, 40, device=DEV)
    out = torch.full((1, 8, 16, 16), SENTINEL, device=DEV)
    st = _lib._stream()

    def call(N=1, H=40, W=40, y0=4, y1=36, x0=4, x1=36, Pn=16, Co=8, o=out, s=slope):
        ptr = lambda v: None if v is None else v.data_ptr()
        return L.te_id_stem_fwd_f32(ptr(o), x.data_ptr(), w.data_ptr(), b.data_ptr(), ptr(s), N, H, W, y0, y1, x0, x1, Pn, Co, st)
    for kw in [dict(y1=4), dict(x1=4), dict(y0=10, y1=8), dict(y1=41), dict(x1=41), dict(y0=-1), dict(x0=-1), dict(Pn=0), dict(Pn=-3),
               dict(N=0), dict(N=65536), dict(Co=0), dict(H=30), dict(W=30)]:
        assert call(**kw) == -2, kw
    assert call(o=None) == -1 and call(s=None) == -1 and b'NULL' in L.te_last_error_string()
    with pytest.raises(RuntimeError, match='window'):
        _lib.id_stem_fwd(x, w, b, slope, (4, 44, 4, 36), 16)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                       # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- 3. squeeze-and-excitation
SE_SHAPES = [(1, 64, 4), (5, 40, 3), (3, 512, 32)]


def _se_case(B, C, Rn):
    """pooled ~ N(0, 1), fc1 He-scaled, fc2 scaled so that the logits spread over a few units: the gates fill (0, 1)"""
    g = torch.Generator().manual_seed(100 * B + C + Rn)
    return torch.randn(B, C, generator=g), torch.randn(Rn, C, generator=g) * (2.0 / C) ** 0.5, torch.randn(C, Rn, generator=g) * 2.5 / Rn ** 0.5


def _se_ref(p, w1, w2, dtype):
    return torch.sigmoid(F.relu(p.to(dtype) @ w1.to(dtype).t()) @ w2.to(dtype).t())


@pytest.mark.parametrize('B,C,Rn', SE_SHAPES)
def test_se_excite(B, C, Rn):
    """rel_l2 of the gates against fp64 <= 4 x that of torch's fp32 on the CPU for the same inputs; a row does not depend on B; a NaN row
    stays in its own image"""
    from transeditor_amd import _lib
    p, w1, w2 = _se_case(B, C, Rn)
    g64 = _se_ref(p, w1, w2, torch.float64)
    assert float(g64.min()) < 0.1 and float(g64.max()) > 0.9
    got = _lib.se_excite(p.to(DEV), w1.to(DEV), w2.to(DEV))
    assert got.shape == (B, C) and got.dtype == torch.float32
    e, yard = rel_l2(got, g64), rel_l2(_se_ref(p, w1, w2, torch.float32), g64)
    print(f'se_excite B={B} C={C} R={Rn}: library {e:.3e}, torch fp32 on the CPU {yard:.3e}, ratio {e / yard:.2f}')
    assert e <= 4 * yard
    more = torch.cat([p, torch.randn(2, C, generator=torch.Generator().manual_seed(1))])
    again = _lib.se_excite(more.to(DEV), w1.to(DEV), w2.to(DEV))
    assert torch.equal(again[:B], got) and torch.equal(_lib.se_excite(p[:1].to(DEV), w1.to(DEV), w2.to(DEV)), got[:1])
    more[B, C // 2] = float('nan')
    bad = _lib.se_excite(more.to(DEV), w1.to(DEV), w2.to(DEV))
    assert bool(bad[B].isnan().all()) and torch.equal(bad[:B], got) and torch.equal(bad[B + 1], again[B + 1])


def test_se_excite_saturates_without_overflow_and_refuses():
    """logits of exactly +-100 (fc1 = the identity on positive pooled values, fc2 = diag(+-100)): finite gates in [0, 1], 1 at +100 and
    below 1e-40 at -100"""
    from transeditor_amd import _lib
    C = 8
    sign = torch.tensor([1.0, -1.0] * (C // 2))
    got = _lib.se_excite(torch.ones(2, C, device=DEV), torch.eye(C, device=DEV), torch.diag(100.0 * sign).to(DEV)).cpu()
    assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert bool((got[:, sign > 0] == 1.0).all()) and bool((got[:, sign < 0] < 1e-40).all())
    L, st = _lib.lib(), _lib._stream()
    out = torch.full((2, C), SENTINEL, device=DEV)
    z = torch.zeros(2048, 8, device=DEV)
    for B, Cn, Rn in [(0, 8, 4), (2, 0, 4), (2, 8, 0), (2, 8, 1025), (-1, 8, 4)]:
        assert L.te_se_excite_f32(out.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), B, Cn, Rn, st) == -2, (B, Cn, Rn)
    assert L.te_se_excite_f32(out.data_ptr(), None, z.data_ptr(), z.data_ptr(), 2, 8, 4, st) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- 4. res * gate + shortcut
# (B, C, Ho, Wo, s, Hs, Ws)
ADD_SHAPES = [(2, 5, 7, 7, 1, 7, 7), (2, 5, 4, 4, 2, 7, 7), (1, 3, 8, 12, 1, 8, 12), (1, 3, 6, 5, 2, 11, 9)]


@pytest.mark.parametrize('B,C,Ho,Wo,s,Hs,Ws', ADD_SHAPES)
def test_se_scale_add(B, C, Ho, Wo, s, Hs, Ws):
    """bitwise res * gate[:, :, None, None] + sc[:, :, ::s, ::s] as torch's fp32 computes it on the CPU (two roundings, no fma); without
    a gate res + sc[...]; a shortcut of another size is refused"""
    from transeditor_amd import _lib
    g = torch.Generator().manual_seed(B + 10 * C + 100 * Ho + Wo)
    res, gate, sc = torch.randn(B, C, Ho, Wo, generator=g), torch.rand(B, C, generator=g), torch.randn(B, C, Hs, Ws, generator=g)
    got = _lib.se_scale_add(res.to(DEV), gate.to(DEV), sc.to(DEV), s)
    assert got.shape == res.shape and got.dtype == torch.float32
    assert torch.equal(got.cpu(), res * gate[:, :, None, None] + sc[:, :, ::s, ::s])
    assert torch.equal(_lib.se_scale_add(res.to(DEV), None, sc.to(DEV), s).cpu(), res + sc[:, :, ::s, ::s])
    L, st = _lib.lib(), _lib._stream()
    out = torch.full((B, C, Ho, Wo), SENTINEL, device=DEV)
    r, q, h = res.to(DEV), gate.to(DEV), sc.to(DEV)

    def call(ho=Ho, wo=Wo, hs=Hs, ws=Ws, ss=s, b=B, c=C, rr=r):
        return L.te_se_scale_add_f32(out.data_ptr(), None if rr is None else rr.data_ptr(), q.data_ptr(), h.data_ptr(), b, c, ho, wo, hs, ws, ss, st)
    assert call(hs=Hs + s) == -2 and call(ws=Ws + s) == -2 and call(ho=Ho + 1) == -2 and call(wo=Wo - 1) == -2
    assert call(ss=3 - s) == -2                                                 # the other stride gives another size
    assert call(ss=3) == -3 and call(ss=0) == -3 and call(b=0) == -2 and call(c=0) == -2 and call(rr=None) == -1
    with pytest.raises(RuntimeError, match='shortcut'):
        _lib.se_scale_add(r, q, h[:, :, :-1].contiguous() if Hs > 1 else h, s)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                        # nothing was launched


# ---------------------------------------------------------------------------------------------------------- 5. the rows
@pytest.mark.parametrize('D', [4, 512, 515])
def test_rows_unit_and_dot(D):
    """te_rows_unit_f32 against fp64 within 2 x 2^-24 of each element (the rounding of the norm and the division's; the fp64 sum
    contributes 2^-53); a zero row gives NaN.  te_rows_dot_f32 within (log2 D + 2) 2^-24 sum |a||b| of fp64."""
    from transeditor_amd import _lib
    g = torch.Generator().manual_seed(D)
    a, b = torch.randn(5, D, generator=g), torch.randn(5, D, generator=g)
    a[3] = 0.0
    u = _lib.rows_unit(a.to(DEV)).cpu()
    assert u.shape == (5, D) and bool(u[3].isnan().all())
    live = [0, 1, 2, 4]
    ref = a.double()[live] / a.double()[live].norm(dim=1, keepdim=True)
    err = (u[live].double() - ref).abs()
    print(f'rows_unit D={D}: max err / |ref| {float((err / ref.abs()).max()) / EPS:.3f} x 2^-24')
    assert bool((err <= 2 * EPS * (1 + EPS) * ref.abs()).all())
    assert torch.equal(_lib.rows_unit(a[:1].to(DEV)).cpu(), u[:1])
    d = _lib.rows_dot(a.to(DEV), b.to(DEV)).cpu()
    d64, mag = (a.double() * b.double()).sum(1), (a.double() * b.double()).abs().sum(1)
    assert d.shape == (5,) and float(d[3]) == 0.0
    print(f'rows_dot D={D}: max err / bound {float(((d.double() - d64).abs()[live] / ((math.log2(D) + 2) * EPS * mag[live])).max()):.4f}')
    assert bool(((d.double() - d64).abs() <= (math.log2(D) + 2) * EPS * mag).all())
    assert torch.equal(_lib.rows_dot(a[:2].to(DEV), b[:2].to(DEV)).cpu(), d[:2])
    L, st = _lib.lib(), _lib._stream()
    out = torch.full((5, D), SENTINEL, device=DEV)
    p = a.to(DEV).data_ptr()
    assert L.te_rows_unit_f32(out.data_ptr(), p, 0, D, st) == -2 and L.te_rows_unit_f32(out.data_ptr(), p, 5, 0, st) == -2
    assert L.te_rows_unit_f32(out.data_ptr(), None, 5, D, st) == -1
    assert L.te_rows_dot_f32(out.data_ptr(), p, p, 0, D, st) == -2 and L.te_rows_dot_f32(out.data_ptr(), p, None, 5, D, st) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- 6. end to end, small
SMALL_UNITS = ((16, 16, 2), (16, 16, 1), (16, 32, 2), (32, 32, 1))
# (units, ir_se, B, explicit unit list)
E2E_CASES = [(SMALL_UNITS, True, 5, False), (SMALL_UNITS, False, 5, False), (((24, 24, 2), (24, 40, 2), (40, 40, 1)), True, 3, True)]
E2E_S, E2E_BOX, E2E_POOL, E2E_DIM = 64, (8, 56, 8, 56), 32, 64


def _small_state_dict(seed, units, se, x):
    return R.state_dict(seed, units=list(units), images=x, box=E2E_BOX, pool=E2E_POOL, se=se, dim=E2E_DIM, reduction=4)


@pytest.fixture(scope='module')
def e2e():
    """per case: the network, the images, the library's embeddings, the fp64 restatement with its gates and the yardstick = rel_l2 of the
    SAME restatement run by torch in fp32 against fp64.  Computed once, shared and never modified."""
    from transeditor_amd.arcface import ArcFaceID
    out = {}
    for case in E2E_CASES:
        units, se, B, explicit = case
        x = R.images(101, B, E2E_S)
        sd = _small_state_dict(3, units, se, x)
        net = ArcFaceID(state_dict=sd, box=E2E_BOX, pool=E2E_POOL, units=list(units) if explicit else None)
        gates = []
        e64 = R.embed(x, sd, torch.float64, list(units), E2E_BOX, E2E_POOL, gates)
        out[case] = dict(net=net, x=x.to(DEV), sd=sd, emb=net(x.to(DEV)), e64=e64, gates=gates,
                         yard=rel_l2(R.embed(x, sd, torch.float32, list(units), E2E_BOX, E2E_POOL), e64))
    return out


@pytest.mark.parametrize('case', E2E_CASES, ids=['ir_se', 'ir', 'ragged'])
def test_embedding_end_to_end(e2e, case):
    """Bar: 4 x the error of the fp32 torch restatement (batch norms unfolded) on the same inputs, on the rel_l2 of the embeddings, the
    project's convention; a similarity within 4 x yardstick x 2 of fp64 (two unit vectors, each within the bar).  Non-degeneracy is
    asserted on the fp64 restatement, not on the library.  Measured on the MI355X: profiles/README.md, 'Identity embedding'."""
    units, se, B, _ = case
    d = e2e[case]
    net, emb, e64, yard = d['net'], d['emb'], d['e64'], d['yard']
    assert net.units == tuple(units) and net.se == (se,) * len(units) and net.dim == E2E_DIM
    assert emb.shape == (B, E2E_DIM) and emb.dtype == torch.float32 and emb.is_cuda
    bar = 4 * yard
    cos = e64 @ e64.t()
    assert float((1 - cos + 9 * torch.eye(B, dtype=torch.float64)).min()) >= 100 * bar          # different images are told apart
    if se:
        g = torch.cat(d['gates'])
        assert float(g.min()) < 0.1 and float(g.max()) > 0.9
    assert any(bool((v < 0).any()) for k, v in d['sd'].items() if k.endswith('res_layer.2.weight'))
    e = rel_l2(emb, e64)
    other = emb.roll(1, 0).contiguous()
    sim = net.similarity(emb, other).double().cpu()
    sim64 = (e64 * e64.roll(1, 0)).sum(1)
    print(f'ArcFaceID units {units} se={se} B={B}: library {e:.3e}, fp32 torch {yard:.3e} (rel_l2 of the embeddings against fp64), ratio '
          f'{e / yard:.2f}; similarity max err / bar {float((sim - sim64).abs().max()) / (2 * bar):.3f}')
    assert e <= bar
    assert bool(((sim - sim64).abs() <= 2 * bar).all())
    assert bool(((emb.double().norm(dim=1) - 1).abs() <= 4 * EPS).all())
    assert torch.equal(net(d['x'][:1]), emb[:1])                                # a batch of one: the same bits
    assert torch.equal(net.embed(d['x']), emb)


# ---------------------------------------------------------------------------------------------------------- 7. the true geometry
@pytest.fixture(scope='module')
def true_geometry():
    """IR-SE50 at 256 px: every weight is drawn from the seed, the SE calibration factors are the golden file's (tools/arcface_golden.py
    found them in fp64)"""
    from transeditor_amd.arcface import ArcFaceID
    z, G = load_golden('arcface_ref'), R.GOLDEN
    sd = R.state_dict(G['seed'], fc2_scale=z['fc2_scale'].tolist())
    net = ArcFaceID(state_dict=sd)
    x = R.images(G['image_seed'], G['B'], G['S']).to(DEV)
    return dict(emb=net(x).cpu(), net=net, shapes={k: tuple(t.shape) for k, t in sd.items()})


def test_true_geometry_against_the_reference(true_geometry):
    """tests/golden/arcface_ref.npz (tools/arcface_golden.py): the embeddings the reference's own Backbone(112, 50, mode='ir_se') returns
    in fp32 on the CPU for these weights and images behind the restated crop and pool, and the fp64 restatement's.  The yardstick is
    the reference's rel_l2 against fp64; the library is held to 4 x it against fp64 and to 5 x it against the reference.  The keys
    ArcFaceID reads are the reference class's."""
    from transeditor_amd.arcface import default_units
    z, G, d = load_golden('arcface_ref'), R.GOLDEN, true_geometry
    assert [int(z[k]) for k in ('seed', 'image_seed', 'B', 'S')] == [G[k] for k in ('seed', 'image_seed', 'B', 'S')]
    net = d['net']
    assert list(net.units) == default_units() == R.UNITS50 and all(net.se) and net.dim == 512 and net.affine
    ref_shapes = {str(k): tuple(int(v) for v in str(s).split(',') if v) for k, s in zip(z['keys'], z['shapes'])}
    assert ref_shapes == d['shapes']                                           # the synthetic state dict IS the reference class's layout
    assert set(net.keys) == {k for k in ref_shapes if not k.endswith('num_batches_tracked')}
    e_ref, e64 = z['emb'], z['emb64']
    yard = rel_l2(e_ref, e64)
    assert float(1 - (e64[0].double() * e64[1].double()).sum()) >= 100 * 4 * yard
    e, e_vs_ref = rel_l2(d['emb'], e64), rel_l2(d['emb'], e_ref)
    print(f'ArcFaceID, IR-SE50 at 256 px: library {e:.3e}, the reference {yard:.3e} (rel_l2 of the embeddings against fp64), ratio '
          f'{e / yard:.2f}; library against the reference {e_vs_ref:.3e}')
    assert e <= 4 * yard
    assert e_vs_ref <= 5 * yard


# ---------------------------------------------------------------------------------------------------------- 8. plumbing
def test_feature_sweeps_on_the_device(e2e):
    from transeditor_amd.edit_eval import feature_sweeps, identity_similarity
    net = e2e[E2E_CASES[0]]['net']
    origin = R.images(12, 2, E2E_S).to(DEV)
    sweeps = {k: torch.stack([R.images(20 + 10 * i + j, 2, E2E_S) for j in range(6)], 1).to(DEV) for i, k in enumerate(('p', 'z', 'pz'))}
    res = feature_sweeps(net, origin, sweeps, batch=4)                          # 12 images in batches of 4
    want = net(origin).cpu().numpy()
    for space in ('p', 'z', 'pz'):
        got = res[space]
        assert got.shape == (2, 7, E2E_DIM) and got.dtype == np.float32
        assert np.array_equal(got[:, 3], want)                                  # the origin, in the middle
        each = net(sweeps[space].flatten(0, 1)).view(2, 6, -1).cpu().numpy()
        assert np.array_equal(np.delete(got, 3, axis=1), each)                  # another batch split: still the same bits
        sim = identity_similarity(got)
        assert sim.shape == (2, 7) and bool((sim[:, 3] == 1.0).all()) and float(np.delete(sim, 3, axis=1).max()) < 0.999


def test_input_checks(e2e):
    net = e2e[E2E_CASES[0]]['net']
    with pytest.raises(ValueError, match='square'):
        net(torch.zeros(1, 3, 64, 60, device=DEV))
    with pytest.raises(ValueError, match='does not lie inside'):
        net(torch.zeros(1, 3, 48, 48, device=DEV))
    with pytest.raises(ValueError, match=r'\[B,3,S,S\]'):
        net(torch.zeros(1, 1, 64, 64, device=DEV))
    with pytest.raises(RuntimeError, match='needs a GPU'):
        net(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match='needs a GPU'):
        net.similarity(torch.zeros(2, 8), torch.zeros(2, 8))
    with pytest.raises(ValueError, match='one shape'):
        net.similarity(torch.zeros(2, 8, device=DEV), torch.zeros(3, 8, device=DEV))
    assert net(torch.zeros(2, 3, 56, 56, device=DEV)).shape == (2, E2E_DIM)     # the box ends at the image's edge

"""Encoder head training on the GPU (transeditor_amd.psp_heads_train, csrc/psp_heads_bwd.hip) against fp64 torch on the CPU: the grouped
data gradient (bitwise te_conv2d_dgrad_f32 per head), the weight and bias gradient on its unsplit and its split route, the upsample
adjoint, the codes adjoint, the whole node against the pinned restatement (tests/psp_heads_bwd_restated.py) with torch's own fp32 as
the yardstick, one and eight training steps, and a step through the real generator.

Measured ratios: profiles/README.md, 'Encoder head training'."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import arcface_restated as R
import psp_encoder_restated as P
import psp_heads_bwd_restated as HB
from conftest import rel_l2
from fp64_check import KINK_CAP, SENTINEL, U32 as EPS, guarded, report_fixture, untouched, within

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SLOPE = 0.01
SLOPE32 = float(np.float32(SLOPE))                       # the slope as the kernels receive it
_IDS = dict(ids=lambda c: 'x'.join(map(str, c)))
RESULTS = []
_report = report_fixture('encoder head training: max err / bound against fp64', RESULTS, widths=(44, 10))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------- 1. the grouped data gradient
# (B, G, Ci, Cg, H, k, s)
DG_CASES = [(3, 3, 64, 128, 8, 3, 2),                     # two channel blocks of g per head, a phase tile that spans images
            (2, 2, 64, 64, 16, 3, 2),                     # two pixel tiles per phase
            (2, 3, 64, 64, 2, 3, 2),                      # the 2 -> 1 plane: three of the four phases see fewer taps
            (2, 2, 128, 64, 7, 3, 2),                     # an odd plane: the four phases have different sizes
            (2, 5, 64, 64, 1, 1, 1)]                      # the grouped linear


@functools.lru_cache(maxsize=None)
def _dg(case):
    """inputs, the fp64 accumulators per head and the bound's magnitude |g| * |w|; computed once per case, never modified"""
    from transeditor_amd import _lib
    B, G, Ci, Cg, H, k, s = case
    pad = k // 2
    Ho = (H + 2 * pad - k) // s + 1
    gen = torch.Generator().manual_seed(sum(p * v for p, v in zip((3, 5, 7, 11, 13, 17, 19), case)))
    g = torch.randn(B, G * Cg, Ho, Ho, generator=gen)
    w = torch.randn(G, Cg, Ci, k, k, generator=gen) * (1.0 / (Cg * k * k)) ** 0.5
    act = torch.randn(B, G * Ci, H, H, generator=gen)
    acc, mag = [], []
    for h in range(G):
        gh, wh = g[:, h * Cg:(h + 1) * Cg].double(), w[h].double()
        acc.append(torch.nn.grad.conv2d_input((B, Ci, H, H), wh, gh, s, pad))
        mag.append(torch.nn.grad.conv2d_input((B, Ci, H, H), wh.abs(), gh.abs(), s, pad))
    acc, mag = torch.cat(acc, 1), torch.cat(mag, 1)
    taps = torch.tensor([[ny * nx for _, nx in _lib.dgrad_phases(k, s, pad)] for _, ny in _lib.dgrad_phases(k, s, pad)], dtype=torch.float64)
    K = Cg * taps[torch.arange(H) % s][:, torch.arange(H) % s]                 # Cg * ny * nx of the phase of (y, x)
    return dict(g=g, w=w, act=act, acc=acc, mag=mag, K=K, pad=pad, Ho=Ho, gd=g.to(DEV), actd=act.to(DEV),
                wt=_lib.heads_dgrad_weight(w.to(DEV), s, (pad, pad)))


def _dg_run(case, d, act='given', g=None, c0=0):
    from transeditor_amd import _lib
    B, G, Ci, Cg, H, k, s = case
    return _lib.conv2d_heads_dgrad(d['gd'] if g is None else g, d['wt'], (B, G * Ci, H, H), G, (k, k), s, (d['pad'], d['pad']),
                                   act=d['actd'] if act == 'given' else None, slope=SLOPE, c0=c0)


@pytest.mark.parametrize('case', DG_CASES, **_IDS)
def test_heads_dgrad_is_conv2d_dgrad_per_head(case):
    """bit for bit te_conv2d_dgrad_f32 on every head alone, with pre = the head's slice of act and a slope vector filled with the scalar;
    act = NULL gives the bare accumulators; g read as a slice of a wider tensor gives the same bits"""
    from transeditor_amd import _lib
    B, G, Ci, Cg, H, k, s = case
    d = _dg(case)
    pad = (d['pad'], d['pad'])
    got, bare = _dg_run(case, d), _dg_run(case, d, act=None)
    assert got.shape == (B, G * Ci, H, H) and got.dtype == torch.float32 and got.is_contiguous()
    slope = torch.full((Ci,), SLOPE, device=DEV)
    for h in range(G):
        gh = d['gd'][:, h * Cg:(h + 1) * Cg].contiguous()
        wt = _lib.dgrad_weight(d['w'][h].to(DEV), s, pad)
        pre = d['actd'][:, h * Ci:(h + 1) * Ci].contiguous()
        assert torch.equal(got[:, h * Ci:(h + 1) * Ci], _lib.conv2d_dgrad(gh, wt, (B, Ci, H, H), (k, k), s, pad, pre=pre, slope=slope)), h
        assert torch.equal(bare[:, h * Ci:(h + 1) * Ci], _lib.conv2d_dgrad(gh, wt, (B, Ci, H, H), (k, k), s, pad)), h
    wide = torch.full((B, 5 + G * Cg + 3, d['Ho'], d['Ho']), float('nan'), device=DEV)
    wide[:, 5:5 + G * Cg] = d['gd']
    assert torch.equal(_dg_run(case, d, g=wide, c0=5), got)


@pytest.mark.parametrize('case', DG_CASES, **_IDS)
def test_heads_dgrad_against_fp64(case):
    """elementwise within (K + 5) 2^-24 (|g| * |w|), K = Cg * ny * nx of the phase, no element left out (act is an input: there is no
    kink); both branches of the mask are live; the guard bands around gx are untouched and every element of gx is written"""
    from transeditor_amd import _lib
    B, G, Ci, Cg, H, k, s = case
    d = _dg(case)
    L = _lib.lib()
    share = float((d['act'] > 0).double().mean())
    assert 0.2 < share < 0.8
    want = torch.where(d['act'] > 0, d['acc'], d['acc'] * SLOPE32)
    n = B * G * Ci * H * H
    buf, inner = guarded(n, DEV)
    rc = L.te_conv2d_heads_dgrad_f32(inner.data_ptr(), d['gd'].data_ptr(), d['wt'].data_ptr(), d['actd'].data_ptr(), B, G, Ci, Cg, H, H, k, k, s,
                                     d['pad'], d['pad'], G * Cg, 0, SLOPE, _stream())
    assert rc == 0
    untouched(str(case), 'gx', buf, n, torch.ones(n, dtype=torch.bool, device=DEV))
    got = inner.view(B, G * Ci, H, H)
    assert torch.equal(got, _dg_run(case, d))
    bound = (d['K'] + 5) * EPS * d['mag']
    within('heads_dgrad ' + 'x'.join(map(str, case)), 'gx', got, want, bound, results=RESULTS)
    within('heads_dgrad ' + 'x'.join(map(str, case)), 'bare', _dg_run(case, d, act=None), d['acc'], bound, results=RESULTS)


@pytest.mark.parametrize('case', DG_CASES, **_IDS)
def test_heads_dgrad_nan_reaches_its_own_window(case):
    """a NaN in g (head 1, image 1) reaches exactly the inputs of that head and image whose window holds it"""
    B, G, Ci, Cg, H, k, s = case
    d = _dg(case)
    oy, ox = d['Ho'] - 1, 0
    g = d['gd'].clone()
    g[1, Cg + 3, oy, ox] = float('nan')
    got = _dg_run(case, d, g=g)
    want = torch.zeros(B, G * Ci, H, H, dtype=torch.bool)
    for ky in range(k):
        for kx in range(k):
            y, x = s * oy - d['pad'] + ky, s * ox - d['pad'] + kx
            if 0 <= y < H and 0 <= x < H:
                want[1, Ci:2 * Ci, y, x] = True
    assert bool(want.any()) and torch.equal(got.isnan().cpu(), want)
    assert torch.equal(got.cpu()[~want], _dg_run(case, d).cpu()[~want])


def test_heads_dgrad_refusals_launch_nothing():
    from transeditor_amd import _lib
    case = DG_CASES[1]
    B, G, Ci, Cg, H, k, s = case
    d = _dg(case)
    L = _lib.lib()
    out = torch.full((B, G * Ci, H, H), SENTINEL, device=DEV)
    p = dict(gx=out.data_ptr(), g=d['gd'].data_ptr(), wt=d['wt'].data_ptr(), act=d['actd'].data_ptr())

    def run(Ci_=Ci, slope=SLOPE, **null):
        q = dict(p, **null)
        return L.te_conv2d_heads_dgrad_f32(q['gx'], q['g'], q['wt'], q['act'], B, G, Ci_, Cg, H, H, k, k, s, 1, 1, G * Cg, 0, slope, _stream())
    assert run(Ci_=72) == -3 and b'multiple of 64' in L.te_last_error_string()
    assert run(slope=0.0) == -3 and run(slope=-0.2) == -3 and b'positive' in L.te_last_error_string()
    assert run(gx=None) == -1 and run(g=None) == -1 and run(wt=None) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(RuntimeError, match='te_conv2d_heads_dgrad_f32'):
        _dg_run((B, G, 72, Cg, H, k, s), dict(d, wt=torch.zeros(G * 72 * Cg * 9, device=DEV)), act=None)
    assert run() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, _dg_run(case, d))


# ------------------------------------------------------------------------------------------- 2. the weight and bias gradient
# (B, G, Ci, Cg, H, k, s, shared), splits (0: the rule)
WG_CASES = [((3, 3, 16, 128, 8, 3, 2, 0), 0),             # N = 144: a column tail; R = 48: a reduction tail, no multiple of 32
            ((3, 3, 16, 128, 8, 3, 2, 1), 0),             # the same, on a shared input
            ((2, 2, 64, 64, 2, 3, 2, 0), 0),              # R = 2: the ky = 0 row and the kx = 0 column only ever see padding
            ((2, 5, 64, 64, 1, 1, 1, 0), 0),              # the grouped linear, R = 2
            ((2, 1, 24, 64, 16, 1, 1, 1), 0),             # a lateral: G = 1, Ci no multiple of 32
            ((5, 2, 8, 64, 32, 3, 2, 1), 1),              # R = 1280: 40 reduction steps in one chain
            ((5, 2, 8, 64, 32, 3, 2, 1), 0)]              # the same shape as the rule runs it: split
SPLIT_CASE = WG_CASES[-1]
_WG_IDS = dict(ids=lambda c: 'x'.join(map(str, c[0])) + f'-splits{c[1]}')


@functools.lru_cache(maxsize=None)
def _wg(case):
    """inputs and, per head, fp64 gw / gb with the bounds' magnitudes and torch's fp32 on the CPU; computed once per shape"""
    B, G, Ci, Cg, H, k, s, shared = case
    pad = k // 2
    Ho = (H + 2 * pad - k) // s + 1
    gen = torch.Generator().manual_seed(sum(p * v for p, v in zip((3, 5, 7, 11, 13, 17, 19, 23), case)))
    g = torch.randn(B, G * Cg, Ho, Ho, generator=gen)
    x = torch.randn(B, Ci if shared else G * Ci, H, H, generator=gen)
    shape = (Cg, Ci, k, k)
    gw, mag, cpu32 = [], [], []
    for h in range(G):
        gh, xh = g[:, h * Cg:(h + 1) * Cg], (x if shared else x[:, h * Ci:(h + 1) * Ci])
        gw.append(torch.nn.grad.conv2d_weight(xh.double(), shape, gh.double(), s, pad))
        mag.append(torch.nn.grad.conv2d_weight(xh.double().abs(), shape, gh.double().abs(), s, pad))
        cpu32.append(torch.nn.grad.conv2d_weight(xh, shape, gh, s, pad))
    return dict(g=g, x=x, gd=g.to(DEV), xd=x.to(DEV), gw=torch.stack(gw), mag=torch.stack(mag), cpu32=torch.stack(cpu32), pad=pad, Ho=Ho,
                gb=g.double().sum((0, 2, 3)), magb=g.double().abs().sum((0, 2, 3)), gb32=g.sum((0, 2, 3)), R=B * Ho * Ho)


def _wg_splits(case, splits):
    from transeditor_amd import _lib
    B, G, Ci, Cg, H, k, s, shared = case
    return splits or _lib.conv2d_heads_wgrad_splits(Cg, Ci, k, k, B, _wg(case)['Ho'], _wg(case)['Ho'])


def _wg_run(case, splits, g=None, x=None, G_=None, c0=0):
    from transeditor_amd import _lib
    B, G, Ci, Cg, H, k, s, shared = case
    d = _wg(case)
    return _lib.conv2d_heads_wgrad(d['gd'] if g is None else g, d['xd'] if x is None else x, (G_ or G, Cg, Ci, k, k), s, (d['pad'], d['pad']),
                                   bool(shared), c0, splits)


@pytest.mark.parametrize('case', WG_CASES, **_WG_IDS)
def test_heads_wgrad_against_fp64(case):
    """gw within (R + S + 5) 2^-24 (|g| * |x|) and gb within (R + S + 5) 2^-24 sum|g|, elementwise, no element left out; torch's fp32 on
    the CPU meets the same bounds; guard bands around gw and gb untouched, every element written; padding-only taps are exactly +0"""
    from transeditor_amd import _lib
    (B, G, Ci, Cg, H, k, s, shared), splits = case
    d = _wg(case[0])
    S = _wg_splits(*case)
    if case is SPLIT_CASE:
        assert S > 1
    if splits == 1:
        assert S == 1 and d['R'] == 1280
    L = _lib.lib()
    nw, nb = G * Cg * Ci * k * k, G * Cg
    wbuf, gw = guarded(nw, DEV)
    bbuf, gb = guarded(nb, DEV)
    ws = torch.empty(S * nw if S > 1 else 1, device=DEV)
    rc = L.te_conv2d_heads_wgrad_f32(gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws.numel() * 4, d['gd'].data_ptr(), d['xd'].data_ptr(), B, G, Ci, Cg,
                                     H, H, k, k, s, d['pad'], d['pad'], G * Cg, 0, shared, splits, _stream())
    assert rc == 0
    untouched(str(case), 'gw', wbuf, nw, torch.ones(nw, dtype=torch.bool, device=DEV))
    untouched(str(case), 'gb', bbuf, nb, torch.ones(nb, dtype=torch.bool, device=DEV))
    gw = gw.view(G, Cg, Ci, k, k)
    w2, b2 = _wg_run(case[0], splits)
    assert torch.equal(w2, gw) and torch.equal(b2, gb)
    name = 'heads_wgrad ' + 'x'.join(map(str, case[0])) + f' S={S}'
    within(name, 'gw', gw, d['gw'], (d['R'] + S + 5) * EPS * d['mag'], results=RESULTS, yardstick=(d['cpu32'], 0.0))
    within(name, 'gb', gb, d['gb'], (d['R'] + S + 5) * EPS * d['magb'], results=RESULTS, yardstick=(d['gb32'], 0.0))
    if H == 2 and k == 3:
        edge = torch.cat([gw[..., 0, :].reshape(-1), gw[..., :, 0].reshape(-1)])
        assert bool((edge == 0).all()) and not bool(torch.signbit(edge).any())
        assert bool((gw[..., 1:, 1:] != 0).all())


@pytest.mark.parametrize('case', WG_CASES, **_WG_IDS)
def test_heads_wgrad_reruns_and_one_head_at_a_time(case):
    """two runs give the same bits; G heads in one launch give the bits of G launches of one head; g read as a slice of a wider tensor too"""
    (B, G, Ci, Cg, H, k, s, shared), splits = case
    d = _wg(case[0])
    gw, gb = _wg_run(case[0], splits)
    again = _wg_run(case[0], splits)
    assert torch.equal(gw, again[0]) and torch.equal(gb, again[1])
    for h in range(G):
        xh = d['xd'] if shared else d['xd'][:, h * Ci:(h + 1) * Ci].contiguous()
        w1, b1 = _wg_run(case[0], splits, g=d['gd'][:, h * Cg:(h + 1) * Cg].contiguous(), x=xh, G_=1)
        assert torch.equal(w1[0], gw[h]) and torch.equal(b1, gb[h * Cg:(h + 1) * Cg]), h
    wide = torch.full((B, 7 + G * Cg + 2, d['Ho'], d['Ho']), float('nan'), device=DEV)
    wide[:, 7:7 + G * Cg] = d['gd']
    sliced = _wg_run(case[0], splits, g=wide, c0=7)
    assert torch.equal(sliced[0], gw) and torch.equal(sliced[1], gb)


def test_heads_wgrad_workspace_and_other_refusals_launch_nothing():
    from transeditor_amd import _lib
    (B, G, Ci, Cg, H, k, s, shared), _ = SPLIT_CASE
    d = _wg(SPLIT_CASE[0])
    L = _lib.lib()
    S = _wg_splits(SPLIT_CASE[0], 0)
    nw = G * Cg * Ci * k * k
    need = L.te_conv2d_heads_wgrad_ws_bytes(B, G, Cg, Ci, k, k, d['Ho'], d['Ho'])
    assert S > 1 and need == S * nw * 4
    gw, gb = torch.full((nw,), SENTINEL, device=DEV), torch.full((G * Cg,), SENTINEL, device=DEV)
    ws = torch.full((need // 4,), SENTINEL, device=DEV)

    def run(ws_=ws.data_ptr(), nbytes=need, gw_=gw.data_ptr(), gb_=gb.data_ptr(), g_=d['gd'].data_ptr(), x_=d['xd'].data_ptr(), Cg_=Cg, splits=0):
        return L.te_conv2d_heads_wgrad_f32(gw_, gb_, ws_, nbytes, g_, x_, B, G, Ci, Cg_, H, H, k, k, s, 1, 1, G * Cg, 0, shared, splits, _stream())
    assert run(ws_=None) == -4 and run(nbytes=need - 4) == -4 and b'workspace' in L.te_last_error_string()
    assert run(gw_=None) == -1 and run(gb_=None) == -1 and run(g_=None) == -1 and run(x_=None) == -1
    assert run(Cg_=72) == -3 and run(splits=17) == -2 and run(splits=16) == -2 and b'non-empty' in L.te_last_error_string()      # 40 steps: 3 per range make 14
    torch.cuda.synchronize()
    assert bool((gw == SENTINEL).all()) and bool((gb == SENTINEL).all()) and bool((ws == SENTINEL).all())
    assert run() == 0
    got = _wg_run(SPLIT_CASE[0], 0)
    assert torch.equal(gw.view_as(got[0]), got[0]) and torch.equal(gb, got[1])


# ------------------------------------------------------------------------------------------- 3. the upsample adjoint
# (planes, h, w, H, W)
UP_CASES = [(6, 4, 4, 8, 8), (5, 3, 5, 7, 6), (4, 1, 1, 4, 4), (3, 4, 4, 4, 4), (2, 8, 8, 16, 16)]


def _up64(t, size):
    return F.interpolate(t, size=size, mode='bilinear', align_corners=True)


@pytest.mark.parametrize('case', UP_CASES, **_IDS)
def test_upsample_add_bwd_against_fp64(case):
    """against fp64 autograd of F.interpolate(..., align_corners=True): within (n + 2) 2^-24 times the same adjoint applied to |g|, n the
    largest number of terms one source pixel sums; equal sizes give g bit for bit; <up(x), g> = <x, up_bwd(g)> with the library's
    forward on one side; the add operand is one more fp32 addition"""
    from transeditor_amd import _lib
    planes, h, w, H, W = case
    gen = torch.Generator().manual_seed(sum(p * v for p, v in zip((3, 5, 7, 11, 13), case)))
    g, x, add = torch.randn(1, planes, H, W, generator=gen), torch.randn(1, planes, h, w, generator=gen), torch.randn(1, planes, h, w, generator=gen)

    def adjoint(cot):
        leaf = torch.zeros(1, planes, h, w, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(_up64(leaf, (H, W)), leaf, cot)[0]
    want, mag = adjoint(g.double()), adjoint(g.double().abs())
    basis = torch.eye(h * w, dtype=torch.float64).view(h * w, 1, h, w)
    n = int((_up64(basis, (H, W)) != 0).flatten(1).sum(1).max())
    buf, inner = guarded(planes * h * w, DEV)
    gd = g.to(DEV)
    assert _lib.lib().te_upsample_add_bwd_f32(inner.data_ptr(), gd.data_ptr(), None, planes, h, w, H, W, _stream()) == 0
    untouched(str(case), 'gx', buf, planes * h * w, torch.ones(planes * h * w, dtype=torch.bool, device=DEV))
    got = _lib.upsample_add_bwd(gd, (1, planes, h, w))
    assert torch.equal(got.view(-1), inner)
    within('upsample_add_bwd ' + 'x'.join(map(str, case)), f'n={n}', got, want, (n + 2) * EPS * mag, results=RESULTS)
    if (h, w) == (H, W):
        assert n == 1 and torch.equal(got.cpu(), g)
    if (h, w) == (1, 1):
        assert n == H * W
    up = _lib.upsample_add(x.to(DEV), torch.zeros(1, planes, H, W, device=DEV)).double().cpu()
    lhs, rhs = float((up * g.double()).sum()), float((x.double() * got.double().cpu()).sum())
    scale = float((up.abs() * g.double().abs()).sum())
    assert abs(lhs - rhs) <= 1e-6 * scale
    assert torch.equal(_lib.upsample_add_bwd(gd, (1, planes, h, w), add=add.to(DEV)), got + add.to(DEV))


# ------------------------------------------------------------------------------------------- 4. the codes adjoint
@pytest.mark.parametrize('B,Ns,Np,D,T', [(3, 5, 4, 64, 4), (2, 14, 16, 64, 16)])
def test_psp_codes_bwd_against_fp64(B, Ns, Np, D, T):
    """glat within (Ns + 2) 2^-24 (|A|^T |gz|), gA and gbz within (B * D + 5) 2^-24 of their absolute sums; the spatial part of glat is a
    bitwise copy of gp transposed; two runs give the same bits"""
    from transeditor_amd import _lib
    gen = torch.Generator().manual_seed(B * 1000 + Ns)
    gz, gp = torch.randn(B, D, T, generator=gen), torch.randn(B, D, Np, generator=gen)
    lat, A = torch.randn(B, Ns + Np, D, generator=gen), torch.randn(T, Ns, generator=gen) * Ns ** -0.5
    glat, gA, gbz = _lib.psp_codes_bwd(gz.to(DEV), gp.to(DEV), lat.to(DEV), A.to(DEV))
    assert glat.shape == (B, Ns + Np, D) and gA.shape == (T, Ns) and gbz.shape == (T,)
    z64, l64, A64 = gz.double(), lat.double(), A.double()
    name = f'psp_codes_bwd B={B} Ns={Ns} Np={Np} D={D} T={T}'
    within(name, 'glat', glat[:, :Ns], torch.einsum('tj,bct->bjc', A64, z64), (Ns + 2) * EPS * torch.einsum('tj,bct->bjc', A64.abs(), z64.abs()),
           results=RESULTS)
    within(name, 'gA', gA, torch.einsum('bct,bjc->tj', z64, l64[:, :Ns]), (B * D + 5) * EPS * torch.einsum('bct,bjc->tj', z64.abs(), l64[:, :Ns].abs()),
           results=RESULTS)
    within(name, 'gbz', gbz, z64.sum((0, 1)), (B * D + 5) * EPS * z64.abs().sum((0, 1)), results=RESULTS)
    assert torch.equal(glat[:, Ns:].cpu(), gp.permute(0, 2, 1))
    again = _lib.psp_codes_bwd(gz.to(DEV), gp.to(DEV), lat.to(DEV), A.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(again, (glat, gA, gbz)))


# ------------------------------------------------------------------------------------------- 5. the node, end to end
E2E_B = 3
GROUPS = (('convs.weight', lambda k: '.convs.' in k and k.endswith('weight')), ('convs.bias', lambda k: '.convs.' in k and k.endswith('bias')),
          ('linear', lambda k: '.linear.' in k), ('latlayer', lambda k: k.startswith('latlayer')), ('adjust_style', lambda k: k.startswith('adjust')),
          ('c1 c2 c3', lambda k: k in ('c1', 'c2', 'c3')))


def _cotangents(seed):
    G = P.SMALL
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(E2E_B, G['D'], G['tokens'], generator=gen), torch.randn(E2E_B, G['D'], G['spatials'], generator=gen)


@pytest.fixture(scope='module')
def node():
    """the small encoder of the existing end-to-end test at B = 3: the library's forward and backward, its branch decisions, the fp64
    restatement pinned to them and the yardstick, the same restatement run by torch in fp32 on the CPU.  Computed once, never modified."""
    from transeditor_amd.psp_encoder import DualSpaceEncoder
    from transeditor_amd.psp_heads_train import TrainableHeads
    G = P.SMALL
    x = R.images(211, E2E_B, G['S'])
    sd = P.small_state_dict(6, images=x)
    enc = DualSpaceEncoder(state_dict=sd, taps=G['taps'], units=G['units'])
    heads = TrainableHeads(enc)
    with torch.no_grad():
        c = enc.backbone(x.to(DEV))
    leaves = [t.clone().requires_grad_(True) for t in c]
    z, p = heads(*leaves)
    masks = HB.library_masks(z.grad_fn.kept[1], heads.program, heads.launch_heads, heads.dim)
    gz, gp = _cotangents(7)
    torch.autograd.backward([z, p], [gz.to(DEV), gp.to(DEV)], retain_graph=True)
    got = {k: v.detach().cpu() for k, v in heads.named_by_reference_key(grads=True).items()}
    got.update({f'c{i + 1}': t.grad.cpu() for i, t in enumerate(leaves)})
    c_cpu = [t.cpu() for t in c]
    return dict(enc=enc, heads=heads, x=x, sd=sd, z=z, p=p, c=c_cpu, got=got, masks=masks, gz=gz, gp=gp,
                free64=HB.gradients(c_cpu, sd, gz, gp, torch.float64), pin64=HB.gradients(c_cpu, sd, gz, gp, torch.float64, masks=masks),
                pin32=HB.gradients(c_cpu, sd, gz, gp, torch.float32, masks=masks))


def test_node_forward_is_encode(node):
    """the codes are DualSpaceEncoder.encode's bit for bit (this checkpoint carries no latent averages)"""
    z, p = node['enc'].encode(node['x'].to(DEV))
    assert node['enc'].z_avg is None and torch.equal(node['z'].detach(), z) and torch.equal(node['p'].detach(), p)
    assert node['z'].requires_grad and node['p'].requires_grad


def test_node_backward_against_the_pinned_restatement(node):
    """rel_l2 of the gradient of every parameter tensor under its reference key, and of c1, c2, c3, against the fp64 restatement pinned
    to the library's own branch decisions; the bar is 4 x the yardstick, the rel_l2 of the same restatement run by torch in fp32 on the CPU.
    Condition on the pinning: the library's masks differ from fp64's own in at most KINK_CAP of the elements.  Non-degeneracy: on fp64
    the gradients for two different cotangents differ by at least 100 x the bar."""
    total = sum(m.numel() for m in node['masks'].values())
    flips = sum(int((m != node['free64']['masks'][k]).sum()) for k, m in node['masks'].items())
    negative = 1 - sum(int(m.sum()) for m in node['masks'].values()) / total
    print(f'TrainableHeads small geometry: {flips} of {total} branch decisions differ from fp64, {negative:.2f} negative')
    assert total == 42432 and flips <= KINK_CAP * total
    assert set(node['got']) == set(node['pin64']['grads'])
    other = HB.gradients(node['c'], node['sd'], *_cotangents(8), torch.float64, masks=node['masks'])['grads']
    worst, fails = {}, []
    for key, want in node['pin64']['grads'].items():
        e, yard = rel_l2(node['got'][key], want), rel_l2(node['pin32']['grads'][key], want)
        far = rel_l2(other[key], want)
        group = next(name for name, has in GROUPS if has(key))
        if group not in worst or e * worst[group][1] > worst[group][0] * yard:
            worst[group] = (e, yard, key)
        print(f'  {key:32s} library {e:.3e}  torch fp32 {yard:.3e}  ratio {e / yard:5.2f}  other cotangents {far:.2f}')
        if not (yard > 0 and e <= 4 * yard and far >= 100 * 4 * yard):
            fails.append((key, e, yard, far))
    for group, (e, yard, key) in worst.items():
        print(f'TrainableHeads gradients, {group}: worst ratio {e / yard:.2f} ({key}: library {e:.3e}, torch fp32 {yard:.3e})')
    assert not fails, fails


def test_node_is_once_differentiable_and_reproducible(node):
    """a second forward and backward give the same bits; a second backward on the same graph raises"""
    heads = node['heads']
    leaves = [t.to(DEV).requires_grad_(True) for t in node['c']]
    z, p = heads(*leaves)
    assert torch.equal(z, node['z']) and torch.equal(p, node['p'])
    params = [getattr(heads, k) for k in heads.names]
    grads = torch.autograd.grad([z, p], leaves + params, [node['gz'].to(DEV), node['gp'].to(DEV)], retain_graph=True)
    named = dict(zip(['c1', 'c2', 'c3'] + heads.names, grads))
    from transeditor_amd.psp_heads_train import unpack
    back = unpack(named, heads.launch_heads, heads.dim, heads.n_styles, heads.n_spatials)
    back.update({k: named[k] for k in ('c1', 'c2', 'c3')})
    for k, v in node['got'].items():
        assert torch.equal(back[k].cpu(), v), k
    with pytest.raises(RuntimeError, match='a second time'):
        torch.autograd.grad([z, p], leaves, [node['gz'].to(DEV), node['gp'].to(DEV)])
    # frozen features: no gradient is computed for them and the parameters' are unchanged
    z2, p2 = heads(*[t.to(DEV) for t in node['c']])
    g2 = torch.autograd.grad([z2, p2], params, [node['gz'].to(DEV), node['gp'].to(DEV)])
    assert all(torch.equal(a, named[k]) for a, k in zip(g2, heads.names))


# ------------------------------------------------------------------------------------------- 6. the training step
STEP_LR, W_NORM = 1e-3, 0.005


def _decoder_matrix():
    G = P.SMALL
    rows = G['D'] * (G['tokens'] + G['spatials'])
    return torch.randn(rows, 3 * G['S'] * G['S'], generator=torch.Generator().manual_seed(99), dtype=torch.float64) * rows ** -0.5


def _decode_with(Wd):
    def decode(z, p):
        return (torch.cat([z.flatten(1), p.flatten(1)], 1) @ Wd).view(z.shape[0], 3, P.SMALL['S'], P.SMALL['S'])
    return decode


def _loss_restated(real, inversed, z, p):
    """EncoderLoss(id_lambda=0, lpips_lambda=0, l2_lambda=1, w_norm_lambda=W_NORM) without latent averages (coach_new.py:285-320)"""
    norm = lambda t: torch.sum(t.norm(2, dim=(1, 2))) / t.shape[0]
    return F.mse_loss(inversed, real) + (norm(z) + norm(p)) * W_NORM


@pytest.fixture(scope='module')
def trained():
    """one heads_step from the small encoder's weights, then seven more on the same batch"""
    from transeditor_amd.encoder_loss import EncoderLoss
    from transeditor_amd.optim import Ranger
    from transeditor_amd.psp_encoder import DualSpaceEncoder
    from transeditor_amd.psp_heads_train import TrainableHeads, heads_step
    G = P.SMALL
    x = R.images(211, E2E_B, G['S'])
    sd = P.small_state_dict(6, images=x)
    enc = DualSpaceEncoder(state_dict=sd, taps=G['taps'], units=G['units'])
    heads = TrainableHeads(enc)
    frozen = {k: v.clone() for k, v in enc.state_dict().items()}
    xd = x.to(DEV)
    with torch.no_grad():
        c = enc.backbone(xd)
    z, _ = heads(*c)
    masks = HB.library_masks(z.grad_fn.kept[1], heads.program, heads.launch_heads, heads.dim)
    before = {k: v.cpu().clone() for k, v in heads.named_by_reference_key().items()}
    Wd = _decoder_matrix()
    crit = EncoderLoss(id_lambda=0, lpips_lambda=0, l2_lambda=1, w_norm_lambda=W_NORM)
    opt = Ranger(heads.parameters(), lr=STEP_LR)
    decode = _decode_with(Wd.float().to(DEV))
    losses = [heads_step(enc, heads, decode, crit, opt, xd)]
    after = {k: v.cpu().clone() for k, v in heads.named_by_reference_key().items()}
    losses += [heads_step(enc, heads, decode, crit, opt, xd) for _ in range(7)]
    return dict(enc=enc, heads=heads, sd=sd, x=x, c=[t.cpu() for t in c], masks=masks, before=before, after=after, frozen=frozen, losses=losses, Wd=Wd)


def test_step_is_ranger_on_the_fp64_gradient(trained):
    """after one step every head parameter equals Ranger's first step (tests/ranger_restated.py at step 1) applied to the fp64 gradient
    of the whole loss, within test_gpu_ranger.py's bar: max|p - p64| <= max(4 x yardstick, 2^-20 max|p64|), the yardstick being the same
    update in fp32 from torch's fp32 gradient on the CPU; the backbone's buffers are bitwise unchanged"""
    t = trained

    def grads(dtype):
        keys = HB.trained_keys(t['sd'])
        Pm = {k: t['sd'][k].to(dtype).clone().requires_grad_(True) for k in keys}
        z, p, _ = HB.stage(*[v.to(dtype) for v in t['c']], Pm, t['masks'])
        loss = _loss_restated(t['x'].to(dtype), _decode_with(t['Wd'].to(dtype))(z, p), z, p)
        return dict(zip(keys, torch.autograd.grad(loss, [Pm[k] for k in keys]))), float(loss)
    g64, loss64 = grads(torch.float64)
    g32, _ = grads(torch.float32)
    first = t['losses'][0]
    assert abs(float(first[0]) - loss64) <= 1e-5 * abs(loss64) and first[1]['loss'] == pytest.approx(loss64, rel=1e-5) and first[2] is None
    assert set(first[1]) == {'loss_l2', 'loss_w_norm', 'loss'}
    worst, clear = (0.0, ''), 0.0
    for key, p0 in t['before'].items():
        want = HB.ranger_first_step(p0.double(), g64[key], STEP_LR)
        yard = float((HB.ranger_first_step(p0, g32[key], STEP_LR).double() - want).abs().max())
        bound = max(4 * yard, 2.0 ** -20 * float(want.abs().max()))
        err = float((t['after'][key].double() - want).abs().max())
        moved = float((want - p0.double()).abs().max())
        worst = max(worst, (err / bound, key))
        clear = max(clear, moved / bound)
        assert moved > 0, key
        assert err <= bound, (key, err, bound)
    print(f'heads_step: worst error / bound {worst[0]:.3f} ({worst[1]}); the largest step is {clear:.0f} x its bound')
    assert clear > 10                                                            # a step that was not taken, or taken twice, would not pass
    now = t['enc'].state_dict()
    assert set(now) == set(t['frozen']) and all(torch.equal(now[k], v) for k, v in t['frozen'].items())


def test_eight_steps_lower_the_loss_and_the_export_encodes_the_same(trained):
    from transeditor_amd.psp_encoder import DualSpaceEncoder
    t, G = trained, P.SMALL
    values = [float(l[0]) for l in t['losses']]
    print('heads_step losses over 8 steps on one batch: ' + ' '.join(f'{v:.5f}' for v in values))
    assert all(np.isfinite(values)) and values[-1] < values[0]
    xd = t['x'].to(DEV)
    with torch.no_grad():
        z, p = t['heads'](*t['enc'].backbone(xd))
    tuned = DualSpaceEncoder(state_dict=t['heads'].export_state_dict(t['sd']), taps=G['taps'], units=G['units'])
    z2, p2 = tuned.encode(xd)
    assert torch.equal(z2, z) and torch.equal(p2, p)
    assert not torch.equal(z2, t['enc'].encode(xd)[0])                           # and the heads did move


# ------------------------------------------------------------------------------------------- 7. the real generator
def test_two_steps_through_the_real_generator():
    """the D = 512 encoder geometry and the generator of test_encoder_codes_feed_the_generator: two steps give finite losses, the
    generator's parameters are unchanged and none of them has a gradient"""
    from transeditor_amd import synth
    from transeditor_amd.encoder_loss import EncoderLoss
    from transeditor_amd.model_spatial_query import Generator
    from transeditor_amd.optim import encoder_optimizer
    from transeditor_amd.psp_encoder import DualSpaceEncoder
    from transeditor_amd.psp_heads_train import TrainableHeads, generator_decoder, heads_step
    G = P.SMALL
    sd = P.state_dict(8, units=G['units'], taps=G['taps'], D=512, styles=(1, 1, 1), spatials=16, tokens=16, depth=2, reduction=4)
    gen = Generator(32, 512, 512, 8, n_trans=8, pixel_norm_op_dim=1)
    gsd = gen.state_dict()
    synth.fill_state_dict(gsd, 21)
    gen.load_state_dict(gsd)
    gen = gen.to(DEV)
    enc = DualSpaceEncoder(state_dict=P.checkpoint(sd, plus=True, averages=True), taps=G['taps'], units=G['units'])
    heads = TrainableHeads(enc)
    with pytest.raises(ValueError, match='256 px generator only; this one is 32 px'):
        generator_decoder(gen, enc.from_plus_space)
    decode = generator_decoder(gen, enc.from_plus_space, resize=False)
    before = [p.detach().clone() for p in gen.parameters()]
    crit = EncoderLoss(id_lambda=0, lpips_lambda=0, l2_lambda=1, w_norm_lambda=W_NORM, start_from_latent_avg=True)
    opt = encoder_optimizer(heads.parameters(), 'ranger', 1e-4)
    x = R.images(31, 2, 32).to(DEV)
    old = [p.detach().clone() for p in heads.parameters()]
    losses = [heads_step(enc, heads, decode, crit, opt, x) for _ in range(2)]
    assert all(np.isfinite(float(l[0])) and np.isfinite(l[1]['loss_l2']) and np.isfinite(l[1]['loss_w_norm']) for l in losses)
    assert all(p.grad is None and not p.requires_grad and torch.equal(p, q) for p, q in zip(gen.parameters(), before))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and not torch.equal(p, q) for p, q in zip(heads.parameters(), old))

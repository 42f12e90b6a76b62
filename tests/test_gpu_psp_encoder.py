"""The dual-space pSp encoder (transeditor_amd.psp_encoder, csrc/psp_heads.hip on the main loop of csrc/conv2d_body.h) against
te_conv2d_f32, fp64 torch and the plain-torch restatement (tests/psp_encoder_restated.py): the grouped head convolution on its unsplit
and its split-K route, the refusals of the new entry points, the align_corners upsample-and-add, the code assembly, the whole encoder
on a small geometry and on the true one (against what the reference's own GradualStyleEncoder returns:
tests/golden/psp_encoder_ref.npz)."""
import pytest
import torch
import torch.nn.functional as F

import arcface_restated as R
import psp_encoder_restated as P
from conftest import load_golden, rel_l2
from fp64_check import SENTINEL, U32 as EPS, within

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SLOPE = 0.01
_IDS = dict(ids=lambda c: 'x'.join(map(str, c)))


def _heads_case(B, G, Ci, Cg, H, k, shared, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci if shared else G * Ci, H, H, generator=g)
    return x, torch.randn(G, Cg, Ci, k, k, generator=g) * (1.0 / (Ci * k * k)) ** 0.5, torch.randn(G * Cg, generator=g) * 0.5


def _heads_ref(x, w, b, s, pad, shared, dtype):
    """per head F.conv2d in `dtype` on the CPU -> (pre-activation, the bound's magnitude |w| * |x| + |bias|)"""
    G, Cg, Ci = w.shape[:3]
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    pre, mag = [], []
    for g in range(G):
        xg = x if shared else x[:, g * Ci:(g + 1) * Ci]
        pre.append(F.conv2d(xg, w[g], b[g * Cg:(g + 1) * Cg], s, pad))
        mag.append(F.conv2d(xg.abs(), w[g].abs(), b[g * Cg:(g + 1) * Cg].abs(), s, pad))
    return torch.cat(pre, 1), torch.cat(mag, 1)


# ------------------------------------------------------------------------------------------- 1. the grouped convolution, unsplit route
# (B, G, Ci, Cg, H, k, s, shared)
UNSPLIT_CASES = [(3, 3, 16, 128, 8, 3, 2, 0),            # two channel blocks per head, 48 pixels: a tile that spans the images
                 (3, 3, 16, 128, 8, 3, 2, 1),            # the same shape on a shared input
                 (2, 2, 8, 64, 16, 3, 2, 0),             # P = 128: two pixel tiles
                 (2, 5, 64, 64, 1, 1, 1, 0)]             # the grouped linear layer


def _unsplit_check(case, c0=0, extra=0):
    from transeditor_amd import _lib
    B, G, Ci, Cg, H, k, s, shared = case
    pad = (k // 2, k // 2)
    x, w, b = _heads_case(B, G, Ci, Cg, H, k, shared, sum(p * v for p, v in zip((3, 5, 7, 11, 13, 17, 19, 23), case)))
    pre64, _ = _heads_ref(x, w, b, s, pad[0], shared, torch.float64)
    assert 0.2 < float((pre64 < 0).double().mean()) < 0.8                      # both branches of the leaky ReLU are live
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    Ho = pre64.shape[2]
    out = None
    if c0 or extra:
        out = torch.full((B, G * Cg + c0 + extra, Ho, Ho), SENTINEL, device=DEV)
    got = _lib.conv2d_heads(xd, wd, bd, s, pad, bool(shared), SLOPE, out, c0, splits=1)
    assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == (B, G * Cg + c0 + extra, Ho, Ho)
    for g in range(G):
        xg = xd if shared else xd[:, g * Ci:(g + 1) * Ci].contiguous()
        plain = _lib.conv2d(xg, wd[g].contiguous(), bd[g * Cg:(g + 1) * Cg].contiguous(), s, pad, act=0)
        assert torch.equal(got[:, c0 + g * Cg:c0 + (g + 1) * Cg], F.leaky_relu(plain, SLOPE)), g
    err = (got[:, c0:c0 + G * Cg].double().cpu() - F.leaky_relu(pre64, SLOPE)).abs().max()
    assert float(err) < 1e-4                                                     # (and the plain convolution is the right one)
    return got


@pytest.mark.parametrize('case', UNSPLIT_CASES, **_IDS)
def test_heads_unsplit_is_conv2d_per_head(case):
    """bitwise leaky(te_conv2d_f32(x_g, w_g, b_g, act = 0)) for every head, torch doing the leaky ReLU"""
    _unsplit_check(case)


def test_heads_unsplit_writes_its_slice_only():
    got = _unsplit_check((2, 2, 8, 64, 8, 3, 2, 0), c0=5, extra=9)
    assert bool((got[:, :5] == SENTINEL).all()) and bool((got[:, 5 + 128:] == SENTINEL).all())
    assert not bool((got[:, 5:5 + 128] == SENTINEL).any())


def test_heads_unsplit_wide_tile_equals_the_narrow_one():
    """two heads of 64 channels on a 128 x 128 plane: one image is 128 x 2 = 256 workgroups of 128 pixels, below kWideGridMin = 512, and
    runs on the 64-pixel tile; two images are 512 and take the 128-pixel one.  K = 72 is unsplit by the rule.  The same bits."""
    from transeditor_amd import _lib
    x, w, b = (t.to(DEV) for t in _heads_case(2, 2, 8, 64, 128, 3, 1, 41))
    assert _lib.conv2d_heads_splits(8, 3, 3, 128, 128) == 1
    full = _lib.conv2d_heads(x, w, b, 1, (1, 1), True, SLOPE)
    assert full.shape == (2, 128, 128, 128)
    for i in range(2):
        assert torch.equal(full[i:i + 1], _lib.conv2d_heads(x[i:i + 1].contiguous(), w, b, 1, (1, 1), True, SLOPE)), i
    assert 0.2 < float((full < 0).float().mean()) < 0.8


def test_heads_slope_one_is_the_identity_and_a_nan_propagates():
    from transeditor_amd import _lib
    x, w, b = _heads_case(2, 2, 8, 64, 4, 3, 0, 77)
    x[1, 9, 1, 1] = float('nan')                                                 # head 1 of image 1
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    got = _lib.conv2d_heads(xd, wd, bd, 2, (1, 1), False, 1.0, splits=1)
    want = torch.cat([_lib.conv2d(xd[:, g * 8:(g + 1) * 8].contiguous(), wd[g].contiguous(), bd[g * 64:(g + 1) * 64].contiguous(), 2, (1, 1)) for g in range(2)], 1)
    assert torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))
    nan = got.isnan()
    assert bool(nan[1, 64:].any()) and not bool(nan[0].any()) and not bool(nan[1, :64].any())


# ------------------------------------------------------------------------------------------- 2. the split route
SPLIT_PLANES = [4, 2]                                     # 4 -> 2 and 2 -> 1: 5 of 9 taps of the latter are padding
SPLIT_G, SPLIT_CI, SPLIT_CG = 3, 512, 64


@pytest.fixture(scope='module')
def split_refs():
    """per plane: inputs for B = 3, the fp64 result, the elementwise bound, torch's fp32 on the CPU.  Computed once, never modified."""
    from transeditor_amd import _lib
    out = {}
    for H in SPLIT_PLANES:
        x, w, b = _heads_case(3, SPLIT_G, SPLIT_CI, SPLIT_CG, H, 3, 0, 900 + H)
        pre64, mag = _heads_ref(x, w, b, 2, 1, 0, torch.float64)
        o64 = F.leaky_relu(pre64, SLOPE)
        S = _lib.conv2d_heads_splits(SPLIT_CI, 3, 3, H // 2, H // 2)
        K = SPLIT_CI * 9
        out[H] = dict(x=x, w=w, b=b, o64=o64, S=S, K=K, bound=(K + S + 5) * EPS * mag + EPS * o64.abs(),
                      cpu32=F.leaky_relu(_heads_ref(x, w, b, 2, 1, 0, torch.float32)[0], SLOPE))
    return out


def _run_split(d, B=3, x=None):
    from transeditor_amd import _lib
    x = d['x'] if x is None else x
    return _lib.conv2d_heads(x[:B].contiguous().to(DEV), d['w'].to(DEV), d['b'].to(DEV), 2, (1, 1), False, SLOPE)


@pytest.mark.parametrize('H', SPLIT_PLANES)
def test_heads_split_against_fp64(split_refs, H):
    """elementwise, no element left out; bound (K + S + 5) 2^-24 (|w| * |x| + |bias|) + 2^-24 |out|; torch's fp32 on the CPU meets it too"""
    d = split_refs[H]
    assert d['S'] > 1
    assert 0.2 < float((d['o64'] < 0).double().mean()) < 0.8
    within(f'conv2d_heads split {H} -> {H // 2}', f'S={d["S"]}', _run_split(d), d['o64'], d['bound'], yardstick=(d['cpu32'], 0.0))


@pytest.mark.parametrize('H', SPLIT_PLANES)
def test_heads_split_batch_independence_and_reruns(split_refs, H):
    d = split_refs[H]
    three, again, one = _run_split(d), _run_split(d), _run_split(d, B=1)
    assert torch.equal(three, again)
    assert torch.equal(three[:1], one)


@pytest.mark.parametrize('H', SPLIT_PLANES)
def test_heads_split_nan_reaches_its_own_windows(split_refs, H):
    """a NaN in head 1's input of image 1 reaches exactly the outputs of that head and image whose window holds it"""
    d = split_refs[H]
    x = d['x'].clone()
    x[1, SPLIT_CI + 300, H - 1, 0] = float('nan')
    got = _run_split(d, x=x).cpu()
    want = torch.zeros_like(got, dtype=torch.bool)
    Ho = H // 2
    for oy in range(Ho):
        for ox in range(Ho):
            if 2 * oy - 1 <= H - 1 <= 2 * oy + 1 and 2 * ox - 1 <= 0 <= 2 * ox + 1:
                want[1, SPLIT_CG:2 * SPLIT_CG, oy, ox] = True
    assert bool(want.any()) and torch.equal(got.isnan(), want)
    assert torch.equal(got[~want], _run_split(d).cpu()[~want])


def test_heads_split_workspace_refusals(split_refs):
    from transeditor_amd import _lib
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d = split_refs[4]
    x, w, b = (d[k].to(DEV) for k in ('x', 'w', 'b'))
    out = torch.full((3, SPLIT_G * SPLIT_CG, 2, 2), SENTINEL, device=DEV)
    need = L.te_conv2d_heads_ws_bytes(3, SPLIT_G, SPLIT_CG, SPLIT_CI, 3, 3, 2, 2)
    assert need == d['S'] * out.numel() * 4
    assert L.te_conv2d_heads_ws_bytes(3, SPLIT_G, SPLIT_CG, 16, 3, 3, 2, 2) == 0 and L.te_conv2d_heads_ws_bytes(0, 1, 64, 16, 3, 3, 2, 2) < 0
    ws = torch.full((need // 4,), SENTINEL, device=DEV)
    geo = (3, SPLIT_G, SPLIT_CI, SPLIT_CG, 4, 4, 3, 3, 2, 1, 1, SPLIT_G * SPLIT_CG, 0, 0, SLOPE, 0, st)
    assert L.te_conv2d_heads_f32(out.data_ptr(), None, need, x.data_ptr(), w.data_ptr(), b.data_ptr(), *geo) == -4
    assert L.te_conv2d_heads_f32(out.data_ptr(), ws.data_ptr(), need - 4, x.data_ptr(), w.data_ptr(), b.data_ptr(), *geo) == -4
    assert b'workspace' in L.te_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    assert L.te_conv2d_heads_f32(out.data_ptr(), ws.data_ptr(), need, x.data_ptr(), w.data_ptr(), b.data_ptr(), *geo) == 0
    assert torch.equal(out, _run_split(d))


# ------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing():
    from transeditor_amd import _lib
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    x, w, b = (t.to(DEV) for t in _heads_case(2, 2, 8, 64, 8, 3, 0, 5))
    out = torch.full((2, 128, 4, 4), SENTINEL, device=DEV)
    p = [t.data_ptr() for t in (out, x, w, b)]

    def heads(out_=p[0], x_=p[1], w_=p[2], b_=p[3], B=2, G=2, Ci=8, Cg=64, H=8, W=8, kh=3, kw=3, s=2, py=1, px=1, Ctot=128, c0=0, shared=0, splits=1):
        return L.te_conv2d_heads_f32(out_, None, 0, x_, w_, b_, B, G, Ci, Cg, H, W, kh, kw, s, py, px, Ctot, c0, shared, SLOPE, splits, st)
    assert heads(out_=None) == -1 and heads(x_=None) == -1 and heads(w_=None) == -1 and heads(b_=None) == -1
    assert heads(Cg=72) == -3 and b'multiple of 64' in L.te_last_error_string()
    assert heads(s=3) == -3 and heads(kh=8) == -3
    assert heads(B=0) == -2 and heads(G=0) == -2 and heads(Cg=0) == -2 and heads(py=3) == -2 and heads(c0=1) == -2 and heads(Ctot=127) == -2
    assert heads(splits=-1) == -2 and heads(splits=17) == -2 and heads(splits=3) == -4         # 3 ranges: a workspace is needed
    assert heads(Ci=1, splits=2) == -2 and b'non-empty' in L.te_last_error_string()            # K = 9: one step of k
    assert L.te_conv2d_heads_splits(0, 3, 3, 1, 1) < 0 and L.te_conv2d_heads_splits(8, 9, 3, 1, 1) < 0
    assert L.te_conv2d_heads_splits(8, 3, 3, 4, 4) == 1 and L.te_conv2d_heads_splits(512, 3, 3, 64, 64) == 1
    y = torch.full((6, 8, 8), SENTINEL, device=DEV)
    q = out.data_ptr()
    assert L.te_upsample_add_f32(None, q, q, 6, 4, 4, 8, 8, st) == -1 and L.te_upsample_add_f32(y.data_ptr(), None, q, 6, 4, 4, 8, 8, st) == -1
    assert L.te_upsample_add_f32(y.data_ptr(), q, None, 6, 4, 4, 8, 8, st) == -1
    assert L.te_upsample_add_f32(y.data_ptr(), q, q, 0, 4, 4, 8, 8, st) == -2 and L.te_upsample_add_f32(y.data_ptr(), q, q, 65536, 4, 4, 8, 8, st) == -2
    assert L.te_upsample_add_f32(y.data_ptr(), q, q, 6, 0, 4, 8, 8, st) == -2 and L.te_upsample_add_f32(y.data_ptr(), q, q, 6, 4, 4, 8, 32769, st) == -2
    z = torch.full((2, 64, 4), SENTINEL, device=DEV)
    zp = z.data_ptr()
    assert L.te_psp_codes_f32(None, zp, q, q, q, None, None, 2, 5, 4, 64, 4, st) == -1 and L.te_psp_codes_f32(zp, None, q, q, q, None, None, 2, 5, 4, 64, 4, st) == -1
    assert L.te_psp_codes_f32(zp, zp, None, q, q, None, None, 2, 5, 4, 64, 4, st) == -1 and L.te_psp_codes_f32(zp, zp, q, None, q, None, None, 2, 5, 4, 64, 4, st) == -1
    assert L.te_psp_codes_f32(zp, zp, q, q, None, None, None, 2, 5, 4, 64, 4, st) == -1
    for bad in [(0, 5, 4, 64, 4), (2, 0, 4, 64, 4), (2, 5, 0, 64, 4), (2, 5, 4, 0, 4), (2, 5, 4, 64, 0)]:
        assert L.te_psp_codes_f32(zp, zp, q, q, q, None, None, *bad, st) == -2, bad
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((y == SENTINEL).all()) and bool((z == SENTINEL).all())
    with pytest.raises(RuntimeError, match='te_conv2d_heads_f32'):
        _lib.conv2d_heads(x, w[:, :, :, :, :2].contiguous(), b, 2, (1, 2), False, SLOPE)       # px >= kw
    with pytest.raises(RuntimeError, match='inconsistent shapes'):
        _lib.conv2d_heads(x, w, b[:-1], 2, (1, 1))
    assert heads() == 0                                                          # and a valid call runs
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# ------------------------------------------------------------------------------------------- 4. upsample and add
UP_CASES = [((4, 4), (8, 8)), ((5, 5), (9, 9)), ((3, 5), (7, 6)), ((1, 1), (4, 4)), ((6, 6), (6, 6))]


@pytest.mark.parametrize('src,dst', UP_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_upsample_add_against_fp64(src, dst):
    """elementwise within 4 x 2^-24 (|taps| + |y|) of fp64 F.interpolate(..., align_corners=True) + y; torch's fp32 on the CPU is held to
    the same bound; equal sizes give bitwise x + y"""
    from transeditor_amd import _lib
    g = torch.Generator().manual_seed(src[0] * 100 + dst[1])
    x, y = torch.randn(2, 3, *src, generator=g), torch.randn(2, 3, *dst, generator=g)
    got = _lib.upsample_add(x.to(DEV), y.to(DEV))
    assert got.shape == y.shape and got.dtype == torch.float32
    want = F.interpolate(x.double(), size=dst, mode='bilinear', align_corners=True) + y.double()
    bound = 4 * EPS * (F.interpolate(x.double().abs(), size=dst, mode='bilinear', align_corners=True) + y.double().abs())
    cpu32 = F.interpolate(x, size=dst, mode='bilinear', align_corners=True) + y
    within(f'upsample_add {src} -> {dst}', 'y', got, want, bound, yardstick=(cpu32, 0.0))
    if src == dst:
        assert torch.equal(got.cpu(), x + y)
    if src == (5, 5):                                                            # exact taps: the even outputs are x + y, the odd ones midpoints
        assert torch.equal(got.cpu()[:, :, ::2, ::2], x + y[:, :, ::2, ::2])


# ------------------------------------------------------------------------------------------- 5. the codes
@pytest.mark.parametrize('B,Ns,Np,D,T', [(3, 5, 4, 64, 4), (2, 14, 16, 512, 16)])
@pytest.mark.parametrize('avg', [True, False], ids=['avg', 'bare'])
def test_psp_codes_against_fp64(B, Ns, Np, D, T, avg):
    """within (Ns + 3) 2^-24 of the sum of magnitudes; a batch of one gives the same bits"""
    from transeditor_amd import _lib
    g = torch.Generator().manual_seed(B * 1000 + Ns)
    lat, A, bz = torch.randn(B, Ns + Np, D, generator=g), torch.randn(T, Ns, generator=g) * Ns ** -0.5, torch.randn(T, generator=g)
    za, pa = (torch.randn(D, T, generator=g), torch.randn(D, Np, generator=g)) if avg else (None, None)
    dev = lambda t: None if t is None else t.to(DEV)
    z, p = _lib.psp_codes(dev(lat), dev(A), dev(bz), Np, dev(za), dev(pa))
    assert z.shape == (B, D, T) and p.shape == (B, D, Np)
    l64 = lat.double()
    z64 = (l64[:, :Ns].permute(0, 2, 1) @ A.double().t()) + bz.double()
    zm = (l64[:, :Ns].abs().permute(0, 2, 1) @ A.double().abs().t()) + bz.double().abs()
    p64, pm = l64[:, Ns:].permute(0, 2, 1), l64[:, Ns:].abs().permute(0, 2, 1)
    if avg:
        z64, zm, p64, pm = z64 + za.double(), zm + za.double().abs(), p64 + pa.double(), pm + pa.double().abs()
    within(f'psp_codes B={B} Ns={Ns} Np={Np} D={D} T={T} avg={avg}', 'z', z, z64, (Ns + 3) * EPS * zm)
    within(f'psp_codes B={B} Ns={Ns} Np={Np} D={D} T={T} avg={avg}', 'p', p, p64, (Ns + 3) * EPS * pm)
    if not avg:
        assert torch.equal(p.cpu(), lat[:, Ns:].permute(0, 2, 1))
    z1, p1 = _lib.psp_codes(dev(lat[1:2].contiguous()), dev(A), dev(bz), Np, dev(za), dev(pa))
    assert torch.equal(z1, z[1:2]) and torch.equal(p1, p[1:2])


# ------------------------------------------------------------------------------------------- 6. end to end, small geometry
E2E_CASES = [True, False]                                 # with and without squeeze-and-excitation
E2E_B = 3


@pytest.fixture(scope='module')
def e2e():
    """per case: the encoder, the images, the library's codes, the fp64 restatement and the yardstick = rel_l2 of the SAME restatement
    run by torch in fp32 against fp64.  Computed once, shared and never modified."""
    from transeditor_amd.psp_encoder import DualSpaceEncoder
    G, out = P.SMALL, {}
    for se in E2E_CASES:
        x = R.images(211, E2E_B, G['S'])
        sd = P.small_state_dict(6, images=x, se=se)
        enc = DualSpaceEncoder(state_dict=sd, taps=G['taps'], units=G['units'])
        z64, p64 = P.encode(x, sd, torch.float64, G['units'], G['taps'])
        z32, p32 = P.encode(x, sd, torch.float32, G['units'], G['taps'])
        z, p = enc.encode(x.to(DEV))
        out[se] = dict(enc=enc, x=x.to(DEV), sd=sd, z=z, p=p, z64=z64, p64=p64, yard=(rel_l2(z32, z64), rel_l2(p32, p64)))
    return out


@pytest.mark.parametrize('se', E2E_CASES, ids=['ir_se', 'ir'])
def test_encoder_end_to_end(e2e, se):
    """Bar: 4 x the error of the fp32 torch restatement (batch norms unfolded) on the same inputs, on the rel_l2 of each code, the
    project's convention.  Non-degeneracy is asserted on the fp64 restatement: the codes of different images differ by at least 100 x the
    bar.  A batch of one gives the same bits."""
    d, G = e2e[se], P.SMALL
    enc = d['enc']
    assert enc.units == tuple(G['units']) and enc.se == (se,) * 3 and (enc.dim, enc.n_styles, enc.n_spatials, enc.tokens, enc.depth) == (64, 5, 4, 4, 2)
    assert enc.geometry['counts'] == G['styles'] and len(enc.program) == 7 and enc.z_avg is None and not enc.from_plus_space
    assert d['z'].shape == (E2E_B, 64, 4) and d['p'].shape == (E2E_B, 64, 4) and d['z'].is_cuda and d['z'].dtype == torch.float32
    for name, got, want, yard in (('z', d['z'], d['z64'], d['yard'][0]), ('p', d['p'], d['p64'], d['yard'][1])):
        e = rel_l2(got, want)
        far = min(rel_l2(want[i], want[j]) for i in range(E2E_B) for j in range(E2E_B) if i != j)
        print(f'DualSpaceEncoder small geometry se={se}: {name}_code library {e:.3e}, torch fp32 {yard:.3e}, ratio {e / yard:.2f}; '
              f'images differ by {far:.3f} = {far / (4 * yard):.0f} x the bar')
        assert far >= 100 * 4 * yard
        assert e <= 4 * yard
    z1, p1 = enc.encode(d['x'][1:2].contiguous())
    assert torch.equal(z1, d['z'][1:2]) and torch.equal(p1, d['p'][1:2])
    with pytest.raises(ValueError, match='a 48 px image'):
        enc.encode(torch.zeros(1, 3, 48, 48, device=DEV))
    with pytest.raises(RuntimeError, match='needs a GPU'):
        enc.encode(torch.zeros(1, 3, 32, 32))


def test_invert_and_edit_sweep():
    """invert through a small generator returns the image the generator gives for those codes, and edit_sweep takes the codes"""
    from transeditor_amd import edit, synth
    from transeditor_amd.inference import GeneratorSampler
    from transeditor_amd.model_spatial_query import Generator
    from transeditor_amd.psp_encoder import DualSpaceEncoder
    G = P.SMALL
    sd = P.state_dict(8, units=G['units'], taps=G['taps'], D=512, styles=(1, 1, 1), spatials=16, tokens=16, depth=2, reduction=4)
    gen = Generator(32, 512, 512, 8, n_trans=8, pixel_norm_op_dim=1)
    gsd = gen.state_dict()
    synth.fill_state_dict(gsd, 21)
    gen.load_state_dict(gsd)
    sampler = GeneratorSampler(gen.to(DEV))
    x = R.images(31, 2, 32).to(DEV)
    bare = DualSpaceEncoder(state_dict=sd, taps=G['taps'], units=G['units']).encode(x)
    for plus in (True, False):
        enc = DualSpaceEncoder(state_dict=P.checkpoint(sd, plus=plus, averages=True), taps=G['taps'], units=G['units'])
        assert enc.from_plus_space == plus and enc.z_avg.shape == (512, 16)
        img, z, p = enc.invert(sampler, x)
        assert z.shape == (2, 512, 16) and p.shape == (2, 512, 16) and img.shape == (2, 3, 32, 32)
        kw = dict(use_style_mapping=False, use_spatial_mapping=False) if plus else {}
        assert torch.equal(img, sampler(z, p, **kw)[0])
        assert rel_l2(z - enc.z_avg, bare[0]) < 1e-5 and rel_l2(p - enc.p_avg, bare[1]) < 1e-5
    big = enc.invert(sampler, x, resize=True)[0]
    assert big.shape == (2, 3, 256, 256)
    zb = torch.randn(1, 512, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = edit.edit_sweep(sampler, z, p, zb / zb.norm(), zb / zb.norm(), z_distance=1.0, p_distance=1.0, steps=3, batch=4)
    assert set(out) == {'p', 'z', 'pz'} and out['pz'].shape == (2, 3, 3, 32, 32)


# ------------------------------------------------------------------------------------------- 7. the true geometry
@pytest.fixture(scope='module')
def true_geometry():
    """GradualStyleEncoder(50, 'ir_se') at 256 px: the 364.7 M weights are drawn from the golden seed once, the SE calibration factors
    are the golden file's (tools/psp_encoder_golden.py found them in fp64)"""
    from transeditor_amd.psp_encoder import DualSpaceEncoder
    z, G = load_golden('psp_encoder_ref'), P.GOLDEN
    sd = P.state_dict(G['seed'], fc2_scale=z['fc2_scale'].tolist())
    shapes = {k: tuple(t.shape) for k, t in sd.items()}
    enc = DualSpaceEncoder(state_dict=sd)
    del sd
    x = R.images(G['image_seed'], G['B'], G['S']).to(DEV)
    zc, pc = enc.encode(x)
    return dict(z=zc.cpu(), p=pc.cpu(), enc=enc, shapes=shapes)


def test_true_geometry_against_the_reference(true_geometry):
    """tests/golden/psp_encoder_ref.npz (tools/psp_encoder_golden.py): the codes the reference's own GradualStyleEncoder(50, 'ir_se')
    returns in fp32 on the CPU for these weights and this image, and the fp64 restatement's.  The yardstick is the reference's rel_l2
    against fp64; the library is held to 4 x it against fp64 and to 5 x it against the reference (ArcFace's rule).  The keys
    DualSpaceEncoder reads are the reference class's.  Measured on the MI355X: ratios 3.44 (z) and 3.46 (p); profiles/README.md,
    'Encoder inversion'."""
    from transeditor_amd.arcface import default_units
    z, G, d = load_golden('psp_encoder_ref'), P.GOLDEN, true_geometry
    assert [int(z[k]) for k in ('seed', 'image_seed', 'B', 'S')] == [G[k] for k in ('seed', 'image_seed', 'B', 'S')]
    enc = d['enc']
    assert list(enc.units) == default_units() and all(enc.se) and (enc.dim, enc.n_styles, enc.n_spatials, enc.tokens, enc.depth) == (512, 14, 16, 16, 4)
    assert enc.geometry['counts'] == (3, 4, 7) and len(enc.program) + 1 == 10    # ten launches for 138 convolutions and 30 linears
    ref_shapes = {str(k): tuple(int(v) for v in str(s).split(',') if v) for k, s in zip(z['keys'], z['shapes'])}
    assert ref_shapes == d['shapes']                                           # the synthetic state dict IS the reference class's layout
    assert set(enc.keys) == {k for k in ref_shapes if not k.endswith('num_batches_tracked')}
    for name in ('z', 'p'):
        ref, f64 = z[name], z[name + '64']
        yard = rel_l2(ref, f64)
        e, e_vs_ref = rel_l2(d[name], f64), rel_l2(d[name], ref)
        print(f'DualSpaceEncoder at 256 px: {name}_code library {e:.3e}, the reference {yard:.3e} (rel_l2 against fp64), ratio {e / yard:.2f}; '
              f'library against the reference {e_vs_ref:.3e}')
        assert e <= 4 * yard
        assert e_vs_ref <= 5 * yard

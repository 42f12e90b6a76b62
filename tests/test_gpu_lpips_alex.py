"""The AlexNet LPIPS diversity score on the GPU (transeditor_amd.lpips_alex, metrics.evaluate_diversity; metrics/lpips.py:49-82,
metrics/evaluate_query.py:82-133): te_alex_stem_fwd_f32 elementwise against fp64, te_lpips_unit_f32 and the all-pairs head against the
fp64 restatement of tests/lpips_alex_restated.py with the fp32 restatement as the yardstick, the head's bitwise properties, the whole
scorer against what the reference's own class returned (tests/golden/lpips_alex_ref.npz), and evaluate_diversity / the command line
end to end on a 32 px generator.

Accuracy bar of a set of pair values, rel_l2 over the upper triangle against fp64: max(4 x yardstick, 2^-20), the yardstick being the
same formula in plain fp32 torch on the CPU for the same inputs (for the golden case: the reference's own values).  4 x is the margin
every scorer of this suite uses; the floor is 16 ulp: a term passes at most eight roundings before it is summed.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_alex_restated as R
from conftest import ROOT
from fp64_check import SENTINEL, U32 as EPS, kink_keep, within

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FLOOR = 2.0 ** -20
K = 363


def _bar(yard):
    return max(4 * yard, FLOOR)


# ------------------------------------------------------------------------------------------------------------------ the stem
STEM_CASES = [(2, 11, 13, 64),          # Ho = 2: padding on every side of every window
              (3, 33, 30, 72),          # a ragged channel block (72 = 64 + 8), floor in the stride (30 + 4 - 11 = 23 = 5 * 4 + 3)
              (1, 256, 256, 64)]        # the true geometry: 63 x 63


def _stem_case(case):
    """images tanh(randn), w ~ N(0, 1), biases of scale 4 sqrt(K) as test_gpu_pose._res_case draws them (few pre-activations near 0)"""
    N, H, W, Co = case
    g = torch.Generator().manual_seed(sum(p * v for p, v in zip((3, 5, 7, 11), case)))
    x = torch.tanh(torch.randn(N, 3, H, W, generator=g))
    return x, torch.randn(Co, 3, 11, 11, generator=g), torch.randn(Co, generator=g) * 4 * K ** 0.5


@pytest.fixture(scope='module')
def stem_refs():
    """per case: the inputs, the fp64 pre-activation, the elementwise bound and torch's own fp32 result on the CPU; computed once"""
    out = {}
    for case in STEM_CASES:
        x, w, b = _stem_case(case)
        s64 = R.scale(x, torch.float64)
        pre = F.conv2d(s64, w.double(), b.double(), stride=4, padding=2)
        bound = (K + 8) * EPS * F.conv2d(s64.abs(), w.double().abs(), b.double().abs(), stride=4, padding=2)
        cpu32 = F.conv2d(R.scale(x, torch.float32), w, b, stride=4, padding=2)
        out[case] = dict(x=x, w=w, b=b, pre=pre, bound=bound, cpu32=cpu32)
    return out


@pytest.mark.parametrize('case', STEM_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_stem_against_fp64(stem_refs, case):
    """|out - out64| <= (K + 8) 2^-24 (|w| * |s(x)| + |b|), K = 363: test_gpu_pose.py's K + S + 3 with S = 1 plus up to four roundings
    for the scaling.  Elements whose fp64 pre-activation lies within the bound of 0 are left out, at most fp64_check.KINK_CAP = 0.1 %;
    torch's fp32 CPU result meets the bound on the same elements.  The share is a property of the seeded operands and the fp64
    reference: none of 512, 1 of 9072 (1.1e-4) and 16 of 254016 (6.3e-5) elements in the three cases."""
    from transeditor_amd import _lib
    N, H, W, Co = case
    d = stem_refs[case]
    out = _lib.alex_stem_fwd(d['x'].to(DEV), d['w'].to(DEV), d['b'].to(DEV))
    assert out.shape == d['pre'].shape == (N, Co, (H - 7) // 4 + 1, (W - 7) // 4 + 1) and out.dtype == torch.float32 and out.is_contiguous()
    pre, bound = d['pre'], d['bound']
    keep = kink_keep(pre, bound)
    want = torch.relu(pre)
    print(f'alex stem {case}: positive {float((want > 0).double().mean()):.2f}')
    within(f'alex stem {case}', 'y', out, want, bound, keep, yardstick=(torch.relu(d['cpu32']), 0.001))
    assert bool((out.cpu()[~keep] >= 0).all())


def test_stem_nan_pixel_reaches_its_windows():
    from transeditor_amd import _lib
    x, w, b = _stem_case((1, 43, 40, 64))
    w, b = w.to(DEV), b.to(DEV)
    clean = _lib.alex_stem_fwd(x.to(DEV), w, b).cpu()
    py, px = 18, 22
    x[0, 1, py, px] = float('nan')
    y = _lib.alex_stem_fwd(x.to(DEV), w, b).cpu()
    Ho, Wo = clean.shape[2:]
    assert (Ho, Wo) == (10, 9)
    oy, ox = torch.arange(Ho).view(-1, 1), torch.arange(Wo).view(1, -1)
    hit = ((4 * oy - 2 <= py) & (py <= 4 * oy + 8) & (4 * ox - 2 <= px) & (px <= 4 * ox + 8)).expand(1, 64, Ho, Wo)
    assert int(hit[0, 0].sum()) == 3 * 3                                       # rows 3 ... 5 (4 oy in [10, 20]), columns 4 ... 6 (4 ox in [14, 24])
    assert torch.equal(y.isnan(), hit)                                         # all channels: no weight is exactly 0
    assert torch.equal(y[~hit], clean[~hit])


def test_stem_is_independent_of_the_batch_and_the_tile():
    """17 images of 256 px are 67 473 output pixels, which the 128-pixel tile takes; one image alone runs on the 64-pixel tile"""
    from transeditor_amd import _lib
    _, w, b = _stem_case(STEM_CASES[2])
    w, b = w.to(DEV), b.to(DEV)
    x = R.images(9, 17, 256).to(DEV)
    full = _lib.alex_stem_fwd(x, w, b)
    assert torch.equal(full, _lib.alex_stem_fwd(x, w, b))                      # two runs
    for i in (0, 8, 16):
        assert torch.equal(full[i:i + 1], _lib.alex_stem_fwd(x[i:i + 1].contiguous(), w, b))
    assert torch.equal(full[5:9], _lib.alex_stem_fwd(x[5:9].contiguous(), w, b))
    assert float((full > 0).float().mean()) > 0.2


def test_stem_refusals_launch_nothing():
    from transeditor_amd import _lib
    L = _lib.lib()
    w, b = torch.zeros(8, 3, 11, 11, device=DEV), torch.zeros(8, device=DEV)
    x = torch.zeros(1, 3, 40, 40, device=DEV)
    out = torch.full((1, 8, 9, 9), SENTINEL, device=DEV)
    st = _lib._stream()

    def call(N, H, W, Co=8, o=out.data_ptr(), xi=x.data_ptr(), wi=w.data_ptr(), bi=b.data_ptr()):
        return L.te_alex_stem_fwd_f32(o, xi, wi, bi, N, H, W, Co, st)
    for N, H, W in [(0, 40, 40), (-1, 40, 40), (65536, 40, 40), (1, 0, 40), (1, 40, -1), (1, 6, 40), (1, 40, 6), (1, 32768, 32768)]:
        assert call(N, H, W) == -2, (N, H, W)
    assert call(1, 40, 40, Co=0) == -2 and call(1, 40, 40, Co=-3) == -2
    for null in ('o', 'xi', 'wi', 'bi'):
        assert call(1, 40, 40, **{null: None}) == -1
    with pytest.raises(RuntimeError, match='te_alex_stem_fwd_f32 failed'):
        _lib.alex_stem_fwd(torch.zeros(1, 3, 6, 40, device=DEV), w, b)
    with pytest.raises(RuntimeError, match='inconsistent shapes'):
        _lib.alex_stem_fwd(x, torch.zeros(8, 3, 7, 7, device=DEV), b)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call(1, 40, 40) == 0                                                # (the same call with good sizes does write)
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# --------------------------------------------------------------------------------------------- normalisation and all-pairs head
HEAD_CASES = [(2, 5, 1), (3, 64, 9),
              (9, 192, 300),            # ragged against the 8-image tile and the 256-pixel block; six channel slices
              (40, 64, 3969)]           # the real layer 1 of a group of 40 at 256 px


def _taps(case, signed=False):
    """relu(randn) with pixels 3, 10, 17, ... of every image zero on all channels; a head in [0, 0.1) or, signed, in [-0.025, 0.075)"""
    N, C, HW = case
    g = torch.Generator().manual_seed(1000 * N + 10 * C + HW + (5 if signed else 0))
    f = torch.relu(torch.randn(N, C, HW, generator=g))
    f[:, :, 3::7] = 0
    return f, (torch.rand(C, generator=g) - (0.25 if signed else 0.0)) * 0.1


def _pairs_gpu(f, w):
    from transeditor_amd import _lib
    fh = _lib.lpips_unit(f.to(DEV))
    return _lib.lpips_allpairs_dist([_lib.lpips_allpairs_fwd(fh, w.to(DEV))], [f.shape[1:]], f.shape[0])


@pytest.mark.parametrize('case', HEAD_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_unit_normalisation(case):
    """f * rsqrt(sum_c f^2 + 1e-10): the sum is exact to fp32 (fp64), rsqrt is rounded once, the product once: 2 roundings, held to 3 ulp
    of the value.  A pixel that is zero on every channel gives exactly 0; in place is the same bits."""
    from transeditor_amd import _lib
    f, _ = _taps(case)
    want = R.unit(f.double())
    fd = f.to(DEV)
    out = _lib.lpips_unit(fd)
    assert out.shape == f.shape and torch.equal(fd.cpu(), f)                    # the input is untouched
    got = out.cpu()
    assert bool((got[:, :, 3::7] == 0).all()) and bool((want[:, :, 3::7] == 0).all())
    err = (got.double() - want).abs()
    print(f'unit {case}: max err / value ulp {float((err / (want.abs() * EPS + 1e-300)).max()):.3f}')
    assert bool((err <= 3 * EPS * want.abs()).all())
    assert _lib.lpips_unit(fd, out=fd) is fd and torch.equal(fd, out)
    f4 = f.view(case[0], case[1], 1, case[2]).to(DEV)                           # [N,C,H,W] is taken as well
    assert torch.equal(_lib.lpips_unit(f4).view_as(out), out)


@pytest.fixture(scope='module')
def head_refs():
    """per (case, signed): the taps, the head, the fp64 matrix and the fp32 restatement's; computed once"""
    out = {}
    for case, signed in [(c, False) for c in HEAD_CASES] + [(HEAD_CASES[2], True)]:
        f, w = _taps(case, signed)
        out[case, signed] = dict(f=f, w=w, D64=R.head_pairwise(R.unit(f.double()), w.double()), D32=R.head_pairwise(R.unit(f), w))
    return out


@pytest.mark.parametrize('case,signed', [(c, False) for c in HEAD_CASES] + [(HEAD_CASES[2], True)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else ('signed' if v else 'nonneg'))
def test_allpairs_head_against_fp64(head_refs, case, signed):
    d = head_refs[case, signed]
    N = case[0]
    D = _pairs_gpu(d['f'], d['w']).cpu()
    assert D.shape == (N, N) and D.dtype == torch.float32
    assert bool((D.diagonal() == 0).all()) and torch.equal(D, D.t())
    if signed:
        assert float(d['w'].min()) < -0.01
    if N == 1:
        return
    ref = R.triu(d['D64'])
    e, yard = R.rel_l2(R.triu(D), ref), R.rel_l2(R.triu(d['D32']), ref)
    print(f'all-pairs head {case}{" signed" if signed else ""}: library {e:.3e}, fp32 restatement {yard:.3e}, ratio to the bar '
          f'{e / _bar(yard):.3f} (bar {_bar(yard):.3e})')
    assert e <= _bar(yard)


def test_allpairs_head_of_one_image():
    f, w = _taps((1, 7, 70))
    assert _pairs_gpu(f, w).cpu().tolist() == [[0.0]]


def test_allpairs_head_is_independent_of_the_group(head_refs):
    """D[i,j] of a group of 9 (two image tiles) and of its sub-groups agree bit for bit, whichever tile and slot the two images land in"""
    d = head_refs[HEAD_CASES[2], False]
    f, w = d['f'], d['w']
    D = _pairs_gpu(f, w).cpu()
    assert torch.equal(D, _pairs_gpu(f, w).cpu())                              # two runs
    for sub in ([1, 4, 8], [8, 0], [7, 8, 2, 3, 5]):
        assert torch.equal(_pairs_gpu(f[sub].contiguous(), w).cpu(), D[sub][:, sub]), sub
    big = head_refs[HEAD_CASES[3], False]
    sub = [39, 0, 17, 8, 31]
    assert torch.equal(_pairs_gpu(big['f'][sub].contiguous(), big['w']).cpu(), _pairs_gpu(big['f'], big['w']).cpu()[sub][:, sub])


def test_allpairs_head_identical_images_and_nan(head_refs):
    d = head_refs[HEAD_CASES[2], True]                                          # the signed head: nothing relies on w >= 0
    f, w = d['f'].clone(), d['w']
    clean = _pairs_gpu(f, w).cpu()
    f[6] = f[2]                                                                 # D(x, x) == 0 across slots, and across tiles
    f[8] = f[2]
    D = _pairs_gpu(f, w).cpu()
    assert D[2, 6] == 0 and D[6, 2] == 0 and D[2, 8] == 0 and D[6, 8] == 0 and bool((D.diagonal() == 0).all())
    assert torch.equal(D[6], D[2]) and torch.equal(D[:, 8], D[:, 2]) and torch.equal(D[:6, :6], clean[:6, :6])
    f = d['f'].clone()
    f[4, 100, 17] = float('nan')                                                # a NaN tap: its pixel's norm, hence all 192 channels there
    D = _pairs_gpu(f, w).cpu()
    hit = torch.zeros(9, 9, dtype=torch.bool)
    hit[4, :] = True
    hit[:, 4] = True
    assert torch.equal(D.isnan(), hit) and torch.equal(D[~hit], clean[~hit])


def test_layers_are_added_in_order(head_refs):
    """te_lpips_allpairs_dist_f32 adds the layers' means as the reference's `lpips_value +=` does: ((m0 + m1) + m2), in fp32"""
    from transeditor_amd import _lib
    parts, shapes, single = [], [], []
    for case in HEAD_CASES[:3]:
        f, w = _taps((9,) + case[1:])
        fh = _lib.lpips_unit(f.to(DEV))
        parts.append(_lib.lpips_allpairs_fwd(fh, w.to(DEV)))
        shapes.append(case[1:])
        single.append(_lib.lpips_allpairs_dist(parts[-1:], shapes[-1:], 9))
    D = _lib.lpips_allpairs_dist(parts, shapes, 9)
    assert torch.equal(D, (single[0] + single[1]) + single[2]) and torch.equal(D, D.t())
    with pytest.raises(RuntimeError, match='are not those of a group'):         # partials of another shape are not read
        _lib.lpips_allpairs_dist(parts[:1], [(64, 9)], 9)
    with pytest.raises(RuntimeError, match='inconsistent shapes'):
        _lib.lpips_allpairs_fwd(torch.zeros(2, 5, 4, device=DEV), torch.zeros(4, device=DEV))


# ------------------------------------------------------------------------------------------------------------ the whole scorer
@pytest.fixture(scope='module')
def golden_ref():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'lpips_alex_ref.npz'))


@pytest.fixture(scope='module')
def scorer(golden_ref):
    """true widths, the seeded convolution weights of the golden file and the reference's own heads"""
    from transeditor_amd.lpips_alex import AlexLPIPS
    sd = R.state_dict(R.GOLDEN['seed'])
    lin = {f'lpips_weights.{l}.main.1.weight': torch.from_numpy(golden_ref[f'lin{l}']).view(1, -1, 1, 1) for l in range(5)}
    return dict(sd=sd, lin=lin, lp=AlexLPIPS(state_dict=sd, lin_state_dict=lin))


def _check_pairs(name, D, d64, yard):
    """the rel_l2 bar, and every pair's value inside the Cauchy-Schwarz bar |dD_ij| <= |dD|_2 <= bar |D64|_2"""
    got = R.triu(D.cpu())
    e, bar = R.rel_l2(got, d64), _bar(yard)
    worst = float((got.double() - d64).abs().max() / (bar * d64.norm()))
    print(f'AlexLPIPS {name}: library {e:.3e}, yardstick {yard:.3e}, ratio to the bar {e / bar:.3f} (bar {bar:.3e}); worst pair / its '
          f'bar {worst:.3f}; values {float(d64.min()):.4f} ... {float(d64.max()):.4f}')
    assert e <= bar and worst <= 1.0
    assert bool((D.diagonal() == 0).all()) and torch.equal(D, D.t())


def test_scorer_against_the_reference_class(scorer, golden_ref):
    """64 px, N = 6: the reference's own LPIPS in fp32 on the CPU is the yardstick"""
    G = R.GOLDEN
    x = R.images(G['image_seed'], G['N'], G['S'])
    d_ref, d64 = torch.from_numpy(golden_ref['d_ref']), torch.from_numpy(golden_ref['d64'])
    yard = R.rel_l2(d_ref, d64)
    D = scorer['lp'].pairwise(x.to(DEV))
    assert D.shape == (6, 6) and D.dtype == torch.float32 and D.is_cuda
    _check_pairs('64 px N=6 (golden)', D, d64, yard)
    assert R.rel_l2(R.triu(D.cpu()), d_ref) <= _bar(yard) + yard                # against the reference's values: the triangle inequality
    assert scorer['lp'].widths == R.WIDTHS


@pytest.mark.parametrize('N,S', [(5, 67), (3, 256)])
def test_scorer_against_fp64(scorer, N, S):
    x = R.images(S + N, N, S)
    d64 = R.triu(R.pairwise(x, scorer['sd'], scorer['lin'], torch.float64))
    yard = R.rel_l2(R.triu(R.pairwise(x, scorer['sd'], scorer['lin'], torch.float32)), d64)
    _check_pairs(f'{S} px N={N}', scorer['lp'].pairwise(x.to(DEV)), d64, yard)


def test_scorer_methods_and_input_checks(scorer):
    lp = scorer['lp']
    x = R.images(3, 6, 40, 52).to(DEV)                                          # not square
    D = lp.pairwise(x)
    assert torch.equal(D, lp.pairwise(x))                                       # two runs
    assert torch.equal(lp.pairwise(x[[4, 1]].contiguous()), D[[4, 1]][:, [4, 1]])        # a pair's value does not depend on its group
    gm = lp.group_mean(x)
    assert gm.ndim == 0 and gm.is_cuda
    assert abs(float(gm) - float(R.triu(D.cpu()).double().mean())) <= 16 * EPS * float(gm)          # 15 positive terms and a division
    d = lp(x[:3], x[3:])                                                        # LPIPS.forward on batches: the mean of the paired distances
    assert d.ndim == 0 and float(d) == float(torch.stack([D[0, 3], D[1, 4], D[2, 5]]).mean())
    assert float(lp(x[1], x[5])) == float(D[1, 5]) and float(lp(x[2], x[2])) == 0.0
    small = lp.pairwise(R.images(4, 2, 32).to(DEV))                             # 32 px: planes of 7, 3, 1, 1, 1
    assert small.shape == (2, 2) and bool(small.isfinite().all()) and float(small[0, 1]) > 0
    with pytest.raises(ValueError, match='at least 7'):
        lp.pairwise(torch.zeros(2, 3, 6, 32, device=DEV))
    with pytest.raises(ValueError, match='max pool'):
        lp.pairwise(torch.zeros(2, 3, 20, 32, device=DEV))
    with pytest.raises(ValueError, match='at least 2 images'):
        lp.group_mean(x[:1])
    with pytest.raises(ValueError, match=r'\[N,3,H,W\]'):
        lp.pairwise(torch.zeros(2, 4, 32, 32, device=DEV))
    with pytest.raises(RuntimeError, match='AlexLPIPS needs a GPU'):
        lp.pairwise(torch.zeros(2, 3, 32, 32))


# ------------------------------------------------------------------------------------------- evaluate_diversity and the command line
SIZE = 32


@pytest.fixture(scope='module')
def tiny(tmp_path_factory, scorer):
    from transeditor_amd import synth
    from transeditor_amd.model_spatial_query import Generator
    G = Generator(SIZE, 512, 512, 2 * (int(np.log2(SIZE)) - 1), n_trans=8, pixel_norm_op_dim=1)
    sd = G.state_dict()
    synth.fill_state_dict(sd, 11)
    G.load_state_dict(sd)
    tmp = tmp_path_factory.mktemp('lpips_alex')
    torch.save({'g_ema': sd}, str(tmp / '7.pt'))
    torch.save(scorer['sd'], str(tmp / 'alexnet.pth'))
    torch.save(scorer['lin'], str(tmp / 'lpips_weights.ckpt'))
    return dict(G=G.to(DEV), tmp=tmp)


def test_evaluate_diversity_end_to_end(tiny, scorer):
    from transeditor_amd import metrics
    from transeditor_amd.inference import GeneratorSampler
    calls = []

    class Spy(GeneratorSampler):
        def __call__(self, style, op_param, **kw):
            out = super().__call__(style, op_param, **kw)
            calls.append((style.clone(), op_param.clone(), out[0].clone()))
            return out
    s, lp = Spy(tiny['G']), scorer['lp']
    a = metrics.evaluate_diversity(s, lp, n_iter=2, group=5, seed=1)
    first = list(calls)
    b = metrics.evaluate_diversity(s, lp, n_iter=2, group=5, seed=1)
    assert all(a[k] == b[k] and np.array_equal(a['per_iteration'][k], b['per_iteration'][k]) for k in ('all', 'same_p', 'same_z'))
    assert len(first) == 6 and all(img.shape == (5, 3, SIZE, SIZE) for _, _, img in first)
    for n, (z, p, _) in enumerate(first):
        same_p, same_z = bool((p == p[:1]).all()), bool((z == z[:1]).all())
        assert (same_p, same_z) == [(False, False), (True, False), (False, True)][n % 3], n
    # the figures against the restatement applied to the images the sampler produced
    names = [n for n, _, _ in metrics.DIVERSITY_GROUPS]
    d64 = [R.triu(R.pairwise(img, scorer['sd'], scorer['lin'], torch.float64)) for _, _, img in first]
    d32 = [R.triu(R.pairwise(img, scorer['sd'], scorer['lin'], torch.float32)) for _, _, img in first]
    lib = [R.triu(lp.pairwise(img).cpu()) for _, _, img in first]
    yard = R.rel_l2(torch.cat(d32), torch.cat(d64))
    e, bar = R.rel_l2(torch.cat(lib), torch.cat(d64)), _bar(yard)
    print(f'evaluate_diversity 32 px: pairs library {e:.3e}, yardstick {yard:.3e}, ratio to the bar {e / bar:.3f}; figures '
          f'{ {k: round(a[k], 6) for k in names} }')
    assert e <= bar
    for k, name in enumerate(names):
        v64 = torch.cat(d64[k::3])                                              # both iterations' pairs of this group
        want = float(torch.stack([d64[k].mean(), d64[k + 3].mean()]).mean())
        # |mean error| <= |error|_2 / sqrt(n) <= bar * rms(d64) (Cauchy-Schwarz), plus the fp32 means' own roundings (10 + 2 terms)
        tol = bar * float(v64.pow(2).mean().sqrt()) + 16 * EPS * abs(want)
        assert abs(a[name] - want) <= tol, (name, a[name], want, tol)
        assert a['per_iteration'][name].shape == (2,) and a['per_iteration'][name].dtype == np.float32
    assert a['same_p'] != a['all'] and a['same_z'] != a['all']
    assert metrics.evaluate_diversity(s, lp, n_iter=1, group=5, seed=2)['all'] != a['all']


def test_cli_prints_one_line_with_the_three_figures(tiny, capsys):
    from transeditor_amd import metrics
    tmp = tiny['tmp']
    capsys.readouterr()
    argv = ['--ckpt', str(tmp / '7.pt'), '--size', str(SIZE), '--lpips', '--alexnet', str(tmp / 'alexnet.pth'), '--lpips_alex_lin',
            str(tmp / 'lpips_weights.ckpt'), '--lpips_iters', '2', '--lpips_group', '5', '--seed', '1']
    res = metrics.main(argv)
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 1 and lines == res
    line = lines[0]
    assert line['metric'] == 'lpips_diversity' and line['ckpt'].endswith('7.pt') and (line['n_iter'], line['group']) == (2, 5)
    assert {'all', 'same_p', 'same_z'} <= set(line) and all(isinstance(line[k], float) and 0 < line[k] < 2 for k in ('all', 'same_p', 'same_z'))
    assert metrics.main(argv) == res                                            # seeded: the same figures bit for bit

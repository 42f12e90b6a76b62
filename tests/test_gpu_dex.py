"""The DEX age / gender scorer (transeditor_amd.dex, csrc/dex.hip) against fp64 restatements (tests/dex_restated.py): the stem with the
preprocessing and the centre crop in it, the softmax / score head, the whole network on small geometries and on the true one (224 px
crop, 4096-wide fc layers, against what the reference's own classes return: tests/golden/dex_ref.npz), and the plumbing around it
(fit_boundaries, score_sweeps, the input checks)."""
import pytest
import torch
import torch.nn.functional as F

import dex_restated as R
import scorer_checks
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ---------------------------------------------------------------------------------------------------------- 1. the stem
STEM_CASES = [(2, 40, 40, 32), (1, 64, 64, 64), (3, 48, 80, 32), (1, 50, 50, 36), (1, 256, 256, 224)]
#              equal offsets    offset 0         unequal offsets  ragged last block  the real geometry


def _stem_weights(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(64, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5 / 128, torch.randn(64, generator=g) * 0.05


def _stem_input(N, H, W, crop, seed):
    """1.5 * randn (a good half of the pixels are clamped) and, in rows 1 ... of image 0's window, the 255 values (k + 0.5) / 255 * 2 - 1
    in all three channels: each maps to k + 0.5 up to rounding, next to a tie of the final round()"""
    x = 1.5 * torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(seed))
    ties = ((torch.arange(255, dtype=torch.float32) + 0.5) / 255 * 2 - 1)
    y0, x0 = (H - crop) // 2, (W - crop) // 2
    k = torch.arange(255)
    x[0, :, y0 + 1 + k // crop, x0 + k % crop] = ties
    return x


@pytest.mark.parametrize('N,H,W,crop', STEM_CASES)
def test_stem_against_fp64(N, H, W, crop):
    """rel_l2 < 1e-6, the bar of test_gpu_vgg_features.py::test_vgg_stem_against_fp64 for the same 27-term fp32 chain: the inputs are
    integers, so one pixel rounded to the wrong side of a tie moves 64 outputs by a weight, about 1e-4 of the norm at these sizes."""
    from transeditor_amd import _lib
    w, b = _stem_weights(N + crop)
    x = _stem_input(N, H, W, crop, 3 * H + W)
    y = _lib.dex_stem_fwd(x.to(DEV), w.to(DEV), b.to(DEV), crop)
    ref = R.stem(x, w, b, crop, torch.float64)
    v = R.preprocess(x, crop)
    assert y.shape == (N, 64, crop, crop) and y.dtype == torch.float32
    assert float((v == 0).float().mean()) > 0.1 and float((v == 255).float().mean()) > 0.1        # the clamp is live on both sides
    e = rel_l2(y, ref)
    print(f'dex stem N={N} {H}x{W} crop {crop}: rel_l2 {e:.3e}')
    assert e < 1e-6
    assert float((y.double().cpu() - ref)[:, :, 0].abs().max()) < 1e-5 * float(ref.abs().max())      # first row (padding side)


@pytest.mark.parametrize('N,H,W,crop', [(2, 40, 40, 32), (1, 50, 50, 36)])       # the second: a ragged last block
def test_stem_is_the_vgg_stem_on_the_preprocessed_crop(N, H, W, crop):
    """te_dex_stem_fwd_f32 and te_vgg_stem_fwd_f32 are one kernel body with two input rules: the same 27-term chain on the same
    integers (the byte-level chain is torch's own bits by construction), so the outputs are bitwise equal."""
    from transeditor_amd import _lib
    w, b = _stem_weights(N + crop)
    x = _stem_input(N, H, W, crop, 3 * H + W)
    y = _lib.dex_stem_fwd(x.to(DEV), w.to(DEV), b.to(DEV), crop)
    assert torch.equal(y, _lib.vgg_stem_fwd(R.preprocess(x, crop).to(DEV), w.to(DEV), b.to(DEV)))


def test_stem_pads_the_crop_not_the_image():
    """the window holds -1 (level 0) everywhere and the image around it +5 (clamped: level 255): every output is relu(bias) exactly,
    also next to the window's edge.  A tap that read the image outside the window would add 255 * w."""
    from transeditor_amd import _lib
    w, b = _stem_weights(1)
    x = torch.full((2, 3, 44, 52), 5.0)
    x[:, :, 6:38, 10:42] = -1.0
    y = _lib.dex_stem_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 32).cpu()
    assert torch.equal(y, torch.relu(b).view(1, 64, 1, 1).expand(2, 64, 32, 32))
    ref = R.stem(x, w, b, 32, torch.float64)
    assert rel_l2(y, ref) < 1e-6


def test_stem_nan_pixel_stays_local():
    from transeditor_amd import _lib
    w, b = _stem_weights(2)
    x = _stem_input(1, 40, 40, 32, 5)
    clean = R.stem(x, w, b, 32, torch.float64)
    x[0, 1, 4 + 10, 4 + 20] = float('nan')                                     # window position (10, 20) of image channel 1
    y = _lib.dex_stem_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 32).cpu()
    hit = torch.zeros(1, 64, 32, 32, dtype=torch.bool)
    hit[:, :, 9:12, 19:22] = True
    assert bool(torch.isnan(y[hit]).all())                                     # all 64 channels: no weight is exactly 0
    assert bool(torch.isfinite(y[~hit]).all())
    assert float((y.double() - clean)[~hit].norm() / clean[~hit].norm()) < 1e-6


def test_stem_refusals():
    from transeditor_amd import _lib
    L = _lib.lib()
    w, b = (t.to(DEV) for t in _stem_weights(3))
    x = torch.zeros(1, 3, 40, 40, device=DEV)
    out = torch.full((1, 64, 40, 40), 7.0, device=DEV)
    st = _lib._stream()

    def call(N, H, W, crop):
        return L.te_dex_stem_fwd_f32(out.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, crop, st)
    for N, H, W, crop in [(1, 40, 40, 0), (1, 40, 40, -2), (1, 40, 40, 42), (1, 30, 40, 32), (1, 40, 30, 32), (1, 40, 40, 33), (1, 41, 40, 32),
                          (1, 40, 41, 32), (65536, 40, 40, 32), (0, 40, 40, 32)]:
        assert call(N, H, W, crop) == -2, (N, H, W, crop)
    assert L.te_dex_stem_fwd_f32(out.data_ptr(), None, w.data_ptr(), b.data_ptr(), 1, 40, 40, 32, st) == -1
    with pytest.raises(RuntimeError, match='even'):
        _lib.dex_stem_fwd(x, w, b, 33)
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0                               # nothing was launched


# ---------------------------------------------------------------------------------------------------------- 2. the head
HEAD_CASES = [(1, 1, 4), (1, 2, 8), (3, 101, 4096), (5, 1024, 64), (65, 7, 260)]


def _head_case(I, C, K):
    """a ~ N(0, 1), w ~ N(0, 1 / K), bias 0.05 N(0, 1): logits that spread by about one"""
    g = torch.Generator().manual_seed(100 * I + C + K)
    return torch.randn(I, K, generator=g), torch.randn(C, K, generator=g) / K ** 0.5, torch.randn(C, generator=g) * 0.05


@pytest.fixture(scope='module')
def head_refs():
    """per case: the inputs, the fp64 probabilities and the yardstick (the same computation by fp32 torch on the CPU against fp64)"""
    out = {}
    for I, C, K in HEAD_CASES:
        a, w, b = _head_case(I, C, K)
        p64 = F.softmax(F.linear(a.double(), w.double(), b.double()), 1)
        p32 = F.softmax(F.linear(a, w, b), 1)
        out[(I, C, K)] = dict(a=a, w=w, b=b, p64=p64, yard=rel_l2(p32, p64))
    return out


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('I,C,K', HEAD_CASES)
def test_head_against_fp64(head_refs, I, C, K, mode):
    """prob: rel_l2 <= max(4 x yardstick, 1e-6), 1e-6 being the bar te_fc_stream_f32's rows are held to; score, per row:
    |d score| <= bar |weights|_2 |p64|_2 (Cauchy-Schwarz on the probability bar)"""
    from transeditor_amd import _lib
    d = head_refs[(I, C, K)]
    p64 = d['p64']
    if C >= 101:                                                               # conditions on the restatement: nothing saturates
        assert float(p64.max()) < 0.5
    elif C >= 2:
        assert float(p64.max()) < 0.95 and float(p64[:, 0].min()) > 1e-3
    score, prob = _lib.cls_score(d['a'].to(DEV), d['w'].to(DEV), d['b'].to(DEV), mode, want_prob=True)
    assert score.shape == (I,) and prob.shape == (I, C) and score.dtype == torch.float32 and prob.dtype == torch.float32
    attribute = 'age' if mode == 0 else 'gender'
    bar = max(4 * d['yard'], 1e-6)
    e = rel_l2(prob, p64)
    s64 = R.score_of(p64, attribute)
    es = (score.double().cpu() - s64).abs()
    sb = R.score_bar(bar, p64, attribute)
    print(f'cls_score I={I} C={C} K={K} mode={mode}: prob rel_l2 {e:.3e} (fp32 torch {d["yard"]:.3e}, bar {bar:.3e}); '
          f'score max err / bar {float((es / sb).max()):.3f}')
    assert e <= bar
    assert bool((es <= sb).all())
    assert torch.equal(_lib.cls_score(d['a'].to(DEV), d['w'].to(DEV), d['b'].to(DEV), mode), score)      # without prob: the same score


def test_head_rows_do_not_depend_on_the_batch(head_refs):
    from transeditor_amd import _lib
    d = head_refs[(65, 7, 260)]
    a, w, b = d['a'].to(DEV), d['w'].to(DEV), d['b'].to(DEV)
    for mode in (0, 1):
        s65, p65 = _lib.cls_score(a, w, b, mode, want_prob=True)
        s1, p1 = _lib.cls_score(a[:1].contiguous(), w, b, mode, want_prob=True)
        assert torch.equal(s65[:1], s1) and torch.equal(p65[:1], p1)
        s64, p64 = _lib.cls_score(a[64:].contiguous(), w, b, mode, want_prob=True)
        assert torch.equal(s65[64:], s64) and torch.equal(p65[64:], p64)
        assert torch.equal(_lib.cls_score(a, w, b, mode), s65)                 # two runs


def test_head_refusals():
    from transeditor_amd import _lib
    L = _lib.lib()
    a, w, b = torch.zeros(3 * 8 + 4, device=DEV), torch.zeros(1025 * 8, device=DEV), torch.zeros(1025, device=DEV)
    score = torch.full((3,), 7.0, device=DEV)
    st = _lib._stream()

    def call(I, C, K, mode, a_ptr=a.data_ptr(), w_ptr=w.data_ptr()):
        return L.te_cls_score_f32(score.data_ptr(), None, a_ptr, w_ptr, b.data_ptr(), I, C, K, mode, st)
    assert call(3, 0, 8, 0) == -2
    assert call(3, 1025, 8, 0) == -2
    assert call(3, 4, 6, 0) == -2
    assert call(3, 4, 0, 0) == -2
    assert call(0, 4, 8, 0) == -2
    assert call(3, 4, 8, 0, a_ptr=a.data_ptr() + 4) == -2                      # a misaligned a
    assert b'16-byte aligned' in L.te_last_error_string()
    assert call(3, 4, 8, 0, w_ptr=w.data_ptr() + 8) == -2
    assert call(3, 4, 8, 2) == -3
    assert call(3, 4, 8, -1) == -3
    assert L.te_cls_score_f32(None, None, a.data_ptr(), w.data_ptr(), b.data_ptr(), 3, 4, 8, 0, st) == -1
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        _lib.cls_score(a[1:25].view(3, 8), w[:32].view(4, 8), b[:4], 0)
    with pytest.raises(RuntimeError, match='te_cls_score_f32 failed'):
        _lib.cls_score(a[:18].view(3, 6), w[:24].view(4, 6), b[:4], 0)
    torch.cuda.synchronize()
    assert float((score - 7.0).abs().max()) == 0.0                             # nothing was launched


# ---------------------------------------------------------------------------------------------------------- 3. end to end, small
E2E_CASES = [(80, 64, (256, 192), 101, 5), (128, 96, (256, 192), 2, 3)]        # (S, crop, hidden, C, B): pool5 2 x 2 and 3 x 3


def _attribute(C):
    return 'age' if C == 101 else 'gender'


def _nondegenerate(p64, s64, attribute, bar):
    """conditions on the fp64 restatement (not on the library): nothing saturates and the rows are told apart far above the bar"""
    if attribute == 'age':
        assert float(p64.max()) < 0.5
    else:
        assert 0.05 < float(p64[:, 0].min()) and float(p64[:, 0].max()) < 0.95
    scorer_checks.rows_told_apart(s64, R.score_bar(bar, p64, attribute))


@pytest.fixture(scope='module')
def e2e():
    """per case: the scorer, the images, the library's probabilities and scores, the fp64 restatement and the yardstick = rel_l2 of the
    SAME restatement run by torch in fp32 against fp64.  Computed once, shared and never modified."""
    from transeditor_amd.dex import DEXScorer
    out = {}
    for S, crop, hidden, C, B in E2E_CASES:
        sd = R.state_dict(1, pool=crop // 32, hidden=hidden, classes=C)
        scorer = DEXScorer(state_dict=sd, attribute=_attribute(C))
        x = R.images(101, B, S)
        p64 = R.probabilities(x, sd, torch.float64)
        out[(S, crop, hidden, C, B)] = dict(scorer=scorer, x=x.to(DEV), prob=scorer.probabilities(x.to(DEV)), score=scorer(x.to(DEV)),
                                            p64=p64, yard=rel_l2(R.probabilities(x, sd, torch.float32), p64))
    return out


@pytest.mark.parametrize('S,crop,hidden,C,B', E2E_CASES)
def test_scorer_end_to_end(e2e, S, crop, hidden, C, B):
    """Bar: 4 x the error of the fp32 torch restatement on the same inputs, as test_gpu_vgg_features.py::test_features_end_to_end (the
    split convolution routes and the split-K sums reorder the additions).  Measured on the MI355X (library / fp32 torch): see
    profiles/README.md, 'DEX scorer'."""
    d = e2e[(S, crop, hidden, C, B)]
    scorer, attribute = d['scorer'], _attribute(C)
    assert (scorer.crop, scorer.pool, scorer.hidden, scorer.classes) == (crop, crop // 32, hidden, C)
    assert d['prob'].shape == (B, C) and d['score'].shape == (B,) and d['score'].dtype == torch.float32 and d['score'].is_cuda
    bar = 4 * d['yard']
    s64 = R.score_of(d['p64'], attribute)
    _nondegenerate(d['p64'], s64, attribute, bar)
    e = rel_l2(d['prob'], d['p64'])
    es, sb = (d['score'].double().cpu() - s64).abs(), R.score_bar(bar, d['p64'], attribute)
    print(f'DEXScorer {attribute} S={S} crop {crop} B={B}: library {e:.3e}, fp32 torch {d["yard"]:.3e} (rel_l2 of the probabilities against '
          f'fp64), ratio {e / d["yard"]:.2f}; score max err / bar {float((es / sb).max()):.3f}')
    assert e <= bar
    assert bool((es <= sb).all())
    p1, s1 = scorer.probabilities(d['x'][:1]), scorer(d['x'][:1])
    e1 = rel_l2(d['prob'][:1], p1)
    print(f'    first row of the batch against a batch of one: {e1:.3e}')
    assert e1 <= bar
    assert bool(((d['score'][:1] - s1).double().cpu().abs() <= R.score_bar(bar, d['p64'][:1], attribute)).all())


def test_preprocessed_path_matches(e2e):
    """what the drop-in hands over (BGR levels, uncropped) through te_vgg_stem_fwd_f32 against the fused stem on the RGB image"""
    d = e2e[E2E_CASES[0]]
    p = d['scorer'].probabilities(scorer_checks.levels(d['x'].cpu()).to(DEV), preprocessed=True)
    assert rel_l2(p, d['p64']) <= 4 * d['yard']


# ---------------------------------------------------------------------------------------------------------- 4. the true geometry
@pytest.fixture(scope='module')
def true_geometry():
    """the 224 px / 4096 / 4096 network for 101 and for 2 classes: the weights before cls are drawn once and shared"""
    from transeditor_amd.dex import DEXScorer
    G = R.GOLDEN
    sd_age, sd_gender = R.state_dict(G['seed'], classes=(101, 2))
    x = R.images(G['image_seed'], G['B'], G['S']).to(DEV)
    out = {}
    for attribute, sd in (('age', sd_age), ('gender', sd_gender)):
        scorer = DEXScorer(state_dict=sd, attribute=attribute)
        out[attribute] = dict(prob=scorer.probabilities(x).cpu(), score=scorer(x).cpu(), geometry=(scorer.crop, scorer.hidden, scorer.classes))
        del scorer
    return out


@pytest.mark.parametrize('attribute', ['age', 'gender'])
def test_true_geometry_against_the_reference(true_geometry, attribute):
    """tests/golden/dex_ref.npz (tools/dex_golden.py): the probabilities and scores the reference's own Age / Gender classes return in
    fp32 on the CPU for these weights and images, and the fp64 restatement's.  The yardstick is the reference's rel_l2 against fp64;
    the library is held to 4 x it against fp64, hence to 5 x it against the reference."""
    z = load_golden('dex_ref')
    G = R.GOLDEN
    assert [int(z[k]) for k in ('seed', 'image_seed', 'B', 'S')] == [G['seed'], G['image_seed'], G['B'], G['S']]
    d = true_geometry[attribute]
    assert d['geometry'] == (224, (4096, 4096), 101 if attribute == 'age' else 2)
    p_ref, p64, s_ref = z[f'{attribute}_prob'], z[f'{attribute}_prob64'], z[f'{attribute}_score']
    yard = rel_l2(p_ref, p64)
    bar = 4 * yard
    s64 = R.score_of(p64.double(), attribute)
    _nondegenerate(p64.double(), s64, attribute, bar)
    e, e_ref = rel_l2(d['prob'], p64), rel_l2(d['prob'], p_ref)
    es, sb = (d['score'].double() - s64).abs(), R.score_bar(bar, p64, attribute)
    print(f'DEXScorer {attribute}, 224 px crop of 256, 4096 / 4096: library {e:.3e}, the reference {yard:.3e} (rel_l2 of the probabilities '
          f'against fp64), ratio {e / yard:.2f}; library against the reference {e_ref:.3e}; score max err / bar {float((es / sb).max()):.3f}')
    assert e <= bar and e_ref <= 5 * yard
    assert bool((es <= sb).all())
    assert bool(((d['score'].double() - s_ref.double()).abs() <= 2 * sb).all())             # each within the bar of fp64 (DEX_REPORT.txt)


# ---------------------------------------------------------------------------------------------------------- 5. plumbing
@pytest.fixture(scope='module')
def generator():
    return scorer_checks.small_generator(DEV)


@pytest.fixture(scope='module')
def small_scorer():
    from transeditor_amd.dex import DEXScorer
    return DEXScorer(state_dict=R.state_dict(9, pool=1, hidden=(64, 48), classes=101), attribute='age')      # a 32 px crop


def test_fit_boundaries(generator, small_scorer):
    from transeditor_amd.dex import fit_boundaries
    scorer_checks.check_fit_boundaries(fit_boundaries, generator, small_scorer)


def test_score_sweeps_on_the_device(small_scorer):
    scorer_checks.check_score_sweeps('age', small_scorer, size=64, bitwise=False, in_unit_range=False)


def test_scorer_input_checks(small_scorer):
    scorer_checks.check_crop_scorer_inputs(small_scorer, 32)

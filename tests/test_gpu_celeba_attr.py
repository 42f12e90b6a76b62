"""The CelebA-HQ attribute scorer (transeditor_amd.celeba_attr, csrc/celeba_attr.hip) against fp64 restatements
(tests/celeba_attr_restated.py): the pool with its activation, the stem with the preprocessing and the box mean in it, the score head,
the whole network on every convolution route it takes and on two geometries against what the reference's own class returns
(tests/golden/celeba_attr_ref.npz), and the plumbing around it (score_sweeps, fit_boundaries, the drop-in, load_scorers)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import celeba_attr_restated as R
import scorer_checks
from conftest import ROOT, load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _poisoned(n):
    return torch.full((n,), 7.0, device=DEV)


# ---------------------------------------------------------------------------------------------------------- 1. the pool
POOL_CASES = [(3, 2, 2), (5, 8, 8), (2, 6, 10), (4, 16, 16), (2, 64, 64), (2, 256, 256)]
#             one window  W == 8    the scalar path                        the largest map of the network
# (the grid is not capped and no thread loops: there is no second trip to reach)


def _pool_input(planes, H, W):
    """randn: the four taps of nearly every window have both signs; the first window of plane 0 is (+3, -1 / -1, -2), whose mean is
    negative while the mean of its activated taps is positive"""
    x = torch.randn(1, planes, H, W, generator=torch.Generator().manual_seed(planes + 10 * H + W))
    x[0, 0, 0, 0], x[0, 0, 0, 1], x[0, 0, 1, 0], x[0, 0, 1, 1] = 3.0, -1.0, -1.0, -2.0
    return x


@pytest.mark.parametrize('slope', [0.2, 1.0])
@pytest.mark.parametrize('planes,H,W', POOL_CASES)
def test_pool_against_fp64(planes, H, W, slope):
    from transeditor_amd import _lib
    x = _pool_input(planes, H, W)
    y = _lib.avgpool2_act(x.to(DEV), slope)
    ref = F.leaky_relu(F.avg_pool2d(x.double(), 2, 2), slope)
    mixed = (F.max_pool2d(x, 2, 2) > 0) & (-F.max_pool2d(-x, 2, 2) < 0)
    assert float(mixed.float().mean()) > 0.5                                   # the activation acts on means of taps of both signs
    assert y.shape == (1, planes, H // 2, W // 2) and y.dtype == torch.float32
    e = rel_l2(y, ref)
    print(f'avgpool2_act {planes} x {H} x {W} slope {slope}: rel_l2 {e:.3e}')
    assert e < 1e-6
    first = float(y[0, 0, 0, 0])
    assert first == float(torch.tensor(-0.25) * torch.tensor(slope))           # act(mean), not mean(act): that would be +0.55 at 0.2
    if slope == 1.0:
        assert rel_l2(y, F.avg_pool2d(x.double(), 2, 2)) < 1e-6                # the plain pool


def test_pool_misaligned_operands_take_the_scalar_path():
    """a contiguous view one float into its storage is not 16-byte aligned: same values, bit for bit"""
    from transeditor_amd import _lib
    x = _pool_input(4, 16, 16).to(DEV)
    want = _lib.avgpool2_act(x, 0.2)
    store = torch.zeros(x.numel() + 1, device=DEV)
    store[1:] = x.flatten()
    xm = store[1:].view(x.shape)
    assert xm.data_ptr() % 16 == 4 and xm.is_contiguous()
    assert torch.equal(_lib.avgpool2_act(xm, 0.2), want)


@pytest.mark.parametrize('planes,H,W', [(5, 8, 8), (2, 6, 10)])
def test_pool_nan_tap_stays_local(planes, H, W):
    from transeditor_amd import _lib
    x = _pool_input(planes, H, W)
    x[0, 1, 3, 5] = float('nan')
    for slope in (0.2, 1.0):
        y = _lib.avgpool2_act(x.to(DEV), slope).cpu()
        hit = torch.zeros_like(y, dtype=torch.bool)
        hit[0, 1, 1, 2] = True
        assert bool(torch.isnan(y[hit]).all()) and bool(torch.isfinite(y[~hit]).all())
        ref = F.leaky_relu(F.avg_pool2d(x.double(), 2, 2), slope)
        assert float((y.double() - ref)[~hit].abs().max()) < 1e-6


def test_pool_refusals():
    from transeditor_amd import _lib
    L = _lib.lib()
    x, out, st = torch.zeros(4 * 8 * 8, device=DEV), _poisoned(4 * 8 * 8), _lib._stream()
    for planes, H, W in [(4, 7, 8), (4, 8, 7), (0, 8, 8), (-1, 8, 8), (4, 0, 8), (4, 8, 0)]:
        assert L.te_avgpool2_act_f32(out.data_ptr(), x.data_ptr(), planes, H, W, 0.2, st) == -2, (planes, H, W)
    assert b'even' in L.te_last_error_string()
    assert L.te_avgpool2_act_f32(None, x.data_ptr(), 4, 8, 8, 0.2, st) == -1
    assert L.te_avgpool2_act_f32(out.data_ptr(), None, 4, 8, 8, 0.2, st) == -1
    with pytest.raises(RuntimeError, match='te_avgpool2_act_f32 failed'):
        _lib.avgpool2_act(torch.zeros(1, 2, 6, 5, device=DEV), 0.2)
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0                               # nothing was launched


# ---------------------------------------------------------------------------------------------------------- 2. the stem
STEM_CASES = [(2, 16, 16, 16), (1, 64, 32, 32), (1, 64, 16, 24), (3, 256, 256, 64), (3, 8, 8, 512)]
#              f = 1            f = 2            f = 4, ragged C0  the real geometry   the widest stem required


def _stem_weights(C0, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C0, 3, generator=g) * (2.0 / 3) ** 0.5, torch.randn(C0, generator=g)


def _stem_input(N, S, seed):
    """1.5 * randn (half of the pixels are clamped) and, from row 1 of image 0 on, in all three channels, the values
    (k + 0.5) / 255 * 2 - 1, k = 0 ... 254, as many as fit: each maps to k + 0.5 up to rounding, next to a tie of the final round()"""
    x = 1.5 * torch.randn(N, 3, S, S, generator=torch.Generator().manual_seed(seed))
    k = torch.arange(min(255, S * S - S))
    x[0].view(3, -1)[:, S + k] = ((k.float() + 0.5) / 255 * 2 - 1)
    return x


@pytest.mark.parametrize('N,S,R_,C0', STEM_CASES)
def test_stem_against_fp64(N, S, R_, C0):
    """rel_l2 < 1e-6 against fp64 of torch's own fp32 preprocessing: the byte levels are integers and so are the sums of the f x f
    blocks, so only the three-term product chain rounds; a pixel rounded to the wrong side of a tie would move C0 outputs by a weight"""
    from transeditor_amd import _lib
    w, b = _stem_weights(C0, N + S + C0)
    x = _stem_input(N, S, 3 * S + R_)
    v = R.preprocess(x)
    assert float((v == 0).float().mean()) > 0.1 and float((v == 255).float().mean()) > 0.1        # the clamp is live on both sides
    y = _lib.attr_stem_fwd(x.to(DEV), w.to(DEV), b.to(DEV), R_)
    ref = R.stem(x, w, b, R_, torch.float64)
    assert y.shape == (N, C0, R_, R_) and y.dtype == torch.float32
    e = rel_l2(y, ref)
    print(f'attr stem N={N} S={S} R={R_} C0={C0}: rel_l2 {e:.3e}')
    assert e < 1e-6
    assert float(ref.min()) < 0 < float(ref.max())                                                # both sides of the leaky ReLU
    yp = _lib.attr_stem_fwd(v.to(DEV), w.to(DEV), b.to(DEV), R_, preprocessed=True)                # the pre-flipped byte image
    assert torch.equal(yp, y)


def test_stem_reads_bgr():
    """a weight matrix that reads channel 0 only sees the image's BLUE plane (the network's input is BGR)"""
    from transeditor_amd import _lib
    x = _stem_input(2, 16, 7)
    w, b = torch.zeros(4, 3), torch.zeros(4)
    w[:, 0] = 1.0
    y = _lib.attr_stem_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 16).cpu()
    blue = x[:, 2].clamp(-1, 1).add(1).div(2).mul(255).round()
    assert torch.equal(y[:, 0], blue) and torch.equal(y[:, 3], blue)
    assert not torch.equal(blue, x[:, 0].clamp(-1, 1).add(1).div(2).mul(255).round())


def test_stem_averages_byte_levels_not_the_raw_image():
    """f = 2.  The block (-1, -1, 1, 0.2) has the levels (0, 0, 255, 153), mean 102; its raw mean -0.2 maps to level 102 as well (the
    map is affine where nothing is clamped or rounded), so a second block, (-3, -1, 1, 0.2), tells the two orders apart: the same
    levels and mean 102, against level 38 of its raw mean -0.7."""
    from transeditor_amd import _lib
    x = torch.zeros(1, 3, 4, 4)
    x[0, :, 0:2, 0:2] = torch.tensor([[-1.0, -1.0], [1.0, 0.2]])
    x[0, :, 0:2, 2:4] = torch.tensor([[-3.0, -1.0], [1.0, 0.2]])
    w, b = torch.eye(3), torch.zeros(3)
    y = _lib.attr_stem_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 2).cpu()
    assert y[0, :, 0, 0].tolist() == [102.0] * 3 and y[0, :, 0, 1].tolist() == [102.0] * 3
    assert y[0, :, 1, 0].tolist() == [128.0] * 3                               # 0 -> 127.5 -> level 128 (ties to even)
    assert rel_l2(y, R.stem(x, w, b, 2, torch.float64)) < 1e-6


def test_stem_nan_pixel_stays_local():
    from transeditor_amd import _lib
    w, b = _stem_weights(32, 2)
    x = _stem_input(1, 64, 5)
    clean = R.stem(x, w, b, 32, torch.float64)
    x[0, 1, 10, 21] = float('nan')                                             # block (5, 10) of image channel 1
    for pre in (False, True):
        xin = R.preprocess(x) if pre else x
        y = _lib.attr_stem_fwd(xin.to(DEV), w.to(DEV), b.to(DEV), 32, preprocessed=pre).cpu()
        hit = torch.zeros(1, 32, 32, 32, dtype=torch.bool)
        hit[:, :, 5, 10] = True
        assert bool(torch.isnan(y[hit]).all())                                 # all 32 channels: no weight is exactly 0
        assert bool(torch.isfinite(y[~hit]).all())
        assert float((y.double() - clean)[~hit].norm() / clean[~hit].norm()) < 1e-6


def test_stem_refusals():
    from transeditor_amd import _lib
    L = _lib.lib()
    w, b = torch.zeros(1025 * 3, device=DEV), torch.zeros(1025, device=DEV)
    x = torch.zeros(3 * 64 * 64, device=DEV)
    out, st = _poisoned(16 * 64 * 64), _lib._stream()

    def call(N, S, R_, C0, pre=0):
        return L.te_attr_stem_fwd_f32(out.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), N, S, R_, C0, pre, st)
    for N, S, R_, C0 in [(1, 48, 32, 16), (1, 16, 32, 16), (1, 0, 32, 16), (1, 64, 0, 16), (1, -64, -32, 16), (1, 64, 32, 0), (1, 64, 32, 1025),
                         (0, 64, 32, 16), (65536, 64, 32, 16)]:
        assert call(N, S, R_, C0) == -2, (N, S, R_, C0)
    assert call(1, 64, 32, 16, pre=2) == -3 and call(1, 64, 32, 16, pre=-1) == -3
    assert L.te_attr_stem_fwd_f32(out.data_ptr(), None, w.data_ptr(), b.data_ptr(), 1, 64, 32, 16, 0, st) == -1
    assert L.te_attr_stem_fwd_f32(None, x.data_ptr(), w.data_ptr(), b.data_ptr(), 1, 64, 32, 16, 0, st) == -1
    with pytest.raises(RuntimeError, match='multiple of the resolution'):
        _lib.attr_stem_fwd(x.view(1, 3, 64, 64), w[:48].view(16, 3), b[:16], 48)
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0                               # nothing was launched


# ---------------------------------------------------------------------------------------------------------- 3. the score head
HEAD_CASES = [(1, 4), (3, 64), (5, 512), (65, 260)]


def _head_case(I, K):
    """a ~ N(0, 1), w ~ N(0, 1 / K), bias 0.05 N(0, 1): logits of order one half"""
    g = torch.Generator().manual_seed(100 * I + K)
    return torch.randn(I, K, generator=g), torch.randn(K, generator=g) / K ** 0.5, torch.randn(1, generator=g) * 0.05


def _head_logit(a, w, b, dtype):
    return F.leaky_relu(a.to(dtype), 0.2) @ w.to(dtype) + b.to(dtype)


def _score_bar(bar, l64):
    """|d score| <= 0.5 |d logit| (d s / d l = -2 s (1 - s)), every |d logit| <= the L2 bar on the batch; 1e-7 for the score's own
    rounding"""
    return 0.5 * bar * float(l64.double().norm()) + 1e-7


@pytest.fixture(scope='module')
def head_refs():
    """per case: the inputs, the fp64 logits and the yardstick (the same computation by fp32 torch on the CPU against fp64)"""
    out = {}
    for I, K in HEAD_CASES:
        a, w, b = _head_case(I, K)
        l64 = _head_logit(a, w, b, torch.float64)
        out[(I, K)] = dict(a=a, w=w, b=b, l64=l64, yard=rel_l2(_head_logit(a, w, b, torch.float32), l64))
    return out


@pytest.mark.parametrize('I,K', HEAD_CASES)
def test_head_against_fp64(head_refs, I, K):
    from transeditor_amd import _lib
    d = head_refs[(I, K)]
    a, w, b = d['a'].to(DEV), d['w'].to(DEV), d['b'].to(DEV)
    logit, score = _lib.attr_score(a, w, b, 0.2)
    assert logit.shape == (I,) and score.shape == (I,) and logit.dtype == torch.float32 and score.dtype == torch.float32
    bar = max(4 * d['yard'], 1e-6)
    e = rel_l2(logit, d['l64'])
    es = float((score.double().cpu() - R.score_of(d['l64'])).abs().max())
    print(f'attr_score I={I} K={K}: logit rel_l2 {e:.3e} (fp32 torch {d["yard"]:.3e}, bar {bar:.3e}); score max err {es:.3e} '
          f'(bar {_score_bar(bar, d["l64"]):.3e})')
    assert e <= bar
    assert es <= _score_bar(bar, d['l64'])
    only_l, none_s = _lib.attr_score(a, w, b, 0.2, want_score=False)
    none_l, only_s = _lib.attr_score(a, w, b, 0.2, want_logit=False)
    assert none_s is None and none_l is None and torch.equal(only_l, logit) and torch.equal(only_s, score)


def test_head_rows_do_not_depend_on_the_batch(head_refs):
    from transeditor_amd import _lib
    d = head_refs[(65, 260)]
    a, w, b = d['a'].to(DEV), d['w'].to(DEV), d['b'].to(DEV)
    l65, s65 = _lib.attr_score(a, w, b, 0.2)
    l1, s1 = _lib.attr_score(a[:1].contiguous(), w, b, 0.2)
    assert torch.equal(l65[:1], l1) and torch.equal(s65[:1], s1)
    l64, s64 = _lib.attr_score(a[64:].contiguous(), w, b, 0.2)
    assert torch.equal(l65[64:], l64) and torch.equal(s65[64:], s64)


def test_head_large_logits_and_nan_rows():
    """logits of exactly +-50 give exactly 0 / 1 (the score decreases in the logit), +-40 the fp64 value, infinities 0 / 1; a NaN row
    gives NaN there only"""
    from transeditor_amd import _lib
    a = torch.tensor([[12.5] * 4, [-12.5] * 4, [10.0] * 4, [-10.0] * 4, [float('inf')] * 4, [-float('inf')] * 4, [1.0, float('nan'), 1.0, 1.0],
                      [0.25] * 4])
    w, b = torch.ones(4), torch.zeros(1)
    logit, score = (t.cpu() for t in _lib.attr_score(a.to(DEV), w.to(DEV), b.to(DEV), 1.0))
    assert logit[:4].tolist() == [50.0, -50.0, 40.0, -40.0]
    assert score[0].item() == 0.0 and score[1].item() == 1.0
    assert abs(score[2].item() / float(R.score_of(torch.tensor([40.0], dtype=torch.float64))) - 1) < 1e-5 and score[3].item() == 1.0
    assert score[4].item() == 0.0 and score[5].item() == 1.0
    assert bool(torch.isnan(logit[6])) and bool(torch.isnan(score[6]))
    assert logit[7].item() == 1.0 and abs(score[7].item() - 1 / (1 + np.exp(2.0))) < 1e-7
    assert bool(torch.isfinite(score[[0, 1, 2, 3, 4, 5, 7]]).all())


def test_head_refusals():
    from transeditor_amd import _lib
    L = _lib.lib()
    a, w, b = torch.zeros(3 * 8 + 4, device=DEV), torch.zeros(16, device=DEV), torch.zeros(1, device=DEV)
    logit, score, st = _poisoned(3), _poisoned(3), _lib._stream()

    def call(I, K, a_ptr=a.data_ptr(), w_ptr=w.data_ptr()):
        return L.te_attr_score_f32(logit.data_ptr(), score.data_ptr(), a_ptr, w_ptr, b.data_ptr(), I, K, 0.2, st)
    assert call(3, 6) == -2 and call(3, 0) == -2 and call(3, -4) == -2 and call(0, 8) == -2
    assert call(3, 8, a_ptr=a.data_ptr() + 4) == -2
    assert b'16-byte aligned' in L.te_last_error_string()
    assert call(3, 8, w_ptr=w.data_ptr() + 8) == -2
    assert L.te_attr_score_f32(None, None, a.data_ptr(), w.data_ptr(), b.data_ptr(), 3, 8, 0.2, st) == -1
    assert L.te_attr_score_f32(logit.data_ptr(), None, None, w.data_ptr(), b.data_ptr(), 3, 8, 0.2, st) == -1
    assert L.te_attr_score_f32(logit.data_ptr(), None, a.data_ptr(), w.data_ptr(), None, 3, 8, 0.2, st) == -1
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        _lib.attr_score(a[1:25].view(3, 8), w[:8], b)
    with pytest.raises(RuntimeError, match='te_attr_score_f32 failed'):
        _lib.attr_score(a[:18].view(3, 6), w[:6], b)
    torch.cuda.synchronize()
    assert float((logit - 7.0).abs().max()) == 0.0 and float((score - 7.0).abs().max()) == 0.0   # nothing was launched


# ---------------------------------------------------------------------------------------------------------- 4. the whole network
@pytest.fixture(scope='module')
def networks():
    """per case of celeba_attr_restated.CASES: the scorer, the images, the library's logits and scores.  The three r64 cases share
    one scorer (one state dict).  Computed once, shared and never modified."""
    from transeditor_amd.celeba_attr import CelebAAttributeScorer
    out, scorers = {}, {}
    for name, c in R.CASES.items():
        key = (c['R'], c['fmap_base'], c['fmap_max'], c['seed'])
        if key not in scorers:
            scorers[key] = CelebAAttributeScorer(state_dict=R.case_state_dict(c), name=name)
        x = R.case_images(c).to(DEV)
        out[name] = dict(scorer=scorers[key], x=x, logit=scorers[key].logits(x), score=scorers[key](x))
    return out


def _expected_routes(name):
    """{map size: convolution kind} the case is meant to cover.  The W == 16 form of TE_CONV_3X3W6 needs an even batch and at least
    128 blocks, which 128 channels reach at a batch of 64: r16w6 covers it, the small batches at R = 64 stay on TE_CONV_3X3 at 16 px."""
    from transeditor_amd import _lib
    if name == 'r16':
        return {16: _lib.CONV_3X3, 8: _lib.CONV_3X3, 4: _lib.CONV_3X3}
    if name == 'r16w6':
        return {16: _lib.CONV_3X3W6, 8: _lib.CONV_3X3, 4: _lib.CONV_3X3}
    return {64: _lib.CONV_3X3W6, 32: _lib.CONV_3X3W6, 16: _lib.CONV_3X3, 8: _lib.CONV_3X3, 4: _lib.CONV_3X3}


@pytest.mark.parametrize('name', list(R.CASES))
def test_network_against_the_fp64_restatement(networks, name):
    """Bar on the logits over the batch: rel_l2 <= max(4 x yardstick, 1e-6), the yardstick being the restatement run by torch in fp32
    on the CPU against fp64 (the margin of the DEX network tests); scores to 0.5 x the absolute logit bar + 1e-7.  Measured on the
    MI355X: profiles/README.md, 'CelebA-HQ attribute scorer'."""
    c, d = R.CASES[name], networks[name]
    scorer = d['scorer']
    l64, l32 = R.case_reference(name)
    R.conditions(l64, R.case_images(c))
    want = _expected_routes(name)
    routes = scorer.conv_routes(c['B'])
    assert len(routes) == scorer.n_convs and {H for H, _ in routes} == set(want)
    assert all(kind == want[H] for H, kind in routes), routes                  # (modconv.fwd_kinds: what forward() launches)
    assert scorer.resolution == c['R'] and d['logit'].shape == (c['B'],) and d['score'].dtype == torch.float32 and d['score'].is_cuda
    yard = rel_l2(l32, l64)
    bar = max(4 * yard, 1e-6)
    e = rel_l2(d['logit'], l64)
    es = float((d['score'].double().cpu() - R.score_of(l64)).abs().max())
    print(f'CelebAAttributeScorer {name} R={c["R"]} S={c["S"]} B={c["B"]}: library {e:.3e}, fp32 torch {yard:.3e} (rel_l2 of the logits against '
          f'fp64), ratio {e / yard:.2f}, bar {bar:.3e}; score max err {es:.3e} (bar {_score_bar(bar, l64):.3e})')
    assert e <= bar
    assert es <= _score_bar(bar, l64)


def test_preprocessed_path_matches(networks):
    """what the drop-in hands over (BGR levels, not yet averaged down) against the fused preprocessing: the same bits"""
    d = networks['r64s128']
    v = R.preprocess(d['x'].cpu()).to(DEV)
    assert torch.equal(d['scorer'].logits(v, preprocessed=True), d['logit'])
    assert torch.equal(d['scorer'](v, preprocessed=True), d['score'])


# ---------------------------------------------------------------------------------------------------------- 5. the golden vectors
@pytest.fixture(scope='module')
def golden_runs():
    from transeditor_amd.celeba_attr import CelebAAttributeScorer
    out = {}
    for name, c in R.GOLDEN.items():
        scorer = CelebAAttributeScorer(state_dict=R.case_state_dict(c), name=name)
        x = R.case_images(c).to(DEV)
        out[name] = dict(logit=scorer.logits(x).cpu(), score=scorer(x).cpu(), geometry=(scorer.resolution, scorer.channels))
        del scorer
    return out


@pytest.mark.parametrize('name', list(R.GOLDEN))
def test_against_the_reference(golden_runs, name):
    """tests/golden/celeba_attr_ref.npz (tools/celeba_attr_golden.py): the logits and scores the reference's own D returns in fp32 on
    the CPU for these weights and images, and the fp64 restatement's logits.  The yardstick is the reference's rel_l2 against fp64; the
    library is held to max(4 x it, 1e-6) against fp64, hence to that plus the yardstick against the reference."""
    z, c, d = load_golden('celeba_attr_ref'), R.GOLDEN[name], golden_runs[name]
    assert {k: int(z[f'{name}_{k}']) for k in c} == c
    chans = {'small': (16, 16, 32, 32, 64, 64, 64, 64), 'true': (64, 64, 128, 128, 256, 256, 512) + (512,) * 7}[name]
    assert d['geometry'] == (c['R'], chans)
    l_ref, s_ref, l64 = z[f'{name}_logit'], z[f'{name}_score'], z[f'{name}_logit64']
    R.conditions(l64, R.case_images(c))
    yard = rel_l2(l_ref, l64)
    bar = max(4 * yard, 1e-6)
    e, e_ref = rel_l2(d['logit'], l64), rel_l2(d['logit'], l_ref)
    es = float((d['score'].double() - R.score_of(l64)).abs().max())
    print(f'CelebAAttributeScorer golden {name} R={c["R"]} B={c["B"]}: library {e:.3e}, the reference {yard:.3e} (rel_l2 of the logits against '
          f'fp64), ratio {e / yard:.2f}, bar {bar:.3e}; library against the reference {e_ref:.3e}; score max err {es:.3e} '
          f'(bar {_score_bar(bar, l64):.3e})')
    assert e <= bar and e_ref <= bar + yard
    assert es <= _score_bar(bar, l64)
    assert float((d['score'].double() - s_ref.double()).abs().max()) <= 2 * _score_bar(bar, l64)


# ---------------------------------------------------------------------------------------------------------- 6. plumbing
@pytest.fixture(scope='module')
def generator():
    return scorer_checks.small_generator(DEV)


def _small_sd(seed):
    return R.state_dict(seed, 16, fmap_base=128, fmap_max=32)


def test_score_sweeps_with_two_scorers(networks):
    from transeditor_amd.celeba_attr import CelebAAttributeScorer
    from transeditor_amd.edit_eval import score_sweeps
    scorers = {'first': networks['r16']['scorer'], 'second': CelebAAttributeScorer(state_dict=_small_sd(3), name='second')}
    g = torch.Generator().manual_seed(12)
    origin = R.images(20, 2, 32).to(DEV)
    sweeps = {k: (origin.unsqueeze(1) + 0.3 * torch.randn(2, 5, 3, 32, 32, generator=g).to(DEV)) for k in ('p', 'z')}
    res = score_sweeps(scorers, origin, sweeps, batch=4)                       # 10 images in batches of 4, 4 and 2
    assert set(res) == {'first', 'second'}
    for name, scorer in scorers.items():
        want = scorer(origin).cpu().numpy()
        for space in ('p', 'z'):
            got = res[name][space]
            assert got.shape == (2, 6) and got.dtype == np.float32
            assert np.array_equal(got[:, 2], want)                             # the origin, in the middle
            each = scorer(sweeps[space].flatten(0, 1)).view(2, 5).cpu().numpy()
            assert np.allclose(np.delete(got, 2, axis=1), each, rtol=1e-5, atol=1e-7)      # (another batch split: not bitwise)
    assert not np.array_equal(res['first']['p'], res['second']['p'])


def test_fit_boundaries(generator, networks):
    from transeditor_amd.dex import fit_boundaries
    scorer_checks.check_fit_boundaries(fit_boundaries, generator, networks['r16']['scorer'], score_range=(0.0, 1.0, True))   # 64 px images: f = 4


def test_dropin_and_load_scorers(tmp_path, monkeypatch, networks):
    """a directory in the reference's layout, <dir>/<attribute>/net_best.pth holding {'state_dict', 'epoch', 'valacc'}: the drop-in's
    eval / estimate_score (preprocessed images, with and without no_soft) and load_scorers read it"""
    from transeditor_amd.celeba_attr import load_scorers
    for name, seed in (('Smiling', R.CASES['r16']['seed']), ('Male', 3)):
        os.makedirs(tmp_path / name)
        torch.save({'state_dict': _small_sd(seed), 'epoch': 7, 'valacc': 0.9}, str(tmp_path / name / 'net_best.pth'))
    d = networks['r16']
    scorers = load_scorers(str(tmp_path), ['Smiling', 'Male'])
    assert list(scorers) == ['Smiling', 'Male'] and scorers['Male'].name == 'Male' and scorers['Smiling'].resolution == 16
    assert torch.equal(scorers['Smiling'](d['x']), d['score'])
    assert not torch.equal(scorers['Male'](d['x']), d['score'])
    sys.path.insert(0, os.path.join(ROOT, 'dropin'))
    names = ('celebahq_utils', 'celebahq_utils.dex')
    try:
        for n in names:
            sys.modules.pop(n, None)
        dex = importlib.import_module('celebahq_utils.dex')
        monkeypatch.setenv('TE_CELEBA_ATTR_DIR', str(tmp_path))
        classifier = dex.eval('Smiling')
        assert dex.eval('Smiling') is classifier
        v = R.preprocess(d['x'].cpu()).to(DEV)
        assert torch.equal(dex.estimate_score(classifier, v), d['score'])
        assert torch.equal(dex.estimate_score(classifier, v, no_soft=True), d['logit'])
        with pytest.raises(RuntimeError, match='Bangs'):
            dex.eval('Bangs')
    finally:
        sys.path.remove(os.path.join(ROOT, 'dropin'))
        for n in names:
            sys.modules.pop(n, None)


def test_scorer_input_checks(networks):
    scorer = networks['r16']['scorer']
    with pytest.raises(ValueError, match='square'):
        scorer(torch.zeros(1, 3, 32, 16, device=DEV))
    with pytest.raises(ValueError, match='multiple of the resolution 16'):
        scorer(torch.zeros(1, 3, 8, 8, device=DEV))
    with pytest.raises(ValueError, match='multiple of the resolution 16'):
        scorer(torch.zeros(1, 3, 24, 24, device=DEV))
    with pytest.raises(ValueError, match=r'\[B,3,S,S\]'):
        scorer(torch.zeros(1, 1, 16, 16, device=DEV))
    with pytest.raises(RuntimeError, match='needs a GPU'):
        scorer(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match='needs a GPU'):
        scorer.logits(torch.zeros(1, 3, 32, 32), preprocessed=True)
    assert scorer(torch.zeros(2, 3, 48, 48, device=DEV)).shape == (2,)        # f = 3

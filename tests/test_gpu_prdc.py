"""PRDC on the GPU (transeditor_amd.prdc over csrc/prdc.hip) against the fp64 restatement of metrics/prdc.py (tests/prdc_restated.py)
and the reference's own recorded output (tests/golden/prdc_ref.npz): exact on integer features at every tile edge, within the fp32
bound on Gaussian features, bit-identical from run to run, and end to end through evaluate_prdc and the command line."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prdc_restated as R
import scorer_checks

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEYS = ('precision', 'recall', 'density', 'coverage')
ARRAYS = ('rr2', 'rf2', 'col_count', 'row_any', 'row_min')


# ---------------------------------------------------------------------------------------------------------- (a) exact cases
# one below, at and above the 128 x 128 x 32 tile edge in N, M and K; the minimal N = k + 1; the longest K; every list length (2..16)
EXACT = [(4, 4, 1, 3), (2, 2, 2, 1), (127, 129, 31, 3), (128, 128, 32, 5), (129, 127, 33, 1), (257, 130, 100, 15), (130, 385, 64, 3),
         (16, 300, 4096, 3)]


def integer_features(N, M, D, seed):
    """integers in [-4, 4] as fp32: every norm, dot product and squared distance is an integer below 2^24, exact in any order.  Some real
    rows are copied into the fake set (d2 = 0 under the strict <) and some rows repeat inside each set (tied radii)."""
    rng = np.random.default_rng(seed)
    real = rng.integers(-4, 5, (N, D)).astype(np.float32)
    fake = rng.integers(-4, 5, (M, D)).astype(np.float32)
    if N >= 4:
        real[N - 1] = real[0]
        real[N // 2] = real[1]
    if M >= 4:
        fake[1] = fake[M - 1]
        fake[M // 2] = real[0]                               # also a real row, which real[N - 1] repeats
        fake[0] = real[N // 3]
    return real, fake


def check_exact(got, want):
    assert np.array_equal(got['rr2'].astype(np.float64), want['rr2'])
    assert np.array_equal(got['rf2'].astype(np.float64), want['rf2'])
    assert got['col_count'].dtype == np.int32 and np.array_equal(got['col_count'], want['col_count'])
    assert np.array_equal(got['row_any'] != 0, want['row_any'])
    assert np.array_equal(got['row_min'].astype(np.float64), want['row_min'])


@pytest.mark.parametrize('N,M,D,k', EXACT)
def test_exact_on_integer_features(N, M, D, k):
    from transeditor_amd import prdc
    real, fake = integer_features(N, M, D, 1000 * N + M + D + k)
    want = R.details(real, fake, k)
    assert float(want['d2'].max()) < 2 ** 24
    got = prdc.prdc_details(real, fake, k)
    check_exact(got, want)
    assert prdc.compute_prdc(torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV), k) == R.numbers(want, k)


def test_kernels_at_the_binding_level():
    """row_sqnorm / prdc_knn / prdc_counts one by one, on an unaligned view (the scalar load path at D % 4 == 0) and with radii that are
    not the sets' own: the counts follow whatever thresholds they are given"""
    from transeditor_amd import _lib
    real, fake = integer_features(70, 150, 8, 5)
    base = torch.zeros(70 * 8 + 1, device=DEV)
    x = base[1:].view(70, 8)                                 # 4-byte aligned only
    x.copy_(torch.from_numpy(real))
    y = torch.from_numpy(fake).to(DEV)
    nx, ny = _lib.row_sqnorm(x), _lib.row_sqnorm(y)
    assert np.array_equal(nx.cpu().numpy(), (real.astype(np.float64) ** 2).sum(1))
    assert np.array_equal(_lib.prdc_knn(x, nx, 2).cpu().numpy(), R.radii2(real, 2))
    rr2 = torch.full((70,), 40.0, device=DEV)
    rf2 = torch.arange(150, device=DEV, dtype=torch.float32)
    cc, ra, rm = _lib.prdc_counts(x, nx, rr2, y, ny, rf2)
    d2 = R.sq_distances(real, fake)
    assert np.array_equal(cc.cpu().numpy(), (d2 < 40.0).sum(0))
    assert np.array_equal(ra.cpu().numpy() != 0, (d2 < np.arange(150.0)[None, :]).any(1))
    assert np.array_equal(rm.cpu().numpy(), d2.min(1))
    with pytest.raises(RuntimeError):
        _lib.prdc_knn(x.double(), nx, 2)
    with pytest.raises(RuntimeError):
        _lib.prdc_knn(y.t(), ny, 2)
    with pytest.raises(RuntimeError):
        _lib.prdc_knn(x.cpu(), nx, 2)
    with pytest.raises(RuntimeError):
        _lib.prdc_knn(y[:3].contiguous(), ny[:3].contiguous(), 3)


# ---------------------------------------------------------------------------------------------------------- (b) real-valued cases
@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(GOLDEN, 'prdc_ref.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def kth(a, k):
    return np.sort(a, axis=1)[:, k]


@pytest.mark.parametrize('case', ['a', 'b'])
def test_gaussian_features_against_fp64_and_the_reference(golden, case):
    """Bound: every fp32 d2(i,j) lies within B(i,j) = 2e-6 (nx[i] + ny[j]) of fp64 (3.5e-7 sum|a b| for an fp32 fma chain at K <= 4096,
    three terms, 2.5x headroom).  An order statistic of values each within its own B lies between the same order statistic of d2 - B and
    of d2 + B, which is how the bound is applied to the radii and the row minimum.  The comparisons are then exact because, in fp64, no
    pair lies within a relative 1e-5 of its threshold (asserted first: a condition on the inputs)."""
    from transeditor_amd import prdc
    real, fake, k = golden[f'{case}_real'], golden[f'{case}_fake'], int(golden[f'{case}_k'])
    want = R.details(real, fake, k)
    gap = R.min_relative_gap(want)
    print(f'case {case}: smallest relative gap between a d2 and its threshold {gap:.2e}')
    assert gap > 1e-5
    got = prdc.prdc_details(real, fake, k)
    nx, ny = (real.astype(np.float64) ** 2).sum(1), (fake.astype(np.float64) ** 2).sum(1)
    for name, x, n_, in (('rr2', real, nx), ('rf2', fake, ny)):
        d = R.sq_distances(x, x)
        np.fill_diagonal(d, 0.0)
        B = 2e-6 * (n_[:, None] + n_[None, :])
        np.fill_diagonal(B, 0.0)
        lo, hi = kth(np.maximum(d - B, 0), k), kth(d + B, k)
        g = got[name].astype(np.float64)
        print(f'case {case} {name}: max |gpu - fp64| / (bound half-width) {float((np.abs(g - want[name]) / ((hi - lo) / 2)).max()):.3f}')
        assert np.all(lo <= g) and np.all(g <= hi)
    B = 2e-6 * (nx[:, None] + ny[None, :])
    g = got['row_min'].astype(np.float64)
    print(f'case {case} row_min: max relative error {float((np.abs(g - want["row_min"]) / want["row_min"]).max()):.2e}')
    assert np.all(np.maximum(want['d2'] - B, 0).min(1) <= g) and np.all(g <= (want['d2'] + B).min(1))
    assert np.array_equal(got['col_count'], want['col_count'])
    assert np.array_equal(got['row_any'] != 0, want['row_any'])
    res = prdc.compute_prdc(real, fake, k)
    ref = dict(zip(KEYS, golden[f'{case}_prdc']))
    n, m = real.shape[0], fake.shape[0]
    assert res['precision'] == ref['precision'] and res['recall'] == ref['recall'] and res['coverage'] == ref['coverage']
    assert round(res['density'] * k * m) == round(ref['density'] * k * m) and res == R.numbers(want, k)
    assert all(type(res[x]) is float for x in KEYS) and tuple(res) == KEYS


# ---------------------------------------------------------------------------------------------------------- (c) determinism
def test_two_runs_are_bit_identical():
    from transeditor_amd import prdc
    rng = np.random.default_rng(3)
    real = rng.standard_normal((257, 100)).astype(np.float32)
    fake = (0.9 * rng.standard_normal((130, 100)) + 0.1).astype(np.float32)
    a = prdc.prdc_details(real, fake, 15)
    b = prdc.prdc_details(real, fake, 15)
    for name in ARRAYS:
        assert a[name].tobytes() == b[name].tobytes(), name


# ---------------------------------------------------------------------------------------------------------- (d) end to end
def pooled(image):
    return F.adaptive_avg_pool2d(image, 8).flatten(1)


@pytest.fixture(scope='module')
def sampler():
    from transeditor_amd.inference import GeneratorSampler
    return GeneratorSampler(scorer_checks.small_generator(DEV, seed=21))


def test_evaluate_prdc_end_to_end(sampler):
    from transeditor_amd import prdc
    real = prdc.fake_features(sampler, pooled, n_sample=40, batch=16, seed=2)          # another draw of the same generator
    assert real.shape == (40, 192) and real.is_cuda
    state = torch.cuda.get_rng_state()
    res = prdc.evaluate_prdc(sampler, pooled, real, n_sample=48, batch=16, nearest_k=3, seed=1)
    assert torch.equal(state, torch.cuda.get_rng_state())                            # the seed idiom leaves the global state alone
    fake = prdc.fake_features(sampler, pooled, n_sample=48, batch=16, seed=1)
    assert fake.shape == (48, 192)
    want = R.details(real.cpu().numpy(), fake.cpu().numpy(), 3)
    assert R.min_relative_gap(want) > 1e-5
    assert res == R.numbers(want, 3)


def test_command_line(tmp_path, capsys, golden):
    from transeditor_amd import prdc
    rp, fp = str(tmp_path / 'real.npy'), str(tmp_path / 'fake.npy')
    np.save(rp, golden['b_real'])
    np.save(fp, golden['b_fake'])
    direct = prdc.compute_prdc(golden['b_real'], golden['b_fake'], 1)
    capsys.readouterr()
    prdc.main(['--real', rp, '--fake', fp, '--nearest_k', '1'])
    lines = [x for x in capsys.readouterr().out.splitlines() if x.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert {x: out[x] for x in KEYS} == direct
    assert out['metric'] == 'prdc' and out['nearest_k'] == 1 and out['n_real'] == 129 and out['n_fake'] == 67


# ---------------------------------------------------------------------------------------------------------- (e) workspace
def test_workspace_is_not_a_distance_matrix():
    from transeditor_amd import _lib
    nb = _lib.lib().te_prdc_ws_bytes(50000, 50000, 4096, 3)
    assert 0 < nb < 1 << 30

"""FID on the GPU (transeditor_amd.fid over csrc/fid.hip) against the fp64 restatement (tests/fid_restated.py) and the reference's own
recorded values (tests/golden/fid_ref.npz): the moments exact on integer features at every tile, fragment, k-step and split edge,
bit-exact where every product and sum is representable, within the fp64 summation bound on real-valued features, bit-identical from
run to run, and end to end through FeatureStats, evaluate_fid and the command line.

The kernel's edges: 64 x 64 tiles of S, 16-column fragments, slabs of 32 samples in k-steps of 4; the sample index is split (partials in
the workspace) whenever there are fewer than 2048 upper tiles (D < 4033) and more than one slab, and not split otherwise."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import fid_restated as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fid_ref.npz')
U = 2.0 ** -53
REF_RTOL = 10 * 1.00e-8            # tests/test_fid_cpu.py: 10 x the largest reference-against-fp64 gap tools/fid_golden.py printed
ONEPASS_B = 100 * 2.05e-9          # 100 x the one-pass-against-two-pass gap it printed for the rank-deficient case b


# ---------------------------------------------------------------------------------------------------------- helpers
def integer_features(N, D, seed):
    """integers in [-4, 4] as fp32, every column with a range and an offset of its own and no row a symmetric pattern: S is far from
    any matrix a row <-> column swap or a permuted fragment row would also produce"""
    rng = np.random.default_rng(seed)
    lo = -4 + (np.arange(D) % 4)
    hi = 4 - ((np.arange(D) // 4) % 3)
    x = rng.integers(lo, hi + 1, (N, D))
    x[:, ::7] = np.abs(x[:, ::7])
    return x.astype(np.float32)


def gpu_moments(x, accumulate=False, S=None, s=None):
    from transeditor_amd import _lib
    D = x.shape[1]
    S = torch.full((D, D), float('nan'), device=DEV, dtype=torch.float64) if S is None else S
    s = torch.full((D,), float('nan'), device=DEV, dtype=torch.float64) if s is None else s
    _lib.fid_moments(S, s, x if torch.is_tensor(x) else torch.from_numpy(x).to(DEV), accumulate)
    return S, s


def check_exact(x, S, s):
    xi = x.astype(np.float64)                               # small integers: every partial sum is an integer far below 2^53, exact
    assert np.array_equal(xi, np.round(xi)) and np.abs(xi).max() <= 4
    assert np.array_equal(s.cpu().numpy(), xi.sum(0))
    assert np.array_equal(np.triu(S.cpu().numpy()), np.triu(xi.T @ xi))


# ---------------------------------------------------------------------------------------------------------- (a) exact moments
EXACT = [(1, 1), (2, 3), (3, 16), (5, 17), (127, 33), (128, 128), (129, 129), (130, 257), (1000, 64), (4097, 48),
         (31, 63), (32, 64), (33, 65), (65, 15),            # the slab of 32 samples and the 64-wide tile, one below / at / above
         (70, 4036), (33, 4033)]                            # no split (2080 upper tiles), 16-byte and scalar loads, two slabs


@pytest.mark.parametrize('N,D', EXACT)
def test_exact_moments_on_integer_features(N, D):
    x = integer_features(N, D, 1000 * N + D)
    S, s = gpu_moments(x)
    check_exact(x, S, s)


def test_one_nonzero_column_against_a_ramp():
    """one sample k0 has a 1 in column c, every other column holds a ramp over (sample, column): row c and column c of S are then row k0
    of the ramp, so each element names the sample and the feature it came from"""
    N, D = 37, 70
    k, j = np.meshgrid(np.arange(N), np.arange(D), indexing='ij')
    for k0, c in ((0, 0), (5, 17), (33, 64), (36, 69), (2, 31)):
        x = ((j + 3 * k) % 9 - 4).astype(np.float32)
        x[:, c] = 0
        x[k0, c] = 1
        S, s = gpu_moments(x)
        check_exact(x, S, s)
        got = S.cpu().numpy()
        assert np.array_equal(got[c, c + 1:], x[k0, c + 1:]) and np.array_equal(got[:c, c], x[k0, :c]) and got[c, c] == 1


def test_products_are_exact_in_fp64():
    """features 1 + m 2^-23, 0 <= m < 256: a product has 47 significant bits and a sum of 16 of them 51, so S is exact in ANY order;
    a product or a partial sum rounded to fp32 anywhere cannot give these bits"""
    rng = np.random.default_rng(7)
    for N, D in ((16, 40), (13, 70)):
        x = (1.0 + rng.integers(0, 256, (N, D)) * 2.0 ** -23).astype(np.float32)
        x64 = x.astype(np.float64)
        assert np.array_equal(x64, 1.0 + np.round((x64 - 1.0) * 2.0 ** 23) * 2.0 ** -23)
        S, s = gpu_moments(x)
        want = np.zeros((D, D))
        for r in x64:                                        # exact whatever numpy's order: accumulate outer products
            want += np.outer(r, r)
        assert np.triu(S.cpu().numpy()).tobytes() == np.triu(want).tobytes()
        assert s.cpu().numpy().tobytes() == x64.sum(0).tobytes()


def test_unaligned_view_and_binding_checks():
    from transeditor_amd import _lib
    x = integer_features(70, 8, 5)
    base = torch.zeros(70 * 8 + 1, device=DEV)
    v = base[1:].view(70, 8)                                 # 4-byte aligned only: the scalar load path at D % 4 == 0
    v.copy_(torch.from_numpy(x))
    assert v.data_ptr() % 16 == 4
    S, s = gpu_moments(v)
    check_exact(x, S, s)
    y = torch.from_numpy(integer_features(24, 12, 6)).to(DEV)
    S = torch.zeros(12, 12, device=DEV, dtype=torch.float64)
    s = torch.zeros(12, device=DEV, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        _lib.fid_moments(S, s, y.double(), False)
    with pytest.raises(RuntimeError):
        _lib.fid_moments(S.float(), s, y, False)
    with pytest.raises(RuntimeError):
        _lib.fid_moments(S, s, y.t(), False)
    with pytest.raises(RuntimeError):
        _lib.fid_moments(S, s, y.cpu(), False)
    with pytest.raises(RuntimeError):
        _lib.fid_moments(S, s, y[:, :8].contiguous(), False)
    with pytest.raises(RuntimeError):
        _lib.fid_moments(S, s[:8].contiguous(), y, False)
    with pytest.raises(RuntimeError, match='n >= 2'):
        _lib.fid_finalize(S, s, 1)


# ---------------------------------------------------------------------------------------------------------- (b) accumulation
def test_update_in_batches_equals_one_call():
    from transeditor_amd import fid
    x = integer_features(165, 70, 11)
    xd = torch.from_numpy(x).to(DEV)
    st = fid.FeatureStats(70, chunk=100)
    for a, b in ((0, 64), (64, 128), (128, 165)):            # the fold at 100 rows falls inside the second batch
        st.update(xd[a:b])
    assert st.count == 165
    st._fold()
    check_exact(x, st.S, st.s)
    whole = fid.FeatureStats(70, chunk=165).update(xd)
    whole._fold()
    assert torch.equal(torch.triu(st.S), torch.triu(whole.S)) and torch.equal(st.s, whole.s)
    m, c = st.finalize()
    m2, c2 = whole.finalize()
    assert m.dtype == np.float64 and c.shape == (70, 70) and np.array_equal(m, m2) and np.array_equal(c, c2) and np.array_equal(c, c.T)


def test_merge_of_two_halves_equals_the_whole():
    from transeditor_amd import fid
    x = integer_features(150, 33, 12)
    xd = torch.from_numpy(x).to(DEV)
    a, b = fid.FeatureStats(33, chunk=64).update(xd[:80]), fid.FeatureStats(33, chunk=64).update(xd[80:])
    a.merge(b)
    assert a.count == 150
    check_exact(x, a.S, a.s)
    empty = fid.FeatureStats(33).merge(a)                    # into an instance that holds nothing yet
    check_exact(x, empty.S, empty.s)
    with pytest.raises(ValueError):
        a.merge(fid.FeatureStats(32))


def test_accumulate_flag():
    x, y = integer_features(90, 70, 13), integer_features(45, 70, 14)
    S, s = gpu_moments(y)                                    # accumulate = 0 over NaN-filled outputs
    check_exact(y, S, s)
    gpu_moments(x, True, S, s)
    check_exact(np.concatenate([y, x]), S, s)
    gpu_moments(x, False, S, s)                              # overwrites what is there
    check_exact(x, S, s)


def test_feature_stats_validation():
    from transeditor_amd import fid
    st = fid.FeatureStats(8)
    with pytest.raises(ValueError):
        st.update(torch.zeros(8, device=DEV))
    with pytest.raises(ValueError):
        st.update(torch.zeros(4, 8, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError):
        st.update(torch.zeros(4, 9, device=DEV))
    with pytest.raises(ValueError):
        st.finalize()
    st.update(torch.ones(1, 8, device=DEV))
    with pytest.raises(ValueError):
        st.finalize()                                        # n = 1
    st.update(torch.ones(8, 5, device=DEV).t())              # a non-contiguous batch is copied into the staging buffer as it is
    m, c = st.finalize()
    assert st.count == 6 and np.array_equal(m, np.ones(8)) and np.array_equal(c, np.zeros((8, 8)))


# ---------------------------------------------------------------------------------------------------------- (c) real-valued features
@pytest.fixture(scope='module')
def golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def float_sets(golden):
    sets = {f'{c}_{k}': golden[f'{c}_{k}'] for c in R.CASES for k in ('real', 'fake')}
    sets['big'] = R.draw((2048, 129), (1, 129), np.random.default_rng(5))[0]
    return sets


@pytest.mark.parametrize('name', ['a_real', 'a_fake', 'b_real', 'b_fake', 'c_real', 'c_fake', 'big'])
def test_float_features_within_the_summation_bound(float_sets, name):
    """|S - S_fp64| <= 4 N 2^-53 sum_k |x_ki| |x_kj|: the products are exact, a sum of N terms in any order errs by at most
    (N - 1) 2^-53 sum |terms| to first order, on each side, with a factor 2 to spare.  mean and cov: the same bound carried through
    (S - s s^T / n) / (n - 1) plus 1e-12 max|S| / n for the handful of roundings of the formula itself (cancellation below 10)."""
    from transeditor_amd import _lib
    x = float_sets[name]
    N, D = x.shape
    n, s64, S64 = R.moments(x)
    S, s = gpu_moments(x)
    Sg, sg = S.cpu().numpy(), s.cpu().numpy()
    BS = 4 * N * U * R.abs_moments(x)
    Bs = 4 * N * U * np.abs(x.astype(np.float64)).sum(0)
    iu = np.triu_indices(D)
    print(f'{name}: max |S - S64| / bound {float((np.abs(Sg - S64)[iu] / BS[iu]).max()):.3f}   '
          f'max |s - s64| / bound {float((np.abs(sg - s64) / Bs).max()):.3f}')
    assert np.all(np.abs(Sg - S64)[iu] <= BS[iu]) and np.all(np.abs(sg - s64) <= Bs)
    mean, cov = (t.cpu().numpy() for t in _lib.fid_finalize(S, s, N))
    m64, c64 = R.mean_cov(x)
    slack = 1e-12 * np.abs(S64).max() / N
    Bc = (BS + (np.abs(s64)[:, None] * Bs[None, :] + np.abs(s64)[None, :] * Bs[:, None]) / N) / (N - 1) + slack
    print(f'{name}: max |mean - np.mean| / bound {float((np.abs(mean - m64) / (Bs / N + slack)).max()):.3f}   '
          f'max |cov - np.cov| / bound {float((np.abs(cov - c64) / Bc).max()):.3f}')
    assert np.all(np.abs(mean - m64) <= Bs / N + slack) and np.all(np.abs(cov - c64) <= Bc)
    assert np.array_equal(cov, cov.T)


@pytest.mark.parametrize('case', list(R.CASES))
def test_compute_fid_on_the_golden_features(golden, case):
    from transeditor_amd import fid
    real, fake = golden[f'{case}_real'], golden[f'{case}_fake']
    got = fid.compute_fid(torch.from_numpy(fake).to(DEV), real)                      # a device tensor and an uploaded array
    want, ref = R.fid_of_features(fake, real), float(golden[f'{case}_fid'])
    print(f'case {case}: gpu {got!r}  fp64 restatement {want!r} (relative {abs(got - want) / want:.2e})  reference {ref!r} '
          f'(relative {abs(got - ref) / ref:.2e})')
    assert type(got) is float
    assert abs(got - want) <= (ONEPASS_B if case == 'b' else 1e-10) * want
    assert abs(got - ref) <= REF_RTOL * ref
    st = fid.FeatureStats(real.shape[1], chunk=64).update(torch.from_numpy(real).to(DEV))
    assert abs(fid.compute_fid(st, R.mean_cov(fake)) - want) <= (ONEPASS_B if case == 'b' else 1e-10) * want


# ---------------------------------------------------------------------------------------------------------- (d) determinism
def test_two_runs_are_bit_identical(float_sets):
    from transeditor_amd import fid
    x = torch.from_numpy(float_sets['big']).to(DEV)
    y = torch.from_numpy(float_sets['a_real']).to(DEV)

    def run():
        st = fid.FeatureStats(129, chunk=500)
        for a in range(0, 2048, 192):
            st.update(x[a:a + 192])
        st._fold()
        return st.S.clone(), st.s.clone(), fid.compute_fid(st, st), fid.compute_fid(y, float_sets['a_fake'])
    a, b = run(), run()
    assert torch.equal(torch.triu(a[0]), torch.triu(b[0])) and torch.equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


# ---------------------------------------------------------------------------------------------------------- (e) end to end
@pytest.fixture(scope='module')
def sampler():
    from transeditor_amd import synth
    from transeditor_amd.inference import GeneratorSampler
    from transeditor_amd.model_spatial_query import Generator
    G = Generator(32, 512, 512, 2 * (int(np.log2(32)) - 1), n_trans=8, pixel_norm_op_dim=1)
    sd = G.state_dict()
    synth.fill_state_dict(sd, 21)
    G.load_state_dict(sd)
    return GeneratorSampler(G.to(DEV))


@pytest.fixture(scope='module')
def projection():
    P = (torch.randn(3 * 32 * 32, 48, generator=torch.Generator().manual_seed(9)) / 55.0).to(DEV)

    def feature_fn(image):                                   # a fixed random projection, summed in a fixed order
        return (image.flatten(1)[:, :, None] * P[None]).sum(1)
    return feature_fn


def test_evaluate_fid_end_to_end(sampler, projection, monkeypatch):
    """Both mapping networks open with a PixelNorm, so codes scaled by `truncation` reach the generator as the same directions and
    the FID moves only through the norm's 1e-8 epsilon (measured: 30.910686 -> 30.910692, 1.9e-7 relative).  So the two values
    are only asked to differ, and the codes recorded on their way into the generator pin the scaling itself."""
    from transeditor_amd import fid, prdc
    seen, call = [], type(sampler).__call__

    def recording(self, z, p, **kw):
        seen.append((z.clone(), p.clone()))
        return call(self, z, p, **kw)
    real = prdc.fake_features(sampler, projection, n_sample=80, batch=40, seed=2)    # another draw of the same generator
    real_stats = fid.FeatureStats(48).update(real)
    state = torch.cuda.get_rng_state()
    got = fid.evaluate_fid(sampler, projection, real_stats, n_sample=96, batch=40, seed=1)
    assert torch.equal(state, torch.cuda.get_rng_state())                            # the seed idiom leaves the global state alone
    fake = prdc.fake_features(sampler, projection, n_sample=96, batch=40, seed=1)
    assert fake.shape == (96, 48)
    want = fid.compute_fid(fake, real)
    assert type(got) is float and got > 0 and abs(got - want) <= 1e-10 * want
    st = fid.fake_stats(sampler, projection, n_sample=96, batch=40, seed=1)
    assert isinstance(st, fid.FeatureStats) and st.count == 96 and st.dim == 48
    monkeypatch.setattr(type(sampler), '__call__', recording)
    again = fid.evaluate_fid(sampler, projection, real_stats, n_sample=96, batch=40, seed=1)
    assert abs(again - got) <= 1e-10 * got
    half = fid.evaluate_fid(sampler, projection, real_stats, n_sample=96, batch=40, seed=1, truncation=0.5)
    print(f'truncation 1.0: {got!r}  truncation 0.5: {half!r}')
    assert half != got
    assert [z.shape[0] for z, _ in seen] == [40, 40, 16] * 2
    for (z1, p1), (zh, ph) in zip(seen[:3], seen[3:]):                               # 0.5 is a power of two: the scaling is exact
        assert torch.equal(zh, 0.5 * z1) and torch.equal(ph, 0.5 * p1) and bool(z1.abs().max() > 1)


def test_command_line(tmp_path, capsys, golden):
    from transeditor_amd import fid
    rp, fp, sp, zp = (str(tmp_path / n) for n in ('real.npy', 'fake.npy', 'inception_real.pkl', 'real.npz'))
    np.save(rp, golden['c_real'])
    np.save(fp, golden['c_fake'])
    direct = fid.compute_fid(golden['c_real'], golden['c_fake'])

    def run(argv):
        capsys.readouterr()
        fid.main(argv)
        lines = [x for x in capsys.readouterr().out.splitlines() if x.strip()]
        assert len(lines) == 1
        return json.loads(lines[0])
    out = run(['--real', rp, '--fake', fp])
    assert out['metric'] == 'fid' and out['fid'] == direct and out['n_real'] == 300 and out['n_fake'] == 300
    out = run(['--features', rp, '--write_stats', sp])
    assert out['n'] == 300 and out['dim'] == 33
    with open(sp, 'rb') as f:
        d = pickle.load(f)
    m64, c64 = R.mean_cov(golden['c_real'])
    assert np.allclose(d['mean'], m64, rtol=0, atol=1e-12) and np.allclose(d['cov'], c64, rtol=0, atol=1e-12)
    out = run(['--stats', sp, '--fake', fp])
    assert out['fid'] == direct and out['stats'] == sp
    run(['--features', rp, '--write_stats', zp])
    assert run(['--stats', zp, '--fake', fp])['fid'] == direct


# ---------------------------------------------------------------------------------------------------------- (f) workspace
def test_workspace_size_is_respected_and_bounded():
    from transeditor_amd import _lib
    L = _lib.lib()
    x = integer_features(200, 130, 15)
    xd = torch.from_numpy(x).to(DEV)
    nb = _lib.fid_moments_ws_bytes(200, 130)
    assert nb > 0 and nb % 8 == 0
    guard = 64
    ws = torch.full((nb // 8 + guard,), -7.25, device=DEV, dtype=torch.float64)
    S = torch.zeros(130, 130, device=DEV, dtype=torch.float64)
    s = torch.zeros(130, device=DEV, dtype=torch.float64)
    rc = L.te_fid_moments_f64(S.data_ptr(), s.data_ptr(), ws.data_ptr(), xd.data_ptr(), 200, 130, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    check_exact(x, S, s)
    assert bool((ws[nb // 8:] == -7.25).all())
    assert L.te_fid_moments_f64(S.data_ptr(), s.data_ptr(), None, xd.data_ptr(), 200, 130, 0, None) == -1    # a split needs its workspace
    # at most ceil(2048 / T) <= 2048 / T + 1 splits of T = 528 upper tiles of 32 KiB each, plus 8 x 64 x tiles(D) sums
    nb = _lib.fid_moments_ws_bytes(50000, 2048)
    assert 0 < nb <= (2048 + 528) * 32768 + 64 * (2048 + 63)
    assert _lib.fid_moments_ws_bytes(50000, 4096) == 0

"""FID without a GPU: frechet_distance against the values the reference's own calc_fid returned (tests/golden/fid_ref.npz, written by
tools/fid_golden.py), its algebraic properties, the statistics files, the command line's parser, and the errors where no device exists.

Gaps printed by tools/fid_golden.py when the fixture was written (also stored in it as <case>_gap_ref / <case>_gap_onepass):
    case a: reference against the fp64 eigenvalue route 1.00e-08;  one-pass fp64 moments against two-pass np.cov 2.16e-15
    case b:                                             3.82e-09;                                                 2.05e-09
    case c:                                             3.28e-09;                                                 2.68e-15
The reference takes an fp32 mean (np.mean of float32 features), which alone is of the order 1e-7 relative; REF_RTOL is 10 x the largest
gap of that origin."""
import os
import pickle

import numpy as np
import pytest

import fid_restated as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fid_ref.npz')
REF_RTOL = 10 * 1.00e-8
ENTRY_POINTS = ('te_fid_moments_f64', 'te_fid_moments_ws_bytes', 'te_fid_finalize_f64')


@pytest.fixture(scope='module')
def golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def stats(golden):
    return {c: (R.mean_cov(golden[f'{c}_real']), R.mean_cov(golden[f'{c}_fake'])) for c in R.CASES}


def test_golden_inputs_are_the_documented_draws(golden):
    for name, (real, fake) in R.draw_all().items():
        assert real.shape == R.CASES[name][0] and fake.shape == R.CASES[name][1] and real.dtype == np.float32
        assert np.array_equal(real, golden[f'{name}_real']) and np.array_equal(fake, golden[f'{name}_fake'])
        assert real.min() >= 0 and fake.min() >= 0
    assert max(float(golden[f'{c}_gap_ref']) for c in R.CASES) <= 1.00e-8 * 1.01       # what the docstring and REF_RTOL quote
    assert os.path.getsize(GOLDEN) < 300 * 1024


@pytest.mark.parametrize('case', list(R.CASES))
def test_frechet_distance_against_the_reference(golden, stats, case):
    from transeditor_amd import fid
    (mr, cr), (mf, cf) = stats[case]
    got, ref = fid.frechet_distance(mf, cf, mr, cr), float(golden[f'{case}_fid'])
    print(f'case {case}: frechet_distance {got!r}  reference {ref!r}  relative gap {abs(got - ref) / ref:.2e}')
    assert type(got) is float
    assert abs(got - ref) <= REF_RTOL * ref
    # the independent restatement of the same route.  Full rank: a handful of fp64 roundings.  Case b: each of the ~40 null directions
    # of the two covariances turns eigenvalue noise of 1e-16 |cov| into a root of 1e-8, so two codings of one formula agree no better
    # than either agrees with the reference
    assert abs(got - R.frechet(mf, cf, mr, cr)) <= (REF_RTOL if case == 'b' else 1e-12) * ref


@pytest.mark.parametrize('case', list(R.CASES))
def test_symmetry_and_zero(stats, case):
    from transeditor_amd import fid
    (mr, cr), (mf, cf) = stats[case]
    ab, ba = fid.frechet_distance(mr, cr, mf, cf), fid.frechet_distance(mf, cf, mr, cr)
    # full rank: fp64 rounding of a handful of D x D products.  Every null direction of either covariance leaves an eigenvalue of
    # rounding noise, eps |cov_a| |cov_b|, whose clipped square root enters the trace: that much per direction is not determined
    D = cr.shape[0]
    null = 2 * D - np.linalg.matrix_rank(cr) - np.linalg.matrix_rank(cf)
    tol = 1e-12 * abs(ab) + null * np.sqrt(2.0 ** -52 * np.linalg.norm(cr, 2) * np.linalg.norm(cf, 2))
    print(f'case {case}: |d(a,b) - d(b,a)| = {abs(ab - ba):.2e}, allowed {tol:.2e} ({null} null directions)')
    assert abs(ab - ba) <= tol
    for m, c in ((mr, cr), (mf, cf)):
        assert abs(fid.frechet_distance(m, c, m, c)) <= 1e-9 * np.trace(c)


def test_rank_deficient_inputs_stay_finite_and_real(golden):
    from transeditor_amd import fid
    real, fake = golden['b_real'], golden['b_fake']
    (mr, cr), (mf, cf) = R.mean_cov(real), R.mean_cov(fake)
    assert np.linalg.matrix_rank(cr) < 64 and np.linalg.matrix_rank(cf) < 64
    v = fid.frechet_distance(mr, cr, mf, cf)
    assert isinstance(v, float) and np.isfinite(v) and v > 0
    x = np.zeros((5, 7))                                                               # rank 1 against rank 0
    x[:, 0] = np.arange(5)
    m1, c1 = R.mean_cov(x)
    v = fid.frechet_distance(m1, c1, np.zeros(7), np.zeros((7, 7)))
    assert np.isfinite(v) and abs(v - (4.0 + 2.5)) <= 1e-12                            # |mean|^2 = 4, tr = var(0..4) = 2.5
    with pytest.raises(ValueError):
        fid.frechet_distance(m1, c1, np.zeros(6), np.zeros((6, 6)))


def test_statistics_files_round_trip(tmp_path, stats):
    from transeditor_amd import fid
    (mean, cov), _ = stats['c']
    for name in ('s.pkl', 's.npz'):
        p = str(tmp_path / name)
        fid.save_stats(p, mean, cov, size=256)
        m, c = fid.load_stats(p)
        assert m.dtype == np.float64 and np.array_equal(m, mean) and np.array_equal(c, cov)
    with open(tmp_path / 's.pkl', 'rb') as f:
        d = pickle.load(f)
    assert set(d) == {'mean', 'cov', 'size'} and d['size'] == 256
    # calc_inception.py:115-116 as a user has it: an fp32 mean, an fp64 cov and two more keys
    p = str(tmp_path / 'inception_x.pkl')
    with open(p, 'wb') as f:
        pickle.dump({'mean': mean.astype(np.float32), 'cov': cov, 'size': 256, 'path': 'ffhq_lmdb'}, f)
    m, c = fid.load_stats(p)
    assert m.dtype == np.float64 and np.array_equal(m, mean.astype(np.float32).astype(np.float64)) and np.array_equal(c, cov)
    with open(p, 'wb') as f:
        pickle.dump({'mean': mean}, f)
    with pytest.raises(ValueError):
        fid.load_stats(p)


def test_command_line_parser():
    from transeditor_amd import fid
    P = fid.build_parser
    assert P().parse_args(['--real', 'r.npy', '--fake', 'f.npy']).mode == 'files'
    assert P().parse_args(['--stats', 's.pkl', '--fake', 'f.npy']).mode == 'stats'
    assert P().parse_args(['--features', 'r.npy', '--write_stats', 'o.pkl']).mode == 'write'
    bad = [[], ['--real', 'r'], ['--fake', 'f'], ['--stats', 's'], ['--features', 'x'], ['--write_stats', 'o'],
           ['--real', 'r', '--stats', 's', '--fake', 'f'], ['--real', 'r', '--fake', 'f', '--features', 'x', '--write_stats', 'o'],
           ['--stats', 's', '--features', 'x', '--write_stats', 'o'], ['--fake', 'f', '--features', 'x', '--write_stats', 'o'],
           ['--real', 'r', '--fake', 'f', '--write_stats', 'o'], ['--ckpt', 'c.pt', '--fake', 'f']]
    for argv in bad:
        with pytest.raises(SystemExit):
            P().parse_args(argv)


def test_needs_a_gpu_where_there_is_none():
    import torch
    from transeditor_amd import fid
    with pytest.raises(ValueError):
        fid.compute_fid(np.zeros((8, 5), np.float64), np.zeros((8, 5), np.float32))
    with pytest.raises(ValueError):
        fid.compute_fid(np.zeros(8, np.float32), np.zeros((8, 5), np.float32))
    with pytest.raises(ValueError):
        fid.FeatureStats(0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a GPU'):
            fid.FeatureStats(8)
        with pytest.raises(RuntimeError, match='needs a GPU'):
            fid.compute_fid(np.zeros((8, 5), np.float32), np.zeros((8, 5), np.float32))
        with pytest.raises(RuntimeError, match='needs a GPU'):
            fid.main(['--real', 'r.npy', '--fake', 'f.npy'])
    # statistics on both sides need no device at all
    m, c = np.zeros(3), np.eye(3)
    assert fid.compute_fid((m, c), (m + 1.0, c)) == pytest.approx(3.0, abs=1e-12)


def test_header_declares_and_binding_binds_the_entry_points():
    from transeditor_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'te_hip.h')).read()
    for name in ENTRY_POINTS:
        assert name + '(' in header and name in _lib.EXPORTS
    assert 'fid_query.py:162-163' in header and 'calc_inception.py:110-111' in header
    L = _lib.lib()
    assert L.te_version() == 3
    assert L.te_fid_moments_ws_bytes(0, 8) < 0 and L.te_fid_moments_ws_bytes(8, 0) < 0 and L.te_fid_moments_ws_bytes(8, 8193) < 0
    assert L.te_fid_moments_ws_bytes(1, 1) == 0 and L.te_fid_moments_ws_bytes(50000, 8192) == 0
    assert L.te_fid_moments_f64(None, None, None, None, 8, 8, 0, None) == -1
    assert L.te_fid_finalize_f64(None, None, None, None, 8, 8, None) == -1

"""PRDC without a GPU: the fp64 restatement (tests/prdc_restated.py) reproduces what the reference's metrics/prdc.py returned for the two
golden cases (tests/golden/prdc_ref.npz, written by tools/prdc_golden.py), and the host side of transeditor_amd.prdc (argument checks,
the command line) works where no GPU exists."""
import os

import numpy as np
import pytest

import prdc_restated as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'prdc_ref.npz')
KEYS = ('precision', 'recall', 'density', 'coverage')


@pytest.fixture(scope='module')
def golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize('case,real_shape,fake_shape,k', [('a', (257, 96), (130, 96), 3), ('b', (129, 33), (67, 33), 1)])
def test_restatement_reproduces_the_reference(golden, case, real_shape, fake_shape, k):
    real, fake = golden[f'{case}_real'], golden[f'{case}_fake']
    assert real.shape == real_shape and fake.shape == fake_shape and real.dtype == np.float32 and int(golden[f'{case}_k']) == k
    d = R.details(real, fake, k)
    got = R.numbers(d, k)
    ref = dict(zip(KEYS, golden[f'{case}_prdc']))
    n, m = real_shape[0], fake_shape[0]
    # the recorded values are means of booleans / counts: compare as the counts they stand for
    assert round(ref['precision'] * m) == round(got['precision'] * m) and got['precision'] == ref['precision']
    assert round(ref['recall'] * n) == round(got['recall'] * n) and got['recall'] == ref['recall']
    assert round(ref['density'] * k * m) == round(got['density'] * k * m)
    assert abs(got['density'] - ref['density']) <= 1e-15 * max(1.0, ref['density'])    # (1 / k) * mean vs sum / (k m): one rounding apart
    assert round(ref['coverage'] * n) == round(got['coverage'] * n) and got['coverage'] == ref['coverage']
    # the margin that lets an fp32 evaluation reproduce them (ISSUE: 3.3e-5 and 1.7e-4 with seed 1)
    assert R.min_relative_gap(d) > 1e-5


def test_golden_inputs_are_the_documented_draws(golden):
    rng = np.random.default_rng(1)
    real = rng.standard_normal((257, 96)).astype(np.float32)
    fake = (0.9 * rng.standard_normal((130, 96)) + 0.1).astype(np.float32)
    assert np.array_equal(real, golden['a_real']) and np.array_equal(fake, golden['a_fake'])
    assert os.path.getsize(GOLDEN) < 200 * 1024


def test_restatement_edge_cases():
    x = np.array([[0.0], [1.0], [1.0], [3.0]])
    assert np.array_equal(R.radii2(x, 1), [1.0, 0.0, 0.0, 4.0])               # duplicates count separately
    assert np.array_equal(R.radii2(x, 3), [9.0, 4.0, 4.0, 9.0])
    d = R.details(x, x, 1)
    assert np.array_equal(d['col_count'], [1, 0, 0, 1]) and np.array_equal(d['row_min'], [0, 0, 0, 0])   # 0 < 0 is false (strict)


def test_module_imports_and_validates_without_a_gpu():
    from transeditor_amd import prdc
    real = np.zeros((8, 5), np.float32)
    fake = np.zeros((9, 5), np.float32)
    for k in (0, 16, -1, 2.0, True):
        with pytest.raises(ValueError, match='nearest_k'):
            prdc.compute_prdc(real, fake, k)
    with pytest.raises(ValueError, match='at least'):
        prdc.compute_prdc(real[:3], fake, 3)
    with pytest.raises(ValueError, match='at least'):
        prdc.compute_prdc(real, fake[:4], 4)
    with pytest.raises(ValueError, match='feature dimension'):
        prdc.compute_prdc(real, np.zeros((9, 6), np.float32), 3)
    with pytest.raises(ValueError, match=r'\[N,D\]'):
        prdc.compute_prdc(real[0], fake, 3)
    with pytest.raises(ValueError, match='float32'):
        prdc.compute_prdc(real.astype(np.float64), fake, 3)
    with pytest.raises(ValueError, match='float32'):
        prdc.prdc_details(real, fake.astype(np.float64), 3)


def test_command_line_parser(tmp_path):
    from transeditor_amd import prdc
    a = prdc.build_parser().parse_args(['--real', 'r.npy', '--fake', 'f.npy'])
    assert (a.real, a.fake, a.nearest_k) == ('r.npy', 'f.npy', 3)
    assert prdc.build_parser().parse_args(['--real', 'r', '--fake', 'f', '--nearest_k', '5']).nearest_k == 5
    with pytest.raises(SystemExit):
        prdc.build_parser().parse_args(['--real', 'r.npy'])
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='GPU'):
            prdc.main(['--real', 'r.npy', '--fake', 'f.npy'])


def test_binding_has_the_prdc_entry_points():
    from transeditor_amd import _lib
    for name in ('te_prdc_ws_bytes', 'te_row_sqnorm_f32', 'te_prdc_knn_f32', 'te_prdc_counts_f32'):
        assert name in _lib.EXPORTS
    L = _lib.lib()
    assert 0 < L.te_prdc_ws_bytes(50000, 50000, 4096, 3) < 1 << 30              # no N x M buffer
    assert L.te_prdc_ws_bytes(3, 50, 8, 3) < 0 and L.te_prdc_ws_bytes(50, 50, 8, 0) < 0 and L.te_prdc_ws_bytes(50, 50, 8, 16) < 0
    assert L.te_prdc_ws_bytes(50, 50, 0, 3) < 0
    assert L.te_prdc_knn_f32(None, None, None, 8, 8, 3, None, None) == -1
    assert L.te_row_sqnorm_f32(None, None, 8, 8, None) == -1

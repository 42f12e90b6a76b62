"""Host side of the DEX age / gender scorer (transeditor_amd.dex), of the editing evaluation (transeditor_amd.edit_eval) and of the drop-in
ffhq_utils.dex: state dict parsing and the geometry read from it, the dependency figure against a literal transcription, the sweep
score layout, the drop-in's surface, the argument parser and the ABI's argument checks.  No GPU is needed."""
import importlib
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import dex_restated as R
from conftest import ROOT


@pytest.fixture(scope='module')
def sd():
    return R.state_dict(0, pool=2, hidden=(24, 16), classes=101)


# ---------------------------------------------------------------------------------------------------------- the state dict
def test_geometry_is_read_from_the_shapes(sd):
    from transeditor_amd import dex
    net = dex.parse_state_dict(sd)
    assert (net['pool'], net['crop'], net['hidden'], net['classes']) == (2, 64, (24, 16), 101)
    assert len(net['convs']) == 13 and tuple(net['convs'][0][0].shape) == (64, 3, 3, 3) and tuple(net['convs'][12][0].shape) == (512, 512, 3, 3)
    assert dex.dex_conv_keys() == [k for k, _, _ in R.conv_keys()]
    assert dex.dex_conv_keys()[:3] == ['conv.0.conv1', 'conv.0.conv2', 'conv.1.conv1'] and dex.dex_conv_keys()[-1] == 'conv.4.conv3'
    real = dex.parse_state_dict({k: (torch.zeros(4096, 25088) if k == 'fc1.0.weight' else v)
                                 for k, v in R.state_dict(0, pool=1, hidden=(4096, 8), classes=2).items()})
    assert (real['pool'], real['crop'], real['hidden'], real['classes']) == (7, 224, (4096, 8), 2)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        s = dex.DEXScorer(state_dict=sd, attribute='age')
    assert (s.pool, s.crop, s.hidden, s.classes, s.attribute) == (2, 64, (24, 16), 101, 'age')
    names = {n for n, _ in s.named_buffers()}
    assert len(names) == 32 and {'w0', 'b12', 'fc1_w', 'fc2_b', 'cls_w', 'cls_b'} <= names and not s.training
    with pytest.warns(RuntimeWarning, match='101 classes'):
        g = dex.DEXScorer(state_dict=sd, attribute='gender')
    assert g.mode == 1 and s.mode == 0
    a, b = R.state_dict(3, pool=1, hidden=(8, 8), classes=(101, 2))                          # one trunk, two heads
    assert a['fc1.0.weight'] is b['fc1.0.weight'] and a['cls.weight'].shape == (101, 8) and b['cls.weight'].shape == (2, 8)
    assert torch.equal(b['cls.weight'], R.state_dict(3, pool=1, hidden=(8, 8), classes=2)['cls.weight'])


def test_state_dict_validation(sd, tmp_path):
    from transeditor_amd.dex import DEXScorer
    bad = dict(sd)
    del bad['conv.2.conv3.bias']
    with pytest.raises(ValueError, match=r'has no conv\.2\.conv3\.weight / conv\.2\.conv3\.bias'):
        DEXScorer(state_dict=bad)
    bad = dict(sd)
    del bad['cls.weight']
    with pytest.raises(ValueError, match=r'has no cls\.weight'):
        DEXScorer(state_dict=bad)
    bad = dict(sd)
    bad['conv.1.conv1.weight'] = torch.zeros(128, 32, 3, 3)
    with pytest.raises(ValueError, match=r'conv\.1\.conv1\.weight is \(128, 32, 3, 3\) / bias \(128,\), expected \(128, 64, 3, 3\)'):
        DEXScorer(state_dict=bad)
    bad = dict(sd)
    bad['fc1.0.weight'] = torch.zeros(24, 512 * 3)                                           # not 512 * pool^2
    with pytest.raises(ValueError, match=r'fc1\.0\.weight is \(24, 1536\)'):
        DEXScorer(state_dict=bad)
    bad = dict(sd)
    bad['fc2.0.weight'] = torch.zeros(16, 20)
    with pytest.raises(ValueError, match=r'fc2\.0\.weight is \(16, 20\), expected \[J, 24\]'):
        DEXScorer(state_dict=bad)
    bad = dict(sd)
    bad['cls.bias'] = torch.zeros(100)
    with pytest.raises(ValueError, match=r'cls\.weight is \(101, 16\) / bias \(100,\)'):
        DEXScorer(state_dict=bad)
    p = str(tmp_path / 'w.pth')
    torch.save(bad, p)
    with pytest.raises(ValueError, match='cls.weight'):
        DEXScorer(p)
    with pytest.raises(ValueError, match='not both'):
        DEXScorer(p, state_dict=sd)
    with pytest.raises(ValueError, match='must be a dict'):
        DEXScorer(state_dict=[1])
    with pytest.raises(ValueError, match="'age' or 'gender'"):
        DEXScorer(state_dict=sd, attribute='pose')
    with pytest.raises(FileNotFoundError, match='absent.pth'):
        DEXScorer(str(tmp_path / 'absent.pth'))


def test_scorer_input_checks_and_no_cpu_path(sd):
    from transeditor_amd.dex import DEXScorer
    s = DEXScorer(state_dict=sd)
    with pytest.raises(ValueError, match=r'\[B,3,S,S\]'):
        s(torch.zeros(1, 1, 64, 64))
    with pytest.raises(ValueError, match='square'):
        s(torch.zeros(1, 3, 64, 66))
    with pytest.raises(ValueError, match='S >= 64'):
        s(torch.zeros(1, 3, 48, 48))
    with pytest.raises(ValueError, match='even'):
        s(torch.zeros(1, 3, 65, 65))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a GPU'):
            s(torch.zeros(1, 3, 64, 64))
        with pytest.raises(RuntimeError, match='needs a GPU'):
            s.probabilities(torch.zeros(1, 3, 66, 66), preprocessed=True)


def test_restatement_shapes_and_preprocessing(sd):
    x = R.images(1, 2, 70)
    v = R.preprocess(x, 64)
    assert tuple(v.shape) == (2, 3, 64, 64) and float(v.min()) == 0 and float(v.max()) == 255 and bool((v == v.round()).all())
    want = ((x[:, [2, 1, 0]].clamp(-1, 1) + 1) / 2 * 255).round()[:, :, 3:67, 3:67]
    assert torch.equal(v, want)
    p = R.probabilities(x, sd, torch.float32)
    assert tuple(p.shape) == (2, 101) and float((p.sum(1) - 1).abs().max()) < 1e-5
    assert torch.equal(R.probabilities(v, sd, torch.float32, preprocessed=True), p)
    assert abs(float(R.score_of(torch.full((1, 101), 1 / 101, dtype=torch.float64), 'age')) - 51.0) < 1e-12      # the weights start at 1
    assert float(R.score_of(torch.tensor([[0.25, 0.75]]), 'gender')) == 0.25


# ---------------------------------------------------------------------------------------------------------- the evaluation
def _literal_ratio(change, interest):
    """calculate_score.py:47-71 for one (attribute pair, space) at the reference's width 7, element by element: per result row the three
    steps right of the origin (columns 3 -> 4 -> 5 -> 6) and the three left of it (3 -> 2 -> 1 -> 0), each sum divided by the row count"""
    sums = {'change+': 0.0, 'change-': 0.0, 'interest+': 0.0, 'interest-': 0.0}
    for name, rows in (('change', change), ('interest', interest)):
        for row in rows:
            assert len(row) == 7
            for k in (4, 5, 6):
                sums[name + '+'] += row[k] - row[k - 1]
            for k in (0, 1, 2):
                sums[name + '-'] += row[k] - row[k + 1]
    m = len(change)
    return (abs((sums['interest+'] / m) / (sums['change+'] / m)) + abs((sums['interest-'] / m) / (sums['change-'] / m))) / 2


def test_dependency_ratio():
    from transeditor_amd.edit_eval import dependency_ratio
    rng = np.random.default_rng(4)
    change, interest = rng.normal(size=(9, 7)).cumsum(1), rng.normal(size=(9, 7))
    got = dependency_ratio(change, interest)
    assert abs(got - _literal_ratio(change.tolist(), interest.tolist())) <= 1e-12 * abs(got)
    assert abs(dependency_ratio(change.astype(np.float32), interest.astype(np.float32)) - got) < 1e-5 * abs(got)
    # one row by hand: change + = (5-4)+(7-5)+(8-7) = 4, change - = (1-2)+(2-3)+(3-4) = -3; interest + = 1, interest - = 0.5 - 2 = -1.5
    one = dependency_ratio([[1, 2, 3, 4, 5, 7, 8]], [[0.5, 0.5, 0.5, 2, 2, 2, 3]])
    assert one == (1 / 4 + 1.5 / 3) / 2
    assert dependency_ratio([[0, 1, 3]], [[5, 5, 6]]) == (1 / 2 + 0 / 1) / 2                  # h = 1
    assert dependency_ratio(np.ones((2, 5)).cumsum(1), np.ones((2, 5)).cumsum(1)) == 1.0
    for bad in (([[1, 2, 3, 4]], [[1, 2, 3, 4]]), ([[1, 2, 3]], [[1, 2, 3, 4, 5]]), ([1, 2, 3], [1, 2, 3]), ([[1]], [[1]])):
        with pytest.raises(ValueError, match='dependency_ratio'):
            dependency_ratio(*bad)


def test_score_sweeps_layout():
    from transeditor_amd.edit_eval import score_sweeps
    calls = []

    def mean_scorer(images):
        calls.append(images.shape[0])
        return images.mean((1, 2, 3))

    origin = torch.arange(2, dtype=torch.float32).view(2, 1, 1, 1).expand(2, 3, 4, 4) + 100                   # scores 100, 101
    sweep = (torch.arange(12, dtype=torch.float32).view(2, 6, 1, 1, 1)).expand(2, 6, 3, 4, 4)                 # scores 0..5, 6..11
    res = score_sweeps({'a': mean_scorer, 'b': lambda im: -im.mean((1, 2, 3))}, origin, {'p': sweep, 'z': sweep + 20}, batch=5)
    assert set(res) == {'a', 'b'} and set(res['a']) == {'p', 'z'}
    assert res['a']['p'].dtype == np.float32 and res['a']['p'].shape == (2, 7)
    assert np.array_equal(res['a']['p'], [[0, 1, 2, 100, 3, 4, 5], [6, 7, 8, 101, 9, 10, 11]])
    assert np.array_equal(res['a']['z'], [[20, 21, 22, 100, 23, 24, 25], [26, 27, 28, 101, 29, 30, 31]])
    assert np.array_equal(res['b']['p'], -res['a']['p'])
    assert calls == [2, 5, 5, 2, 5, 5, 2]                                                      # the origin, then 12 images per sweep
    odd = score_sweeps({'a': mean_scorer}, origin, {'pz': sweep[:, :5]}, batch=64)['a']['pz']  # 5 steps: the origin in column 2
    assert np.array_equal(odd, [[0, 1, 100, 2, 3, 4], [6, 7, 101, 8, 9, 10]])
    with pytest.raises(ValueError, match="sweep 'p'"):
        score_sweeps({'a': mean_scorer}, origin, {'p': sweep[:1]}, batch=4)
    with pytest.raises(ValueError, match='batch'):
        score_sweeps({'a': mean_scorer}, origin, {'p': sweep}, batch=0)


# ---------------------------------------------------------------------------------------------------------- the drop-in
def test_dropin_surface_and_named_errors(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, 'dropin'))
    names = ('ffhq_utils', 'ffhq_utils.dex')
    try:
        for n in names:
            sys.modules.pop(n, None)
        dex = importlib.import_module('ffhq_utils.dex')
        assert dex.__file__ == os.path.join(ROOT, 'dropin', 'ffhq_utils', 'dex.py')
        assert callable(dex.eval) and callable(dex.estimate_age) and callable(dex.estimate_gender)
        monkeypatch.delenv('TE_DEX_DIR', raising=False)
        for call in (lambda: dex.eval('age'), lambda: dex.eval('gender'), lambda: dex.estimate_age(torch.zeros(1, 3, 256, 256))):
            with pytest.raises(RuntimeError, match='TE_DEX_DIR'):
                call()
        monkeypatch.setenv('TE_DEX_DIR', str(tmp_path))
        with pytest.raises(RuntimeError, match='age_sd.pth'):
            dex.eval('age')
        with pytest.raises(RuntimeError, match='gender_sd.pth'):
            dex.estimate_gender(torch.zeros(1, 3, 256, 256))
        with pytest.raises(ValueError, match="'pose'"):
            dex.eval('pose')
        torch.save(R.state_dict(0, pool=1, hidden=(8, 8), classes=2), str(tmp_path / 'gender_sd.pth'))
        dex.eval('gender')                                                                   # loads; the scorer is kept
        assert dex._scorer('gender').crop == 32 and dex._scorer('gender').attribute == 'gender'
    finally:
        sys.path.remove(os.path.join(ROOT, 'dropin'))
        for n in names:
            sys.modules.pop(n, None)


# ---------------------------------------------------------------------------------------------------------- the command line, the ABI
def test_command_line():
    from transeditor_amd import dex, edit
    parse = dex.build_parser().parse_args
    a = parse(['--ckpt', 'G.pt', '--weights', 'age_sd.pth', '--write_z_boundary', 'zb.npy', '--write_p_boundary', 'pb.npy'])
    assert (a.ckpt, a.weights, a.attribute, a.num_sample, a.write_z_boundary, a.write_p_boundary, a.write_scores) == \
        ('G.pt', 'age_sd.pth', 'age', 10000, 'zb.npy', 'pb.npy', None)
    assert (a.ratio, a.split_ratio, a.truncation, a.size, a.batch, a.seed, a.para_num) == (0.02, 0.7, 0.7, 256, 16, None, 16)
    a = parse(['--ckpt', 'G.pt', '--weights', 'g.pth', '--attribute', 'gender', '--num_sample', '500', '--write_z_boundary', 'z.npy',
               '--write_p_boundary', 'p.npy', '--write_scores', 's.npy', '--seed', '3', '--batch', '8'])
    assert (a.attribute, a.num_sample, a.write_scores, a.seed, a.batch) == ('gender', 500, 's.npy', 3, 8)
    for bad in (['--ckpt', 'G.pt', '--weights', 'w.pth', '--write_z_boundary', 'z.npy'], ['--weights', 'w.pth', '--write_z_boundary', 'z.npy',
                '--write_p_boundary', 'p.npy'], ['--ckpt', 'G.pt', '--weights', 'w.pth', '--attribute', 'pose', '--write_z_boundary', 'z.npy',
                '--write_p_boundary', 'p.npy']):
        with pytest.raises(SystemExit):
            parse(bad)
    full = ['--ckpt', 'G.pt', '--weights', 'w.pth', '--write_z_boundary', 'z.npy', '--write_p_boundary', 'p.npy']
    with pytest.raises(SystemExit):
        dex.main(full + ['--size', '48'])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a GPU'):
            dex.main(full)
    assert 'write_z_boundary' not in edit.build_parser().format_help()                        # edit's own parser is as it was
    assert 'transeditor_amd.dex' in edit.__doc__


def test_abi_entry_points_and_argument_checks():
    import ctypes
    from transeditor_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    for name in ('te_dex_stem_fwd_f32', 'te_cls_score_f32'):
        assert name in _lib.EXPORTS and name + '(' in header
    assert 'M5' in header and 'api.py:42-65' in header and 'edit_all_noinversion_ffhq.py:113-116' in header and 'models.py:55-56' in header
    L = _lib.lib()
    assert L.te_version() == 3
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16                                 # validation only: never dereferenced
    assert L.te_dex_stem_fwd_f32(None, p, p, p, 1, 40, 40, 32, None) == -1 and b'NULL' in L.te_last_error_string()
    for N, H, W, crop in [(1, 40, 40, 0), (1, 40, 40, 42), (1, 40, 40, 33), (1, 41, 40, 32), (1, 40, 30, 32), (65536, 40, 40, 32)]:
        assert L.te_dex_stem_fwd_f32(p, p, p, p, N, H, W, crop, None) == -2, (N, H, W, crop)
    assert L.te_cls_score_f32(p, None, p, p, None, 3, 4, 8, 0, None) == -1
    for I, C, K in [(3, 0, 8), (3, 1025, 8), (3, 4, 6), (3, 4, 0), (0, 4, 8)]:
        assert L.te_cls_score_f32(p, None, p, p, p, I, C, K, 0, None) == -2, (I, C, K)
    assert L.te_cls_score_f32(p, None, p + 4, p, p, 3, 4, 8, 0, None) == -2 and b'16-byte aligned' in L.te_last_error_string()
    assert L.te_cls_score_f32(p, None, p, p + 8, p, 3, 4, 8, 1, None) == -2
    assert L.te_cls_score_f32(p, None, p, p, p, 3, 4, 8, 2, None) == -3 and b'mode' in L.te_last_error_string()
    assert (_lib.CLS_EXPECTATION, _lib.CLS_FIRST) == (0, 1)

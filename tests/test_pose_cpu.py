"""Host side of the pose scorer (transeditor_amd.pose) and of the drop-in's estimate_pose: state dict parsing and the geometry read from it,
the batch-norm fold against conv + batch norm in fp64, every named error, the argument parser, the drop-in's surface and the ABI's
argument checks.  No GPU is needed."""
import ctypes
import importlib
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import pose_restated as R
import scorer_checks
from conftest import ROOT, rel_l2

SMALL = (8, 12, 16, 20)


@pytest.fixture(scope='module')
def sd():
    return R.state_dict(0, widths=SMALL)


# ---------------------------------------------------------------------------------------------------------- the state dict
def test_geometry_is_read_from_the_shapes(sd):
    from transeditor_amd import pose
    net = pose.parse_state_dict(sd)
    assert net['widths'] == SMALL and net['classes'] == 2 and R.widths_of(sd) == SMALL
    keys = pose.pose_conv_keys()
    assert len(keys) == 20 and set(net['convs']) == {k for k, *_ in keys}
    assert {(k, b) for k, b, *_ in keys} == {(k, b) for k, b, _ in R.conv_bn_keys()}
    assert keys[0] == ('backbone.0', 'backbone.1', 2, 3, False) and keys[1] == ('backbone.4.0.conv1', 'backbone.4.0.bn1', 1, 1, False)
    assert keys[2] == ('backbone.4.0.conv2', 'backbone.4.0.bn2', 1, 1, True)
    assert keys[5:8] == [('backbone.5.0.conv1', 'backbone.5.0.bn1', 2, 1, False), ('backbone.5.0.downsample.0', 'backbone.5.0.downsample.1', 2, 0, False),
                         ('backbone.5.0.conv2', 'backbone.5.0.bn2', 1, 1, True)]
    assert tuple(net['convs']['backbone.0'][0].shape) == (8, 3, 7, 7) and tuple(net['convs']['backbone.7.0.downsample.0'][0].shape) == (20, 16, 1, 1)
    assert all(w.dtype == torch.float32 and b.dtype == torch.float32 and b.shape == (w.shape[0],) for w, b in net['convs'].values())
    s = pose.PoseScorer(state_dict=sd)
    assert (s.crop, s.widths, s.classes) == (224, SMALL, 2) and not s.training
    names = {n for n, _ in s.named_buffers()}
    assert len(names) == 42 and {'w0', 'b19', 'extra_w', 'extra_b'} <= names
    assert pose.PoseScorer(state_dict=sd, crop=62).crop == 62
    assert any(k.endswith('num_batches_tracked') for k in sd)
    bare = {k: v for k, v in sd.items() if not k.endswith('num_batches_tracked')}                 # ignored: present or not
    assert torch.equal(pose.PoseScorer(state_dict=bare).w7, s.w7)
    wide = R.state_dict(2, widths=(8, 8, 8, 12), classes=5)                                        # equal widths still downsample at stride 2
    assert pose.parse_state_dict(wide)['widths'] == (8, 8, 8, 12) and pose.parse_state_dict(wide)['classes'] == 5
    assert callable(pose.fit_boundaries)


def test_state_dict_validation(sd, tmp_path):
    from transeditor_amd.pose import PoseScorer
    bad = dict(sd)
    del bad['backbone.5.0.downsample.0.weight']
    with pytest.raises(ValueError, match=r'state_dict has no backbone\.5\.0\.downsample\.0\.weight \(not a ClassifyModel state dict'):
        PoseScorer(state_dict=bad)
    bad = dict(sd)
    del bad['backbone.6.1.bn2.running_var']
    with pytest.raises(ValueError, match=r'has no backbone\.6\.1\.bn2\.running_var'):
        PoseScorer(state_dict=bad)
    bad = dict(sd)
    del bad['extra_layer.bias']
    with pytest.raises(ValueError, match=r'has no extra_layer\.weight / extra_layer\.bias'):
        PoseScorer(state_dict=bad)
    bad = dict(sd)
    bad['backbone.0.weight'] = torch.zeros(8, 3, 3, 3)
    with pytest.raises(ValueError, match=r'backbone\.0\.weight is \(8, 3, 3, 3\), expected \(None, 3, 7, 7\)'):
        PoseScorer(state_dict=bad)
    bad = dict(sd)
    bad['backbone.4.0.conv1.weight'] = torch.zeros(12, 8, 3, 3)                                   # layer1 has no downsample: the stem's width
    with pytest.raises(ValueError, match=r'backbone\.4\.0\.conv1\.weight is \(12, 8, 3, 3\), expected \(8, 8, 3, 3\)'):
        PoseScorer(state_dict=bad)
    bad = dict(sd)
    bad['backbone.5.1.conv2.weight'] = torch.zeros(12, 8, 3, 3)
    with pytest.raises(ValueError, match=r'backbone\.5\.1\.conv2\.weight is \(12, 8, 3, 3\), expected \(12, 12, 3, 3\)'):
        PoseScorer(state_dict=bad)
    bad = dict(sd)
    bad['backbone.6.0.bn1.bias'] = torch.zeros(12)
    with pytest.raises(ValueError, match=r'backbone\.6\.0\.bn1\.bias is \(12,\), expected \(16,\)'):
        PoseScorer(state_dict=bad)
    bad = dict(sd)
    bad['extra_layer.weight'] = torch.zeros(2, 16)
    with pytest.raises(ValueError, match=r'extra_layer\.weight is \(2, 16\) / bias \(2,\), expected \(None, 20\)'):
        PoseScorer(state_dict=bad)
    p = str(tmp_path / 'weight.pkl')
    torch.save(bad, p)
    with pytest.raises(ValueError, match='extra_layer.weight'):
        PoseScorer(p)
    with pytest.raises(ValueError, match='not both'):
        PoseScorer(p, state_dict=sd)
    with pytest.raises(ValueError, match='must be a dict'):
        PoseScorer(state_dict=[1])
    with pytest.raises(ValueError, match='crop must be a positive integer'):
        PoseScorer(state_dict=sd, crop=0)
    with pytest.raises(FileNotFoundError, match='pose classifier weight file not found: .*absent.pkl'):
        PoseScorer(str(tmp_path / 'absent.pkl'))
    torch.save(sd, p)
    assert PoseScorer(p).widths == SMALL


def test_scorer_input_checks_and_no_cpu_path(sd):
    from transeditor_amd.pose import PoseScorer
    s = PoseScorer(state_dict=sd, crop=64)
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


# ---------------------------------------------------------------------------------------------------------- the fold
@pytest.mark.parametrize('key,bn,stride,pad', [('backbone.0', 'backbone.1', 2, 3), ('backbone.5.0.conv1', 'backbone.5.0.bn1', 2, 1),
                                               ('backbone.6.0.downsample.0', 'backbone.6.0.downsample.1', 2, 0),
                                               ('backbone.7.1.conv2', 'backbone.7.1.bn2', 1, 1)])
def test_fold_against_conv_and_batch_norm(sd, key, bn, stride, pad):
    """conv(x, w') + b' against batch_norm(conv(x, w)) in fp64: the fold done in fp64 agrees to rel_l2 <= 1e-12 (both sides are a
    handful of fp64 roundings), and what the scorer keeps is those folded values rounded ONCE to fp32"""
    from transeditor_amd import pose
    from transeditor_amd.inception_features import fold_bn
    w = sd[f'{key}.weight']
    stats = [sd[f'{bn}.{t}'] for t in R.BN_KEYS]
    x = torch.randn(2, w.shape[1], 13, 11, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    gamma, beta, mean, var = (t.double() for t in stats)
    want = F.batch_norm(F.conv2d(x, w.double(), None, stride, pad), mean, var, gamma, beta, False, 0.0, R.BN_EPS)
    w64, b64 = fold_bn(w, *stats, eps=pose.BN_EPS, dtype=torch.float64)
    assert w64.dtype == torch.float64 and pose.BN_EPS == R.BN_EPS == 1e-5
    e = rel_l2(F.conv2d(x, w64, b64, stride, pad), want)
    print(f'{key}: folded against conv + batch norm, fp64: rel_l2 {e:.3e}')
    assert e <= 1e-12
    wf, bf = pose.parse_state_dict(sd)['convs'][key]
    assert torch.equal(wf, w64.float()) and torch.equal(bf, b64.float())                         # one rounding of the fp64 values
    assert float((wf.double() - w64).abs().max()) > 0                                            # (and the rounding is there)


def test_restatement_shapes(sd):
    x = R.images(1, 2, 70)
    p = R.probabilities(x, sd, torch.float32, 62)
    assert tuple(p.shape) == (2, 2) and float((p.sum(1) - 1).abs().max()) < 1e-5
    assert tuple(R.features(x, sd, torch.float64, 62).shape) == (2, 20)
    assert torch.equal(R.probabilities(scorer_checks.levels(x), sd, torch.float32, 62, preprocessed=True), p)
    cal = R.state_dict(0, widths=SMALL, images=x, crop=62)                                       # calibrated on the images
    lg = R.logits(x, cal, torch.float64, 62)
    assert abs(float((lg - cal['extra_layer.bias'].double()).std()) - 1) < 1e-5                  # the weight: unit spread of f @ w.T
    assert float(lg.mean(0).abs().max()) < 1e-5                                                  # the bias: zero mean per class
    assert torch.equal(cal['backbone.6.0.conv1.weight'], sd['backbone.6.0.conv1.weight'])
    # the module form holds the same network under torchvision's names
    net = R.resnet18(widths=SMALL)
    assert [n for n, _ in net.named_children()] == ['conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4', 'avgpool', 'fc']
    body = torch.nn.Sequential(*list(net.children())[:-1])
    assert {k for k in body.state_dict()} == {k[len('backbone.'):] for k in sd if k.startswith('backbone.')}
    body.load_state_dict({k[len('backbone.'):]: t for k, t in sd.items() if k.startswith('backbone.')})
    body.eval()
    with torch.no_grad():
        f = torch.flatten(body(R.preprocess(x, 62)), 1)
    assert rel_l2(f, R.features(x, sd, torch.float64, 62)) < 1e-5


# ---------------------------------------------------------------------------------------------------------- the drop-in
def test_dropin_estimate_pose(tmp_path, monkeypatch, sd):
    sys.path.insert(0, os.path.join(ROOT, 'dropin'))
    names = ('ffhq_utils', 'ffhq_utils.dex')
    try:
        for n in names:
            sys.modules.pop(n, None)
        dex = importlib.import_module('ffhq_utils.dex')
        assert callable(dex.estimate_pose) and 'estimate_pose' in dex.__doc__ and 'celebahq_utils' in dex.__doc__
        monkeypatch.delenv('TE_DEX_DIR', raising=False)
        with pytest.raises(RuntimeError, match='TE_DEX_DIR'):
            dex.estimate_pose(torch.zeros(1, 3, 256, 256))
        monkeypatch.setenv('TE_DEX_DIR', str(tmp_path))
        with pytest.raises(RuntimeError, match=r'classifier/pose/weight\.pkl not found'):
            dex.estimate_pose(torch.zeros(1, 3, 256, 256))
        with pytest.raises(ValueError, match='estimate_pose'):                                   # eval('pose') still raises, and says where pose is
            dex.eval('pose')
        os.makedirs(tmp_path / 'classifier' / 'pose')
        torch.save(sd, str(tmp_path / 'classifier' / 'pose' / 'weight.pkl'))
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match='needs a GPU'):
                dex.estimate_pose(torch.zeros(1, 3, 256, 256))
        assert dex._scorer('pose').crop == 224 and dex._scorer('pose').widths == SMALL           # loaded once and kept
    finally:
        sys.path.remove(os.path.join(ROOT, 'dropin'))
        for n in names:
            sys.modules.pop(n, None)


# ---------------------------------------------------------------------------------------------------------- the command line, the ABI
def test_command_line():
    from transeditor_amd import pose
    parse = pose.build_parser().parse_args
    a = parse(['--ckpt', 'G.pt', '--weights', 'weight.pkl', '--write_z_boundary', 'zb.npy', '--write_p_boundary', 'pb.npy'])
    assert (a.ckpt, a.weights, a.crop, a.num_sample, a.write_z_boundary, a.write_p_boundary, a.write_scores) == \
        ('G.pt', 'weight.pkl', 224, 10000, 'zb.npy', 'pb.npy', None)
    assert (a.ratio, a.split_ratio, a.truncation, a.size, a.batch, a.seed, a.para_num) == (0.02, 0.7, 0.7, 256, 16, None, 16)
    a = parse(['--ckpt', 'G.pt', '--weights', 'w.pkl', '--crop', '62', '--num_sample', '500', '--write_z_boundary', 'z.npy',
               '--write_p_boundary', 'p.npy', '--write_scores', 's.npy', '--seed', '3', '--batch', '8'])
    assert (a.crop, a.num_sample, a.write_scores, a.seed, a.batch) == (62, 500, 's.npy', 3, 8)
    for bad in (['--ckpt', 'G.pt', '--weights', 'w.pkl', '--write_z_boundary', 'z.npy'],
                ['--weights', 'w.pkl', '--write_z_boundary', 'z.npy', '--write_p_boundary', 'p.npy'],
                ['--ckpt', 'G.pt', '--weights', 'w.pkl', '--attribute', 'pose', '--write_z_boundary', 'z.npy', '--write_p_boundary', 'p.npy']):
        with pytest.raises(SystemExit):
            parse(bad)
    full = ['--ckpt', 'G.pt', '--weights', 'w.pkl', '--write_z_boundary', 'z.npy', '--write_p_boundary', 'p.npy']
    with pytest.raises(SystemExit):
        pose.main(full + ['--size', '48'])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a GPU'):
            pose.main(full)


def test_abi_entry_points_and_argument_checks():
    from transeditor_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    for name in ('te_conv2d_res_f32', 'te_pose_stem_fwd_f32', 'te_maxpool3s2p1_f32'):
        assert name in _lib.EXPORTS and name + '(' in header
    assert 'M7' in header and 'models.py:73-89' in header and 'api.py:61-65' in header and 'resnet.hip' in build.SOURCES
    L = _lib.lib()
    assert L.te_version() == 3
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16                                 # validation only: never dereferenced
    res_args = (1, 3, 4, 8, 8, 3, 3, 1, 1, 1, 1, None)
    assert L.te_conv2d_res_f32(None, None, None, None, None, *res_args) == -1 and b'NULL' in L.te_last_error_string()
    assert L.te_conv2d_res_f32(p, p, p, p, None, *res_args) == -1                            # the residual is not optional
    assert L.te_conv2d_res_f32(p, p, p, p, p, 1, 3, 4, 8, 8, 3, 3, 3, 1, 1, 1, None) == -3 and b'stride' in L.te_last_error_string()
    assert L.te_conv2d_res_f32(p, p, p, p, p, 1, 3, 4, 8, 8, 3, 3, 1, 3, 1, 1, None) == -2
    assert L.te_conv2d_res_f32(p, p, p, p, p, 1, 3, 4, 8, 8, 3, 3, 1, 1, 1, 2, None) == -3
    assert L.te_pose_stem_fwd_f32(None, None, None, None, 1, 40, 40, 32, 8, 0, None) == -1 and b'NULL' in L.te_last_error_string()
    for N, H, W, crop, Co in [(1, 40, 40, 0, 8), (1, 40, 40, 42, 8), (1, 40, 40, 33, 8), (1, 41, 40, 32, 8), (1, 40, 30, 32, 8),
                              (65536, 40, 40, 32, 8), (0, 40, 40, 32, 8), (1, 40, 40, 32, 0)]:
        assert L.te_pose_stem_fwd_f32(p, p, p, p, N, H, W, crop, Co, 0, None) == -2, (N, H, W, crop, Co)
    assert L.te_pose_stem_fwd_f32(p, p, p, p, 1, 40, 40, 32, 8, 2, None) == -3 and b'preprocessed' in L.te_last_error_string()
    assert L.te_maxpool3s2p1_f32(None, None, 3, 8, 8, None) == -1 and b'NULL' in L.te_last_error_string()
    assert L.te_maxpool3s2p1_f32(p, p, 0, 8, 8, None) == -2 and L.te_maxpool3s2p1_f32(p, p, 3, 0, 8, None) == -2

"""Host side of the CelebA-HQ attribute scorer (transeditor_amd.celeba_attr) and of the drop-in celebahq_utils.dex: state dict parsing
and the geometry read from it, the folded scales, the restatement's own conditions for every seed the GPU tests use, the drop-in's
surface, the argument parser and the ABI's argument checks.  No GPU is needed."""
import ctypes
import importlib
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import celeba_attr_restated as R
from conftest import ROOT, load_golden


@pytest.fixture(scope='module')
def sd():
    return R.state_dict(0, 16, fmap_base=128, fmap_max=32)                    # channels 16 / 32


# ---------------------------------------------------------------------------------------------------------- the state dict
def test_geometry_is_read_from_the_shapes(sd):
    from transeditor_amd import celeba_attr
    net = celeba_attr.parse_state_dict(sd)
    assert net['resolution'] == 16 and net['channels'] == (16, 16, 32, 32, 32, 32)
    assert len(net['convs']) == 5 and tuple(net['stem'][0].shape) == (16, 3) and tuple(net['dense0'][0].shape) == (32, 512)
    assert tuple(net['dense1'][0].shape) == (32,) and tuple(net['dense1'][1].shape) == (1,)
    wrapped = celeba_attr.parse_state_dict({'state_dict': sd, 'epoch': 3, 'valacc': 0.9})             # the reference's file content
    assert wrapped['resolution'] == 16 and torch.equal(wrapped['convs'][2][0], net['convs'][2][0])
    extra = dict(sd)
    extra['fromrgb_lod3.conv.conv.weight'], extra['fromrgb_lod3.conv.wscale.b'] = torch.zeros(7, 3, 1, 1), torch.zeros(5)
    assert 'lod_in' in sd and celeba_attr.parse_state_dict(extra)['channels'] == net['channels']     # both ignored
    assert [k for k, _, _, _ in R.layers(16, 128, 32)] == ['fromrgb_lod0.conv', '16x16.conv0', '16x16.conv1', '8x8.conv0', '8x8.conv1',
                                                            '4x4.conv', '4x4.dense0', '4x4.dense1']
    real = [s[0] for _, s, _, _ in R.layers(256)]
    assert real == [64, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 512, 512, 512, 1]       # the real files: 13 3x3 convolutions
    s = celeba_attr.CelebAAttributeScorer(state_dict=sd, name='Smiling')
    assert (s.resolution, s.channels, s.name, s.n_convs, s.training) == (16, net['channels'], 'Smiling', 5, False)
    names = {n for n, _ in s.named_buffers()}
    assert names == {'stem_w', 'stem_b', 'dense0_w', 'dense0_b', 'dense1_w', 'dense1_b'} | {f'{t}{i}' for t in 'wb' for i in range(5)}
    with pytest.raises(RuntimeError, match='eval only'):
        s.train()


def test_scales_are_folded_into_the_weights(sd):
    """the loader multiplies gain / sqrt(fan-in) into the weights; the identity it relies on, conv(x, w) * s + b == conv(x, w * s) + b,
    in fp64, and the constants themselves"""
    from transeditor_amd import celeba_attr
    net = celeba_attr.parse_state_dict(sd)
    assert torch.equal(net['stem'][0], (sd['fromrgb_lod0.conv.conv.weight'] * math.sqrt(2 / 3)).view(16, 3))
    assert torch.equal(net['convs'][1][0], sd['16x16.conv1.conv.weight'] * math.sqrt(2 / (9 * 16)))
    assert torch.equal(net['convs'][4][0], sd['4x4.conv.conv.weight'] * math.sqrt(2 / (9 * 32)))
    assert torch.equal(net['dense0'][0], sd['4x4.dense0.linear.weight'] * math.sqrt(2 / 512))
    assert torch.equal(net['dense1'][0], (sd['4x4.dense1.linear.weight'] * math.sqrt(1 / 32)).view(32))        # gain 1
    assert torch.equal(net['convs'][0][1], sd['16x16.conv0.wscale.b'])
    g = torch.Generator().manual_seed(1)
    x, w, b = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((2, 16, 8, 8), (32, 16, 3, 3), (32,)))
    s = math.sqrt(2 / (9 * 16))
    a, c = F.conv2d(x, w, padding=1) * s + b.view(1, -1, 1, 1), F.conv2d(x, w * s, b, padding=1)
    assert float((a - c).abs().max()) < 1e-13 * float(a.abs().max())
    h, wl = torch.randn(3, 64, generator=g, dtype=torch.float64), torch.randn(8, 64, generator=g, dtype=torch.float64)
    assert float((F.linear(h, wl) * 0.125 - F.linear(h, wl * 0.125)).abs().max()) == 0.0


def test_state_dict_validation(sd, tmp_path):
    from transeditor_amd.celeba_attr import CelebAAttributeScorer
    for key in ('fromrgb_lod0.conv.conv.weight', 'fromrgb_lod0.conv.wscale.b', '16x16.conv1.conv.weight', '8x8.conv0.wscale.b',
                '8x8.conv1.conv.weight', '4x4.conv.conv.weight', '4x4.dense0.linear.weight', '4x4.dense1.wscale.b'):
        bad = dict(sd)
        del bad[key]
        with pytest.raises(ValueError, match='has no ' + key.rsplit('.', 2)[0].replace('.', r'\.')):
            CelebAAttributeScorer(state_dict=bad)
    bad = dict(sd)
    del bad['8x8.conv0.conv.weight']                                                               # a hole in the pyramid
    with pytest.raises(ValueError, match=r'has no 8x8\.conv0\.conv\.weight / 8x8\.conv0\.wscale\.b'):
        CelebAAttributeScorer(state_dict=bad)
    with pytest.raises(ValueError, match=r'has no \{r\}x\{r\}\.conv0\.conv\.weight'):
        CelebAAttributeScorer(state_dict={'lod_in': torch.tensor(0.0)})
    bad = dict(sd)
    bad['8x8.conv0.conv.weight'] = torch.zeros(32, 24, 3, 3)                                       # a broken channel chain
    with pytest.raises(ValueError, match=r'8x8\.conv0\.conv\.weight is \(32, 24, 3, 3\) / bias \(32,\), expected \(\*, 32, 3, 3\)'):
        CelebAAttributeScorer(state_dict=bad)
    bad = dict(sd)
    bad['16x16.conv1.wscale.b'] = torch.zeros(31)
    with pytest.raises(ValueError, match=r'16x16\.conv1\.conv\.weight is \(32, 16, 3, 3\) / bias \(31,\)'):
        CelebAAttributeScorer(state_dict=bad)
    bad = dict(sd)
    bad['fromrgb_lod0.conv.conv.weight'] = torch.zeros(16, 3, 3, 3)
    with pytest.raises(ValueError, match=r'fromrgb_lod0\.conv\.conv\.weight is \(16, 3, 3, 3\)'):
        CelebAAttributeScorer(state_dict=bad)
    bad = dict(sd)
    bad['4x4.dense0.linear.weight'] = torch.zeros(32, 32 * 9)                                      # not C * 16 inputs
    with pytest.raises(ValueError, match=r'4x4\.dense0\.linear\.weight is \(32, 288\) / bias \(32,\), expected \(\*, 512\)'):
        CelebAAttributeScorer(state_dict=bad)
    bad = dict(sd)
    bad['4x4.dense1.linear.weight'], bad['4x4.dense1.wscale.b'] = torch.zeros(2, 32), torch.zeros(2)           # two outputs
    with pytest.raises(ValueError, match=r'4x4\.dense1\.linear\.weight is \(2, 32\) / bias \(2,\), expected \(1, 32\)'):
        CelebAAttributeScorer(state_dict=bad)
    bad = dict(sd)
    bad['24x24.conv0.conv.weight'], bad['24x24.conv0.wscale.b'] = torch.zeros(16, 16, 3, 3), torch.zeros(16)    # not a power of two
    with pytest.raises(ValueError, match=r'24x24\.conv0\.conv\.weight, expected a power of two >= 8'):
        CelebAAttributeScorer(state_dict=bad)
    with pytest.raises(ValueError, match=r'4x4\.conv0\.conv\.weight, expected a power of two >= 8'):
        CelebAAttributeScorer(state_dict={'4x4.conv0.conv.weight': torch.zeros(8, 8, 3, 3)})
    p = str(tmp_path / 'net_best.pth')
    torch.save({'state_dict': bad, 'epoch': 1, 'valacc': 0.5}, p)
    with pytest.raises(ValueError, match='24x24'):
        CelebAAttributeScorer(p)
    with pytest.raises(ValueError, match='not both'):
        CelebAAttributeScorer(p, state_dict=sd)
    with pytest.raises(ValueError, match='must be a dict'):
        CelebAAttributeScorer(state_dict=[1])
    with pytest.raises(FileNotFoundError, match='absent.pth'):
        CelebAAttributeScorer(str(tmp_path / 'absent.pth'))
    torch.save({'state_dict': sd, 'epoch': 1, 'valacc': 0.5}, p)
    assert CelebAAttributeScorer(p).resolution == 16


def test_scorer_input_checks_and_no_cpu_path(sd):
    from transeditor_amd.celeba_attr import CelebAAttributeScorer
    s = CelebAAttributeScorer(state_dict=sd)
    with pytest.raises(ValueError, match=r'\[B,3,S,S\]'):
        s(torch.zeros(1, 1, 16, 16))
    with pytest.raises(ValueError, match='square'):
        s(torch.zeros(1, 3, 16, 32))
    with pytest.raises(ValueError, match='multiple of the resolution 16'):
        s(torch.zeros(1, 3, 24, 24))
    with pytest.raises(ValueError, match='multiple of the resolution 16'):
        s(torch.zeros(1, 3, 8, 8))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a GPU'):
            s(torch.zeros(1, 3, 16, 16))
        with pytest.raises(RuntimeError, match='needs a GPU'):
            s.logits(torch.zeros(1, 3, 32, 32), preprocessed=True)


# ---------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_preprocessing_and_score():
    x = R.images(1, 2, 32)
    v = R.preprocess(x)
    assert tuple(v.shape) == (2, 3, 32, 32) and float(v.min()) == 0 and float(v.max()) == 255 and bool((v == v.round()).all())
    assert torch.equal(v, ((x[:, [2, 1, 0]].clamp(-1, 1) + 1) / 2 * 255).round())
    assert torch.equal(R.box_mean(v, 32), v) and torch.equal(R.box_mean(v, 16), F.avg_pool2d(v, 2, 2))
    sd = R.state_dict(0, 16, 128, 32)
    l = R.logits(x, sd, torch.float32)
    assert tuple(l.shape) == (2,) and torch.equal(R.logits(v, sd, torch.float32, preprocessed=True), l)
    s = R.score_of(torch.tensor([0.0, 1.0, -1.0], dtype=torch.float64))
    assert s[0] == 0.5 and abs(float(s[1]) - 1 / (1 + math.exp(2))) < 1e-15 and abs(float(s[1] + s[2]) - 1) < 1e-15       # decreasing in l
    assert float(sd['4x4.dense1.linear.weight'].std()) < 2 / 255                                   # dense1 / 255


@pytest.mark.parametrize('name', list(R.CASES))
def test_restatement_conditions_hold_for_the_gpu_cases(name):
    """every fp64 score in (0.05, 0.95), a logit spread of at least 0.1 across the batch, the clamp live on both sides: for the seeds
    tests/test_gpu_celeba_attr.py uses"""
    l64, l32 = R.case_reference(name)
    f = R.conditions(l64, R.case_images(R.CASES[name]))
    yard = float((l32.double() - l64).norm() / l64.norm())
    print(f'{name}: {f}, fp32 torch against fp64 {yard:.3e}')
    assert 0 < yard < 1e-5


@pytest.mark.parametrize('name', list(R.GOLDEN))
def test_restatement_conditions_hold_for_the_golden_cases(name):
    """the same on the stored fp64 logits of tests/golden/celeba_attr_ref.npz (the true geometry takes seconds in fp64: not rerun)"""
    z, c = load_golden('celeba_attr_ref'), R.GOLDEN[name]
    assert {k: int(z[f'{name}_{k}']) for k in c} == c
    R.conditions(z[f'{name}_logit64'], R.case_images(c))
    assert torch.allclose(R.score_of(z[f'{name}_logit'].double()).float(), z[f'{name}_score'], rtol=0, atol=1e-6)
    if name == 'small':
        assert torch.allclose(R.logits(R.case_images(c), R.case_state_dict(c), torch.float64), z[f'{name}_logit64'], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------- the drop-in
def test_dropin_surface_and_named_errors(tmp_path, monkeypatch, sd):
    sys.path.insert(0, os.path.join(ROOT, 'dropin'))
    names = ('celebahq_utils', 'celebahq_utils.dex')
    try:
        for n in names:
            sys.modules.pop(n, None)
        dex = importlib.import_module('celebahq_utils.dex')
        assert dex.__file__ == os.path.join(ROOT, 'dropin', 'celebahq_utils', 'dex.py')
        assert callable(dex.eval) and callable(dex.estimate_score)
        monkeypatch.delenv('TE_CELEBA_ATTR_DIR', raising=False)
        with pytest.raises(RuntimeError, match='TE_CELEBA_ATTR_DIR'):
            dex.eval('Smiling')
        monkeypatch.setenv('TE_CELEBA_ATTR_DIR', str(tmp_path))
        with pytest.raises(RuntimeError, match=r'Smiling.net_best\.pth not found'):
            dex.eval('Smiling')
        os.makedirs(tmp_path / 'Wavy_Hair')
        torch.save({'state_dict': sd, 'epoch': 1, 'valacc': 0.5}, str(tmp_path / 'Wavy_Hair' / 'net_best.pth'))
        classifier = dex.eval('Wavy_Hair')                                                         # loads; the scorer is kept
        assert classifier.name == 'Wavy_Hair' and classifier.resolution == 16 and dex.eval('Wavy_Hair') is classifier
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match='needs a GPU'):
                dex.estimate_score(classifier, torch.zeros(1, 3, 16, 16), no_soft=True)
        ffhq = open(os.path.join(ROOT, 'dropin', 'ffhq_utils', 'dex.py')).read()
        assert 'celebahq_utils' in ffhq and 'no CelebA' not in ffhq
    finally:
        sys.path.remove(os.path.join(ROOT, 'dropin'))
        for n in names:
            sys.modules.pop(n, None)


def test_load_scorers(tmp_path, sd):
    from transeditor_amd.celeba_attr import load_scorers
    for name in ('Male', 'Bangs'):
        os.makedirs(tmp_path / name)
        torch.save({'state_dict': sd, 'epoch': 1, 'valacc': 0.5}, str(tmp_path / name / 'net_best.pth'))
    scorers = load_scorers(str(tmp_path), ['Bangs', 'Male'])
    assert list(scorers) == ['Bangs', 'Male'] and [s.name for s in scorers.values()] == ['Bangs', 'Male']
    with pytest.raises(FileNotFoundError, match='Smiling'):
        load_scorers(str(tmp_path), ['Male', 'Smiling'])


# ---------------------------------------------------------------------------------------------------------- the command line, the ABI
def test_command_line():
    from transeditor_amd import celeba_attr
    parse = celeba_attr.build_parser().parse_args
    a = parse(['--ckpt', 'G.pt', '--weights', 'net_best.pth', '--write_z_boundary', 'zb.npy', '--write_p_boundary', 'pb.npy'])
    assert (a.ckpt, a.weights, a.name, a.num_sample, a.write_z_boundary, a.write_p_boundary, a.write_scores, a.no_soft) == \
        ('G.pt', 'net_best.pth', None, 10000, 'zb.npy', 'pb.npy', None, False)
    assert (a.ratio, a.split_ratio, a.truncation, a.size, a.batch, a.seed, a.para_num) == (0.02, 0.7, 0.7, 256, 16, None, 16)
    a = parse(['--ckpt', 'G.pt', '--weights', 'w.pth', '--name', 'Smiling', '--num_sample', '500', '--write_z_boundary', 'z.npy',
               '--write_p_boundary', 'p.npy', '--write_scores', 's.npy', '--no_soft', '--seed', '3', '--batch', '8'])
    assert (a.name, a.num_sample, a.write_scores, a.no_soft, a.seed, a.batch) == ('Smiling', 500, 's.npy', True, 3, 8)
    for bad in (['--ckpt', 'G.pt', '--weights', 'w.pth', '--write_z_boundary', 'z.npy'],
                ['--weights', 'w.pth', '--write_z_boundary', 'z.npy', '--write_p_boundary', 'p.npy'],
                ['--ckpt', 'G.pt', '--write_z_boundary', 'z.npy', '--write_p_boundary', 'p.npy']):
        with pytest.raises(SystemExit):
            parse(bad)
    full = ['--ckpt', 'G.pt', '--weights', 'w.pth', '--write_z_boundary', 'z.npy', '--write_p_boundary', 'p.npy']
    with pytest.raises(SystemExit):
        celeba_attr.main(full + ['--size', '48'])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a GPU'):
            celeba_attr.main(full)


def test_abi_entry_points_and_argument_checks():
    from transeditor_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    for name in ('te_attr_stem_fwd_f32', 'te_avgpool2_act_f32', 'te_attr_score_f32'):
        assert name in _lib.EXPORTS and name + '(' in header
    assert 'M6' in header and 'attribute_classifier.py:152-215' in header and 'attribute_utils.py:28-32' in header
    L = _lib.lib()
    assert L.te_version() == 3
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16                                  # validation only: never dereferenced
    assert L.te_attr_stem_fwd_f32(None, p, p, p, 1, 64, 32, 16, 0, None) == -1 and b'NULL' in L.te_last_error_string()
    for N, S, R_, C0 in [(1, 48, 32, 16), (1, 16, 32, 16), (1, 0, 32, 16), (1, 64, 0, 16), (1, 64, 32, 0), (1, 64, 32, 1025), (0, 64, 32, 16),
                         (65536, 64, 32, 16)]:
        assert L.te_attr_stem_fwd_f32(p, p, p, p, N, S, R_, C0, 0, None) == -2, (N, S, R_, C0)
    assert L.te_attr_stem_fwd_f32(p, p, p, p, 1, 64, 32, 16, 2, None) == -3 and b'preprocessed' in L.te_last_error_string()
    assert L.te_avgpool2_act_f32(p, None, 4, 8, 8, 0.2, None) == -1
    for planes, H, W in [(4, 7, 8), (4, 8, 7), (0, 8, 8), (4, 0, 8), (4, 8, 0), (1 << 40, 2, 2)]:
        assert L.te_avgpool2_act_f32(p, p, planes, H, W, 0.2, None) == -2, (planes, H, W)
    assert L.te_attr_score_f32(None, None, p, p, p, 3, 8, 0.2, None) == -1
    assert L.te_attr_score_f32(p, None, p, p, None, 3, 8, 0.2, None) == -1
    for I, K in [(3, 6), (3, 0), (0, 8), (1 << 31, 8)]:
        assert L.te_attr_score_f32(p, p, p, p, p, I, K, 0.2, None) == -2, (I, K)
    assert L.te_attr_score_f32(p, None, p + 4, p, p, 3, 8, 0.2, None) == -2 and b'16-byte aligned' in L.te_last_error_string()
    assert L.te_attr_score_f32(None, p, p, p + 8, p, 3, 8, 0.2, None) == -2

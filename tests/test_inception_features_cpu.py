"""Host side of the Inception-v3 pool3 feature extractor (transeditor_amd.inception_features), of the FID command line's dataset and
checkpoint modes and of the drop-in metrics.inception: state dict validation, the batch norm fold, the restatement's shape walk, the
argument parser, and the ABI's argument checks.  No GPU is needed."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

import inception_restated as R
from conftest import ROOT


@pytest.fixture(scope='module')
def sd():
    return R.state_dict(0)


def _dropin():
    spec = importlib.util.spec_from_file_location('te_dropin_metrics_inception', os.path.join(ROOT, 'dropin', 'metrics', 'inception.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_layer_table_matches_the_restatement():
    from transeditor_amd import inception_features as IF
    assert len(IF.LAYERS) == 94 and len(R.SHAPES) == 94
    for name, ci, co, k, stride, pad in IF.LAYERS:
        assert R.SHAPES[name] == (ci, co, *k), name
        assert stride in (1, 2) and pad[0] < k[0] and pad[1] < k[1]


def test_state_dict_validation(sd, tmp_path, monkeypatch):
    from transeditor_amd.inception_features import WEIGHTS_FILE, InceptionV3Features, default_inception_path
    bad = dict(sd)
    del bad['Mixed_6c.branch7x7dbl_3.bn.running_var']
    with pytest.raises(ValueError, match='has no Mixed_6c.branch7x7dbl_3.bn.running_var'):
        InceptionV3Features(state_dict=bad)
    bad = dict(sd)
    del bad['Mixed_7a.branch3x3_2.conv.weight']
    with pytest.raises(ValueError, match='has no Mixed_7a.branch3x3_2.conv.weight'):
        InceptionV3Features(state_dict=bad)
    bad = dict(sd)
    bad['Mixed_6b.branch7x7_2.conv.weight'] = torch.zeros(128, 128, 7, 1)                    # (1, 7) transposed
    with pytest.raises(ValueError, match=r'Mixed_6b.branch7x7_2.conv.weight is \(128, 128, 7, 1\), expected \(128, 128, 1, 7\)'):
        InceptionV3Features(state_dict=bad)
    bad = dict(sd)
    bad['Conv2d_1a_3x3.bn.bias'] = torch.zeros(31)
    with pytest.raises(ValueError, match=r'Conv2d_1a_3x3.bn.bias is \(31,\), expected \(32,\)'):
        InceptionV3Features(state_dict=bad)
    p = str(tmp_path / 'w.pth')
    torch.save(bad, p)
    with pytest.raises(ValueError, match='expected'):
        InceptionV3Features(p)
    with pytest.raises(ValueError, match='not both'):
        InceptionV3Features(p, state_dict=sd)
    with pytest.raises(ValueError, match='must be a dict'):
        InceptionV3Features(state_dict=[1])
    absent = str(tmp_path / 'absent.pth')
    with pytest.raises(FileNotFoundError, match='absent.pth'):
        InceptionV3Features(absent)
    monkeypatch.setattr(torch.hub, 'get_dir', lambda: str(tmp_path / 'hub'))
    assert default_inception_path() == os.path.join(str(tmp_path / 'hub'), 'checkpoints', WEIGHTS_FILE)
    with pytest.raises(FileNotFoundError, match=WEIGHTS_FILE):                               # the default path, named in full
        InceptionV3Features()


def test_ignored_keys_and_buffers(sd):
    from transeditor_amd.inception_features import InceptionV3Features
    more = dict(sd)
    more['fc.weight'], more['AuxLogits.conv0.conv.weight'] = torch.zeros(3, 3), torch.zeros(1)      # wrong shapes: never looked at
    net = InceptionV3Features(state_dict=more, resize_input=False)
    names = {n for n, _ in net.named_buffers()}
    assert len(names) == 188 and {'w0', 'b0', 'w93', 'b93'} <= names
    assert tuple(net.w0.shape) == (32, 3, 3, 3) and tuple(net.w93.shape) == (192, 2048, 1, 1)
    assert not net.training and net.resize_input is False
    with pytest.raises(ValueError, match=r'\[B,3,H,W\]'):
        net(torch.zeros(1, 1, 80, 80))
    with pytest.raises(ValueError, match='at least 75'):
        net(torch.zeros(1, 3, 74, 80))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='GPU'):
            net(torch.zeros(1, 3, 80, 80))


def test_bn_fold_against_fp64(sd):
    """conv(x, w') + b' in fp64 with the folded fp32 parameters against conv -> batch norm in fp64 with the originals: the fold is exact
    up to its one rounding to fp32 (2^-24 relative on each of w' and b')"""
    from transeditor_amd.inception_features import BN_EPS, fold_bn
    n = 'Mixed_6b.branch7x7_2'
    w, ga, be, mu, var = (sd[f'{n}.{k}'] for k in ('conv.weight', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var'))
    wf, bf = fold_bn(w, ga, be, mu, var)
    assert wf.dtype == torch.float32 and bf.dtype == torch.float32 and wf.shape == w.shape and bf.shape == (128,)
    g = ga.double() / torch.sqrt(var.double() + BN_EPS)
    assert torch.equal(wf, (w.double() * g.view(-1, 1, 1, 1)).float()) and torch.equal(bf, (be.double() - mu.double() * g).float())
    x = torch.randn(2, 128, 5, 9, generator=torch.Generator().manual_seed(1)).double()
    ref = F.batch_norm(F.conv2d(x, w.double(), padding=(0, 3)), mu.double(), var.double(), ga.double(), be.double(), False, 0.0, BN_EPS)
    got = F.conv2d(x, wf.double(), bf.double(), padding=(0, 3))
    bound = 2.0 ** -24 * (F.conv2d(x.abs(), wf.double().abs(), bf.double().abs(), padding=(0, 3)))
    assert bool(((got - ref).abs() <= 1.01 * bound).all())


def test_restatement_shape_walk(sd):
    x = torch.rand(1, 3, 64, 48, generator=torch.Generator().manual_seed(2)) * 2 - 1
    h = R.mixed_7c(x, sd, torch.float32)                                                     # resized to 299 x 299
    assert tuple(h.shape) == (1, 2048, 8, 8)
    small = R.mixed_7c(torch.zeros(1, 3, 75, 75), sd, torch.float32, resize_input=False)
    assert tuple(small.shape) == (1, 2048, 1, 1)
    f = R.pool3(torch.zeros(2, 3, 75, 91), sd, torch.float32, resize_input=False)
    assert tuple(f.shape) == (2, 2048) and f.dtype == torch.float32


def test_command_line_modes():
    from transeditor_amd import fid
    parse = fid.build_parser().parse_args
    a = parse(['--dataset', 'lmdb', '--inception', 'w.pth', '--write_stats', 'o.pkl'])
    assert (a.mode, a.dataset, a.inception, a.write_stats) == ('dataset', 'lmdb', 'w.pth', 'o.pkl')
    assert (a.size, a.n_sample, a.batch, a.seed, a.flip) == (256, 50000, 64, None, False)      # calc_inception.py's defaults
    a = parse(['--ckpt', 'c.pt', '--stats', 's.pkl', '--inception', 'w.pth'])
    assert (a.mode, a.ckpt, a.stats, a.dataset, a.inception) == ('model', 'c.pt', 's.pkl', None, 'w.pth')
    assert (a.truncation, a.para_num, a.num_trans, a.channel_multiplier, a.start_num) == (1.0, 16, 8, 2, 0)      # fid_query.py's defaults
    a = parse(['--ckpt', 'c.pt', '--dataset', 'lmdb', '--size', '64', '--n_sample', '100', '--batch', '8', '--seed', '2',
               '--truncation', '0.5'])
    assert (a.mode, a.stats, a.dataset, a.size, a.n_sample, a.batch, a.seed, a.truncation, a.inception) == \
        ('model', None, 'lmdb', 64, 100, 8, 2, 0.5, None)
    assert parse(['--real', 'r.npy', '--fake', 'f.npy']).mode == 'files'                       # the three feature-file modes are as before
    assert parse(['--stats', 's.pkl', '--fake', 'f.npy']).mode == 'stats'
    assert parse(['--features', 'r.npy', '--write_stats', 'o.pkl']).mode == 'write'
    for bad in (['--ckpt', 'c.pt'], ['--dataset', 'lmdb'], ['--inception', 'w.pth'],
                ['--ckpt', 'c.pt', '--stats', 's.pkl', '--dataset', 'lmdb'], ['--ckpt', 'c.pt', '--stats', 's.pkl', '--fake', 'f.npy'],
                ['--ckpt', 'c.pt', '--stats', 's.pkl', '--write_stats', 'o.pkl'], ['--ckpt', 'c.pt', '--stats', 's.pkl', '--size', '48'],
                ['--dataset', 'lmdb', '--write_stats', 'o.pkl', '--features', 'r.npy'],
                ['--dataset', 'lmdb', '--write_stats', 'o.pkl', '--stats', 's.pkl'],
                ['--real', 'r.npy', '--fake', 'f.npy', '--inception', 'w.pth'],
                ['--features', 'r.npy', '--write_stats', 'o.pkl', '--inception', 'w.pth']):
        with pytest.raises(SystemExit):
            parse(bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a GPU'):
            fid.main(['--ckpt', 'c.pt', '--stats', 's.pkl'])
        with pytest.raises(RuntimeError, match='needs a GPU'):
            fid.main(['--dataset', 'lmdb', '--write_stats', 'o.pkl'])


def test_dropin_refusals(tmp_path, monkeypatch):
    D = _dropin()
    for kw in (dict(output_blocks=[2]), dict(output_blocks=[0, 3]), dict(output_blocks=[3], use_fid_inception=False),
               dict(output_blocks=[3], requires_grad=True)):
        with pytest.raises(ValueError, match='InceptionV3'):
            D.InceptionV3(**kw)
    monkeypatch.setattr(torch.hub, 'get_dir', lambda: str(tmp_path / 'hub'))                  # valid arguments: the weights are looked up
    with pytest.raises(FileNotFoundError, match='pt_inception-2015-12-05-6726825d.pth'):
        D.InceptionV3([3], normalize_input=False)
    assert D.InceptionV3.DEFAULT_BLOCK_INDEX == 3 and D.InceptionV3.BLOCK_INDEX_BY_DIM[2048] == 3


def test_abi_entry_points_and_argument_checks():
    from transeditor_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    for name in ('te_conv2d_f32', 'te_pool3_f32', 'te_resize_bilinear_f32'):
        assert name in _lib.EXPORTS and name + '(' in header
    assert 'inception.py:147-150' in header and 'calc_inception.py:55' in header
    L = _lib.lib()
    assert L.te_version() == 3
    null = (None, None, None, None)
    assert L.te_conv2d_f32(*null, 1, 3, 4, 8, 8, 3, 3, 1, 0, 0, 4, 0, 0, None) == -1
    assert b'NULL' in L.te_last_error_string()
    assert L.te_pool3_f32(None, None, 1, 2, 8, 8, 0, 2, 0, None) == -1
    assert L.te_resize_bilinear_f32(None, None, 3, 8, 8, 16, 16, None) == -1
    assert _lib.conv2d_out_hw(299, 299, 3, 3, 2) == (149, 149) and _lib.conv2d_out_hw(17, 17, 1, 7, 1, (0, 3)) == (17, 17)
    assert _lib.conv2d_out_hw(9, 11, 3, 3, 2) == (4, 5)

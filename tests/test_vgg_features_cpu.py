"""Host side of the VGG16 fc7 feature extractor (transeditor_amd.vgg_features) and of the PRDC command line's checkpoint mode: state
dict validation, the argument parser, dataset_features' sampling, and the ABI's argument checks.  No GPU is needed."""
import pytest
import torch

import vgg_restated as R


def _full_cpu_state_dict():
    """valid shapes throughout; the classifier weights are uninitialised memory (only their shapes are read here)"""
    sd = R.conv_state_dict(0)
    for idx, j, k in R.FC:
        sd[f'classifier.{idx}.weight'] = torch.empty(j, k)
        sd[f'classifier.{idx}.bias'] = torch.zeros(j)
    return sd


def test_state_dict_validation(tmp_path):
    from transeditor_amd.vgg_features import VGG16Features
    sd = R.conv_state_dict(0)
    with pytest.raises(ValueError, match='classifier.0.weight'):
        VGG16Features(state_dict=sd)
    sd['classifier.0.weight'], sd['classifier.0.bias'] = torch.zeros(2, 2), torch.zeros(2)
    with pytest.raises(ValueError, match=r'classifier.0.weight is \(2, 2\).*expected \(4096, 25088\)'):
        VGG16Features(state_dict=sd)
    p = str(tmp_path / 'vgg16.pth')
    torch.save(sd, p)
    with pytest.raises(ValueError, match='expected'):
        VGG16Features(p)
    del sd['features.28.bias']
    with pytest.raises(ValueError, match='features.28.weight / features.28.bias'):
        VGG16Features(state_dict=sd)
    with pytest.raises(FileNotFoundError, match='VGG16Features: vgg16 file not found'):
        VGG16Features(str(tmp_path / 'absent.pth'))
    with pytest.raises(ValueError, match='not both'):
        VGG16Features(p, state_dict=sd)


def test_logits_layer_is_ignored():
    from transeditor_amd.vgg_features import VGG16Features
    sd = _full_cpu_state_dict()
    sd['classifier.6.weight'], sd['classifier.6.bias'] = torch.zeros(3, 3), torch.zeros(5)      # wrong shapes: never looked at
    net = VGG16Features(state_dict=sd)
    names = {n for n, _ in net.named_buffers()}
    assert {'w0', 'b12', 'fc6_w', 'fc6_b', 'fc7_w', 'fc7_b'} <= names and len(names) == 30
    assert tuple(net.fc6_w.shape) == (4096, 25088) and tuple(net.fc7_w.shape) == (4096, 4096)
    assert not net.training
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='GPU'):
            net(torch.zeros(1, 3, 64, 64))


def test_command_line_modes():
    from transeditor_amd import prdc
    parse = prdc.build_parser().parse_args
    a = parse(['--real', 'r.npy', '--fake', 'f.npy'])
    assert a.mode == 'files'
    a = parse(['--ckpt', 'c.pt', '--dataset', 'lmdb', '--size', '256', '--vgg16', 'v.pth'])
    assert (a.mode, a.ckpt, a.dataset, a.size, a.vgg16) == ('model', 'c.pt', 'lmdb', 256, 'v.pth')
    assert (a.n_sample, a.batch, a.nearest_k, a.seed) == (50000, 64, 3, None)                  # calc_prdc.py's defaults
    a = parse(['--ckpt', 'c.pt', '--dataset', 'lmdb', '--n_sample', '100', '--batch', '8', '--nearest_k', '5', '--seed', '2'])
    assert (a.n_sample, a.batch, a.nearest_k, a.seed, a.vgg16) == (100, 8, 5, 2, None)
    for bad in (['--ckpt', 'c.pt'], ['--dataset', 'lmdb'], ['--fake', 'f.npy'], [],
                ['--real', 'r.npy', '--fake', 'f.npy', '--ckpt', 'c.pt', '--dataset', 'lmdb'],
                ['--real', 'r.npy', '--fake', 'f.npy', '--dataset', 'lmdb'], ['--real', 'r.npy', '--ckpt', 'c.pt', '--dataset', 'lmdb'],
                ['--ckpt', 'c.pt', '--dataset', 'lmdb', '--size', '48']):
        with pytest.raises(SystemExit):
            parse(bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='GPU'):
            prdc.main(['--ckpt', 'c.pt', '--dataset', 'lmdb'])


def test_dataset_features_sampling():
    from transeditor_amd import prdc
    data = [torch.full((3, 4, 4), float(i)) for i in range(23)]
    seen = []

    def feature_fn(x):
        seen.append(x.shape[0])
        return x.mean((2, 3))                               # [B,3]: the item's index, three times

    def ids(**kw):
        f = prdc.dataset_features(data, feature_fn, device='cpu', **kw)
        assert f.shape == (kw['n_sample'], 3) and f.dtype == torch.float32
        return [int(v) for v in f[:, 0].tolist()]
    full = ids(n_sample=23, batch=8, seed=4)
    assert seen == [8, 8, 7]                                # the last batch is the shorter one
    assert sorted(full) == list(range(23)) and full != list(range(23))      # a permutation, not the identity
    assert ids(n_sample=23, batch=8, seed=4) == full
    assert ids(n_sample=23, batch=8, seed=5) != full
    part = ids(n_sample=10, batch=4, seed=4)
    assert part == full[:10] and len(set(part)) == 10       # the head of the same permutation: no image twice
    assert sorted(ids(n_sample=23, batch=64)) == list(range(23))            # unseeded: still without replacement
    with pytest.raises(ValueError, match='n_sample'):
        prdc.dataset_features(data, feature_fn, n_sample=24, batch=8, device='cpu')
    with pytest.raises(ValueError, match='n_sample'):
        prdc.dataset_features(data, feature_fn, n_sample=0, batch=8, device='cpu')
    with pytest.raises(ValueError, match=r'\[B,D\]'):
        prdc.dataset_features(data, lambda x: x.mean((1, 2, 3)), n_sample=4, batch=4, device='cpu')


def test_real_image_transform():
    from PIL import Image
    from transeditor_amd import prdc
    img = Image.new('RGB', (64, 64), (255, 0, 127))
    t = prdc.real_image_transform(64)(img)
    assert t.shape == (3, 64, 64) and t.dtype == torch.float32
    assert float(t[0].min()) == 1.0 and float(t[1].max()) == -1.0 and abs(float(t[2, 0, 0]) - (127 / 255 * 2 - 1)) < 1e-6
    assert prdc.real_image_transform(32)(Image.new('RGB', (96, 64))).shape == (3, 32, 32)      # resized on the short side, cropped


def test_abi_entry_points_and_argument_checks():
    from transeditor_amd import _lib
    for name in ('te_fc_stream_f32', 'te_fc_stream_ws_bytes', 'te_fc_stream_splits', 'te_adaptive_avgpool_f32', 'te_vgg_stem_fwd_f32'):
        assert name in _lib.EXPORTS
    L = _lib.lib()
    assert L.te_version() == 3
    for J, K in ((4096, 25088), (4096, 4096), (40, 8), (130, 4096), (1, 4)):
        S = L.te_fc_stream_splits(J, K)
        assert 1 <= S <= K // 4 and S <= 32
        assert L.te_fc_stream_ws_bytes(1, J, K) == S * J * 4 and L.te_fc_stream_ws_bytes(64, J, K) == 64 * S * J * 4
    assert L.te_fc_stream_splits(4096, 25088) * 64 >= 256                       # fc6's 64 strips alone would leave CUs idle
    assert L.te_fc_stream_splits(4, 6) < 0 and L.te_fc_stream_splits(4, 0) < 0 and L.te_fc_stream_splits(0, 8) < 0
    assert L.te_fc_stream_ws_bytes(0, 4, 8) < 0
    assert L.te_fc_stream_f32(None, None, None, None, None, 3, 4, 8, 0, None) == -1
    assert b'NULL' in L.te_last_error_string()
    assert L.te_adaptive_avgpool_f32(None, None, 6, 8, 8, 7, 7, None) == -1
    assert L.te_vgg_stem_fwd_f32(None, None, None, None, 1, 32, 32, None) == -1

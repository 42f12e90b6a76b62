"""Host side of the ArcFace identity network (transeditor_amd.arcface) and of the identity figures of transeditor_amd.edit_eval, without a
GPU: the state dict parser and its messages, the folded form the kernels run against the unfolded restatement in fp64 (which pins the
affine-gather design: border pixels included), the affine-less output_layer.4, identity_ratio against a literal loop restatement of
our_interfaceGAN/calculate_score_id.py:58-90, identity_similarity, the command line and the build."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import arcface_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = [(16, 16, 2), (16, 16, 1), (16, 32, 2), (32, 32, 1)]
S, BOX, POOL, DIM = 64, (8, 56, 8, 56), 32, 64


@pytest.fixture(scope='module')
def small():
    x = R.images(101, 3, S)
    return x, R.state_dict(3, units=UNITS, images=x, box=BOX, pool=POOL, dim=DIM, reduction=4)


# ---------------------------------------------------------------------------------------------------------- the parser
def test_parse_state_dict_reads_the_geometry(small):
    from transeditor_amd import arcface
    _, sd = small
    net = arcface.parse_state_dict(sd, pool=POOL)
    assert [(u['cin'], u['depth'], u['stride']) for u in net['units']] == UNITS and net['side'] == 8 and net['affine']
    assert all(u['fc1'].shape == (u['depth'] // 4, u['depth']) and u['fc2'].shape == (u['depth'], u['depth'] // 4) for u in net['units'])
    assert [u['sc'] is not None for u in net['units']] == [False, False, True, False]
    assert net['keys'] == {k for k in sd if not k.endswith('num_batches_tracked')}
    assert net['fc'][0].shape == (DIM, 32 * 8 * 8) and net['fc'][0].dtype == torch.float32
    # an explicit list with other strides that the keys still describe (the Linear then expects another plane)
    other = [(16, 16, 1), (16, 16, 2), (16, 32, 2), (32, 32, 1)]
    assert [u['stride'] for u in arcface.parse_state_dict(sd, units=other, pool=POOL)['units']] == [1, 2, 2, 1]
    ir = R.state_dict(3, units=UNITS, pool=POOL, dim=DIM, se=False)
    assert all(u['fc1'] is None for u in arcface.parse_state_dict(ir, pool=POOL)['units'])
    assert arcface.default_units() == R.UNITS50 and len(R.UNITS50) == 24


def test_parse_state_dict_messages(small):
    from transeditor_amd import arcface
    _, sd = small

    def without(*keys, **put):
        out = {k: v for k, v in sd.items() if k not in keys}
        out.update(put)
        return out
    with pytest.raises(ValueError, match=r'has no body\.2\.res_layer\.4\.running_var'):
        arcface.parse_state_dict(without('body.2.res_layer.4.running_var'), pool=POOL)
    with pytest.raises(ValueError, match=r'has no input_layer\.2\.weight'):
        arcface.parse_state_dict(without('input_layer.2.weight'), pool=POOL)
    with pytest.raises(ValueError, match=r'body\.1\.res_layer\.2\.weight is \(15,\), expected \(16,\)'):
        arcface.parse_state_dict(without(**{'body.1.res_layer.2.weight': torch.zeros(15)}), pool=POOL)
    with pytest.raises(ValueError, match=r'body\.2\.shortcut_layer\.0\.weight is \(32, 16, 3, 3\)'):
        arcface.parse_state_dict(without(**{'body.2.shortcut_layer.0.weight': torch.zeros(32, 16, 3, 3)}), pool=POOL)
    with pytest.raises(ValueError, match=r'has no body\.2\.shortcut_layer\.0\.weight'):
        arcface.parse_state_dict(without('body.2.shortcut_layer.0.weight'), pool=POOL)
    with pytest.raises(ValueError, match=r'body\.3\.res_layer\.5\.fc2\.weight is .* expected \(32, 8, 1, 1\)'):
        arcface.parse_state_dict(without(**{'body.3.res_layer.5.fc2.weight': torch.zeros(32, 4, 1, 1)}), pool=POOL)
    # a unit that does not take what the one before it gives
    with pytest.raises(ValueError, match=r'body\.1\.res_layer\.1\.weight is \(16, 8, 3, 3\): the unit takes 8 channels, the layer before it gives 16'):
        arcface.parse_state_dict(without(**{'body.1.res_layer.1.weight': torch.zeros(16, 8, 3, 3)}), pool=POOL)
    # an inconsistent unit list: another width, too few units, too many, a stride that is none
    with pytest.raises(ValueError, match=r'body\.2\.res_layer\.1\.weight is \(32, 16, 3, 3\), which is not unit 2 of the list, \(16, 16, 1\)'):
        arcface.parse_state_dict(sd, units=[(16, 16, 2), (16, 16, 1), (16, 16, 1), (16, 32, 2)], pool=POOL)
    with pytest.raises(ValueError, match=r'body\.3\.res_layer\.1\.weight, past the 3 units'):
        arcface.parse_state_dict(sd, units=UNITS[:3], pool=POOL)
    with pytest.raises(ValueError, match=r'has no body\.4\.res_layer\.1\.weight'):
        arcface.parse_state_dict(sd, units=UNITS + [(32, 32, 1)], pool=POOL)
    with pytest.raises(ValueError, match='stride 1 or 2'):
        arcface.parse_state_dict(sd, units=[(16, 16, 3)], pool=POOL)
    # the Linear does not fit the plane the units leave (a pool of 24 leaves 6 x 6)
    with pytest.raises(ValueError, match=r'output_layer\.3\.weight is \(64, 2048\).*32 \* 6 \* 6'):
        arcface.parse_state_dict(sd, pool=24)
    with pytest.raises(ValueError, match='only one of output_layer.4.weight'):
        arcface.parse_state_dict(without('output_layer.4.bias'), pool=POOL)
    with pytest.raises(ValueError, match='give path or state_dict, not both'):
        arcface.ArcFaceID('x.pth', state_dict=sd)
    with pytest.raises(FileNotFoundError, match='ArcFace IR-SE weight file not found'):
        arcface.ArcFaceID('/nonexistent/model_ir_se50.pth')
    with pytest.raises(ValueError, match='box must be'):
        arcface.ArcFaceID(state_dict=sd, box=(8, 8, 8, 56), pool=POOL)
    with pytest.raises(ValueError, match='pool must be'):
        arcface.ArcFaceID(state_dict=sd, box=BOX, pool=0)


# ---------------------------------------------------------------------------------------------------------- the folded form
def _folded_embed(x, net, box, pool, shift_as_bias=False):
    """the contract of each kernel restated in torch, fp64, on what parse_state_dict(dtype=float64) returns: this is the arithmetic the
    device runs.  shift_as_bias: the WRONG design, the leading batch norm's shift folded into a bias."""
    w, b, slope = net['stem']
    h = F.prelu(F.conv2d(R.extract(x, box, pool, torch.float64), w, b, 1, 1), slope)                     # te_id_stem_fwd_f32
    for u in net['units']:
        if shift_as_bias:
            bias = (u['w1'] * u['shift'].view(1, -1, 1, 1)).sum((1, 2, 3))
            t = F.prelu(F.conv2d(h * u['scale'].view(1, -1, 1, 1), u['w1'], bias, 1, 1), u['slope'])
        else:
            v = F.pad(h * u['scale'].view(1, -1, 1, 1) + u['shift'].view(1, -1, 1, 1), (1, 1, 1, 1))      # the affine inside, zeros around
            t = F.prelu(F.conv2d(v, u['w1']), u['slope'])                                                 # te_conv2d_prelu_f32
        r = F.conv2d(t, u['w2'], u['b2'], u['stride'], 1)                                                 # te_conv2d_f32
        if u['fc1'] is not None:
            gate = torch.sigmoid(F.relu(r.mean((2, 3)) @ u['fc1'].t()) @ u['fc2'].t())                    # te_se_excite_f32
            r = r * gate[:, :, None, None]
        if u['sc'] is not None:
            sc = F.conv2d(h, u['sc'][0], u['sc'][1], u['stride'], 0)
        else:
            sc = h[:, :, ::u['stride'], ::u['stride']]
        h = r + sc                                                                                        # te_se_scale_add_f32
    e = h.flatten(1) @ net['fc'][0].t() + net['fc'][1]                                                    # te_fc_stream_f32
    return e / e.norm(dim=1, keepdim=True)                                                                # te_rows_unit_f32


@pytest.mark.parametrize('se,affine', [(True, True), (False, False)])
def test_folded_form_is_the_unfolded_network(small, se, affine):
    """the two agree to 1e-12 on every element of the embeddings, which every border pixel of every unit feeds; folding the shift into a
    bias instead moves them in the second digit"""
    from transeditor_amd import arcface
    x, sd = small
    if not (se and affine):
        sd = R.state_dict(3, units=UNITS, pool=POOL, dim=DIM, se=se, affine=affine)
    net = arcface.parse_state_dict(sd, pool=POOL, dtype=torch.float64)
    assert net['stem'][0].dtype == torch.float64 and net['affine'] == affine
    want = R.embed(x, sd, torch.float64, UNITS, BOX, POOL)
    got = _folded_embed(x, net, BOX, POOL)
    assert float((got - want).abs().max()) <= 1e-12
    wrong = _folded_embed(x, net, BOX, POOL, shift_as_bias=True)
    assert float((wrong - want).abs().max()) > 1e-3


def test_affine_less_output_layer(small):
    """IR_SE_50() builds BatchNorm1d(512, affine=False): no output_layer.4.weight / .bias; taken as gamma 1, beta 0"""
    from transeditor_amd import arcface
    _, sd = small
    bare = {k: v for k, v in sd.items() if k not in ('output_layer.4.weight', 'output_layer.4.bias')}
    ones = dict(bare, **{'output_layer.4.weight': torch.ones(DIM), 'output_layer.4.bias': torch.zeros(DIM)})
    a, b = arcface.parse_state_dict(bare, pool=POOL), arcface.parse_state_dict(ones, pool=POOL)
    assert not a['affine'] and b['affine']
    assert torch.equal(a['fc'][0], b['fc'][0]) and torch.equal(a['fc'][1], b['fc'][1])
    assert a['keys'] == b['keys'] - {'output_layer.4.weight', 'output_layer.4.bias'}
    assert not torch.equal(a['fc'][0], arcface.parse_state_dict(sd, pool=POOL)['fc'][0])


# ---------------------------------------------------------------------------------------------------------- the identity figures
def _cosine_distance(u, v):
    """scipy.spatial.distance.cosine restated"""
    return 1.0 - float(np.dot(u, v)) / (float(np.sqrt(np.dot(u, u))) * float(np.sqrt(np.dot(v, v))))


def _ratio_loop(feats, change):
    """calculate_score_id.py:58-90 line by line for h = 3 (columns 0 ... 6, the origin in column 3)"""
    cp = cn = ip = in_ = 0.0
    for i in range(len(change)):
        cp += np.sum(np.array(change[i][6]) - np.array(change[i][3]))
        cn += np.sum(np.array(change[i][0]) - np.array(change[i][3]))
        ip += _cosine_distance(feats[i][6], feats[i][3])
        in_ += _cosine_distance(feats[i][0], feats[i][3])
        cp += np.sum(np.array(change[i][4:7]) - np.array(change[i][3:6]))
        cn += np.sum(np.array(change[i][0:3]) - np.array(change[i][1:4]))
        for j in range(3):
            ip += _cosine_distance(feats[i][4 + j], feats[i][3 + j])
            in_ += _cosine_distance(feats[i][0 + j], feats[i][1 + j])
    cp, ip, cn, in_ = (v / len(change) for v in (cp, ip, cn, in_))
    return (abs(ip / cp) + abs(in_ / cn)) / 2


def test_identity_ratio_is_the_reference_loop():
    from transeditor_amd.edit_eval import identity_ratio
    rng = np.random.default_rng(5)
    M, D = 6, 20
    # a straight path through the origin plus a little noise: the cosine distance grows with the square of the distance walked, so the
    # end-to-origin term is about nine single steps, while the scores' end-to-origin term is three
    f = rng.standard_normal((M, 1, D)) + 0.3 * np.arange(-3, 4).reshape(1, 7, 1) * rng.standard_normal((M, 1, D)) + 0.02 * rng.standard_normal((M, 7, D))
    c = np.cumsum(rng.random((M, 7)) * 0.1, axis=1) + rng.standard_normal((M, 1))
    want = _ratio_loop(f, c)
    got = identity_ratio(f.astype(np.float32), c.astype(np.float32))
    assert isinstance(got, float)
    assert abs(identity_ratio(f, c) - want) <= 1e-12 * want
    assert abs(got - _ratio_loop(f.astype(np.float32).astype(np.float64), c.astype(np.float32).astype(np.float64))) <= 1e-12 * want
    # dependency_ratio-style sums (the consecutive terms alone) give another figure: the end-to-origin terms are in
    def dist(a, b):
        return 1.0 - np.sum(a * b, -1) / np.sqrt(np.sum(a * a, -1) * np.sum(b * b, -1))
    cp, cn = np.sum(c[:, 4:] - c[:, 3:-1]) / M, np.sum(c[:, :3] - c[:, 1:4]) / M
    ip, in_ = np.sum(dist(f[:, 4:], f[:, 3:-1])) / M, np.sum(dist(f[:, :3], f[:, 1:4])) / M
    assert abs((abs(ip / cp) + abs(in_ / cn)) / 2 - want) > 0.05 * want
    # another h
    f5, c5 = f[:, 1:6], c[:, 1:6]
    cp = (np.sum(c5[:, 4] - c5[:, 2]) + np.sum(c5[:, 3:] - c5[:, 2:-1])) / M
    cn = (np.sum(c5[:, 0] - c5[:, 2]) + np.sum(c5[:, :2] - c5[:, 1:3])) / M
    ip = (np.sum(dist(f5[:, 4], f5[:, 2])) + np.sum(dist(f5[:, 3:], f5[:, 2:-1]))) / M
    in_ = (np.sum(dist(f5[:, 0], f5[:, 2])) + np.sum(dist(f5[:, :2], f5[:, 1:3]))) / M
    assert abs(identity_ratio(f5, c5) - (abs(ip / cp) + abs(in_ / cn)) / 2) <= 1e-12
    for bad_f, bad_c in [(f[:, :6], c[:, :6]), (f, c[:, :5]), (f[0], c), (f, c[:, :, None]), (f[:, :1], c[:, :1]), (f[:3], c)]:
        with pytest.raises(ValueError, match='identity_ratio'):
            identity_ratio(bad_f, bad_c)


def test_identity_similarity_and_feature_sweeps_layout():
    from transeditor_amd.edit_eval import feature_sweeps, identity_similarity
    rng = np.random.default_rng(7)
    f = rng.standard_normal((4, 7, 33)).astype(np.float32)
    sim = identity_similarity(f)
    assert sim.shape == (4, 7) and sim.dtype == np.float64 and bool((sim[:, 3] == 1.0).all())
    f64 = f.astype(np.float64)
    want = np.einsum('nsd,nd->ns', f64, f64[:, 3]) / (np.linalg.norm(f64, axis=2) * np.linalg.norm(f64[:, 3], axis=1)[:, None])
    assert float(np.abs(np.delete(sim - want, 3, axis=1)).max()) <= 1e-15 and float(np.abs(sim).max()) <= 1.0
    for bad in (f[:, :6], f[0], f[:, :1]):
        with pytest.raises(ValueError, match='identity_similarity'):
            identity_similarity(bad)
    # the layout, with an `embed` that runs anywhere: the channel means and the corner pixel, returned as [B,4,1,1] (it is flattened)
    calls = []

    def embed(images):
        calls.append(images.shape[0])
        return torch.cat([images.mean((2, 3)), images[:, :1, 0, 0]], 1)[:, :, None, None]
    g = torch.Generator().manual_seed(3)
    origin, sweeps = torch.randn(3, 3, 8, 8, generator=g), {'z': torch.randn(3, 6, 3, 8, 8, generator=g), 'p': torch.randn(3, 4, 3, 8, 8, generator=g)}
    res = feature_sweeps(embed, origin, sweeps, batch=4)
    assert calls == [3, 4, 4, 4, 4, 2, 4, 4, 4] and set(res) == {'z', 'p'}
    assert res['z'].shape == (3, 7, 4) and res['p'].shape == (3, 5, 4) and res['z'].dtype == np.float32
    flat = lambda t: embed(t).reshape(t.shape[0], -1).numpy()
    assert np.array_equal(res['z'][:, 3], flat(origin)) and np.array_equal(res['p'][:, 2], flat(origin))
    assert np.array_equal(np.delete(res['z'], 3, axis=1), flat(sweeps['z'].flatten(0, 1)).reshape(3, 6, 4))
    assert np.array_equal(np.delete(res['p'], 2, axis=1), flat(sweeps['p'].flatten(0, 1)).reshape(3, 4, 4))
    with pytest.raises(ValueError, match='batch must be positive'):
        feature_sweeps(embed, origin, sweeps, batch=0)
    with pytest.raises(ValueError, match="sweep 'z'"):
        feature_sweeps(embed, origin[:2], sweeps, batch=4)


# ---------------------------------------------------------------------------------------------------------- the command line, the ABI
def test_command_line(tmp_path, small):
    from transeditor_amd import arcface
    parse = arcface.build_parser().parse_args
    a = parse(['--weights', 'model_ir_se50.pth', '--a', 'A.pt', '--b', 'B.pt'])
    assert (a.weights, a.a, a.b, a.batch, a.box, a.pool) == ('model_ir_se50.pth', 'A.pt', 'B.pt', 16, [35, 223, 32, 220], 112)
    a = parse(['--weights', 'w.pth', '--a', 'A.pt', '--b', 'B.pt', '--batch', '4', '--box', '8', '56', '8', '56', '--pool', '32'])
    assert (a.batch, a.box, a.pool) == (4, [8, 56, 8, 56], 32)
    for bad in (['--a', 'A.pt', '--b', 'B.pt'], ['--weights', 'w.pth', '--a', 'A.pt'], ['--weights', 'w.pth', '--a', 'A.pt', '--b', 'B.pt', '--box', '1', '2']):
        with pytest.raises(SystemExit):
            parse(bad)
    assert arcface.result_line([0.5, 0.7, 0.9]) == 'New Average score is 0.70+-0.16'              # np.std: the population deviation
    with pytest.raises(SystemExit):
        arcface.main(['--weights', 'w.pth', '--a', 'A.pt', '--b', 'B.pt', '--batch', '0'])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a GPU'):
            arcface.main(['--weights', 'w.pth', '--a', 'A.pt', '--b', 'B.pt'])
        x, sd = small
        net = arcface.ArcFaceID(state_dict=sd, box=BOX, pool=POOL)                                   # builds without a GPU, runs only on one
        assert net.units == tuple(UNITS) and net.dim == DIM and net.stem_w.dtype == torch.float32
        with pytest.raises(RuntimeError, match='needs a GPU'):
            net(x)


def test_abi_entry_points_and_the_build():
    """the six entry points are declared, bound and exported by the library that `python -m transeditor_amd.build` makes from
    csrc/irse.hip for gfx950; their argument checks run on the host"""
    import ctypes
    from transeditor_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    names = ('te_conv2d_prelu_f32', 'te_id_stem_fwd_f32', 'te_se_excite_f32', 'te_se_scale_add_f32', 'te_rows_unit_f32', 'te_rows_dot_f32')
    for name in names:
        assert name in _lib.EXPORTS and name + '(' in header
    assert 'M9' in header and 'model_irse.py:10-49' in header and 'id_loss.py:8-21' in header
    assert 'irse.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'irse.hip'))
    build.build()                                                               # (a no-op when the library is up to date)
    L = _lib.lib()
    assert L.te_arch() == b'gfx950' and all(hasattr(L, n) for n in names)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16                   # validation only: never dereferenced
    conv = (1, 3, 4, 8, 8, 3, 3, 1, 1, 1, None)
    assert L.te_conv2d_prelu_f32(None, None, None, None, None, None, None, *conv) == -1 and b'NULL' in L.te_last_error_string()
    assert L.te_conv2d_prelu_f32(p, p, p, p, None, p, p, *conv) == -1
    assert L.te_conv2d_prelu_f32(p, p, p, p, p, p, None, *conv) == -1 and b'both' in L.te_last_error_string()
    assert L.te_conv2d_prelu_f32(p, p, p, p, p, p, p, 1, 3, 4, 8, 8, 3, 3, 3, 1, 1, None) == -3 and b'stride' in L.te_last_error_string()
    assert L.te_conv2d_prelu_f32(p, p, p, p, p, p, p, 1, 3, 4, 8, 8, 3, 3, 1, 3, 1, None) == -2
    for N, H, W, y0, y1, x0, x1, Pn, Co in [(1, 40, 40, 4, 4, 4, 36, 16, 8), (1, 40, 40, 4, 41, 4, 36, 16, 8), (1, 40, 40, 4, 36, -1, 36, 16, 8),
                                            (1, 40, 40, 4, 36, 4, 36, 0, 8), (0, 40, 40, 4, 36, 4, 36, 16, 8), (65536, 40, 40, 4, 36, 4, 36, 16, 8),
                                            (1, 40, 40, 4, 36, 4, 36, 16, 0)]:
        assert L.te_id_stem_fwd_f32(p, p, p, p, p, N, H, W, y0, y1, x0, x1, Pn, Co, None) == -2, (N, H, W, y0, y1, x0, x1, Pn, Co)
    assert L.te_id_stem_fwd_f32(p, None, p, p, p, 1, 40, 40, 4, 36, 4, 36, 16, 8, None) == -1
    assert L.te_se_excite_f32(p, p, p, p, 2, 8, 1025, None) == -2 and L.te_se_excite_f32(p, p, p, p, 0, 8, 4, None) == -2
    assert L.te_se_excite_f32(p, p, None, p, 2, 8, 4, None) == -1
    assert L.te_se_scale_add_f32(p, p, p, p, 1, 3, 4, 4, 7, 9, 2, None) == -2 and b'shortcut' in L.te_last_error_string()
    assert L.te_se_scale_add_f32(p, p, p, p, 1, 3, 4, 4, 7, 7, 3, None) == -3 and L.te_se_scale_add_f32(p, p, None, None, 1, 3, 4, 4, 7, 7, 2, None) == -1
    assert L.te_rows_unit_f32(p, p, 0, 8, None) == -2 and L.te_rows_unit_f32(p, None, 2, 8, None) == -1
    assert L.te_rows_dot_f32(p, p, p, 2, 0, None) == -2 and L.te_rows_dot_f32(p, p, None, 2, 8, None) == -1

"""Host side of the AlexNet LPIPS diversity score (transeditor_amd.lpips_alex, metrics.evaluate_diversity; metrics/lpips.py:49-82,
metrics/evaluate_query.py:82-133): weight parsing, the three figures' naming and draw order, the command line, the C ABI's refusals
(decided before any launch) and the restatement of tests/lpips_alex_restated.py against what the reference's own class returned
(tests/golden/lpips_alex_ref.npz, tools/lpips_alex_golden.py).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lpips_alex_restated as R
from conftest import ROOT

SMALL = (8, 12, 16, 12, 8)


@pytest.fixture(scope='module')
def golden_ref():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'lpips_alex_ref.npz'))


# ------------------------------------------------------------------------------------------------------------------ the weights
def test_parse_reads_the_geometry_from_the_shapes():
    from transeditor_amd import lpips_alex as A
    sd, lin = R.state_dict(3, SMALL), R.lin_state_dict(4, SMALL)
    sd['classifier.1.weight'] = torch.zeros(2, 2)                               # ignored
    net = A.parse_state_dicts(sd, lin)
    assert net['widths'] == SMALL and [tuple(h.shape) for h in net['heads']] == [(c,) for c in SMALL]
    assert [tuple(w.shape) for w, _ in net['convs']] == [(8, 3, 11, 11), (12, 8, 5, 5), (16, 12, 3, 3), (12, 16, 3, 3), (8, 12, 3, 3)]
    assert torch.equal(net['heads'][2], lin['lpips_weights.2.main.1.weight'].reshape(-1))
    m = A.AlexLPIPS(state_dict=sd, lin_state_dict=lin)
    assert m.widths == SMALL and not m.training and set(dict(m.named_buffers())) == {f'{n}{l}' for n in ('w', 'b', 'lin') for l in range(5)}
    assert (A.CONVS, A.GEOMETRY, A.POOL_BEFORE) == (R.CONVS, R.GEOMETRY, R.POOL_BEFORE)


def test_parse_names_the_key_that_is_wrong(tmp_path):
    from transeditor_amd import lpips_alex as A
    sd, lin = R.state_dict(3, SMALL), R.lin_state_dict(4, SMALL)
    with pytest.raises(ValueError, match=r'features\.6\.weight'):
        A.parse_state_dicts({k: v for k, v in sd.items() if k != 'features.6.weight'}, lin)
    with pytest.raises(ValueError, match=r'features\.3\.weight is \(12, 8, 3, 3\)'):
        A.parse_state_dicts(dict(sd, **{'features.3.weight': torch.zeros(12, 8, 3, 3)}), lin)
    with pytest.raises(ValueError, match=r'features\.8\.weight'):              # the input width must be the previous layer's
        A.parse_state_dicts(dict(sd, **{'features.8.weight': torch.zeros(12, 15, 3, 3)}), lin)
    with pytest.raises(ValueError, match=r'lpips_weights\.4\.main\.1\.weight'):
        A.parse_state_dicts(sd, {k: v for k, v in lin.items() if not k.startswith('lpips_weights.4')})
    with pytest.raises(ValueError, match=r'lpips_weights\.1\.main\.1\.weight is \(12,\)'):
        A.parse_state_dicts(sd, dict(lin, **{'lpips_weights.1.main.1.weight': torch.zeros(12)}))
    with pytest.raises(ValueError, match=r'lpips_weights\.1\.main\.1\.weight has 13 channels, but its tap features\.3 has 12'):
        A.parse_state_dicts(sd, dict(lin, **{'lpips_weights.1.main.1.weight': torch.zeros(1, 13, 1, 1)}))
    with pytest.raises(ValueError, match='alexnet_path or state_dict, not both'):
        A.AlexLPIPS(alexnet_path='a.pth', state_dict=sd, lin_state_dict=lin)
    with pytest.raises(ValueError, match='lin_path or state_dict, not both'):
        A.AlexLPIPS(state_dict=sd, lin_path='l.ckpt', lin_state_dict=lin)
    with pytest.raises(FileNotFoundError, match='nothing is downloaded'):
        A.AlexLPIPS(alexnet_path=str(tmp_path / 'missing.pth'), lin_state_dict=lin)
    with pytest.raises(FileNotFoundError, match='lpips_weights.ckpt'):
        A.AlexLPIPS(state_dict=sd)
    assert A.default_alexnet_path().endswith(os.path.join('checkpoints', 'alexnet-owt-7be5be79.pth'))
    torch.save(sd, tmp_path / 'a.pth')
    torch.save(lin, tmp_path / 'l.ckpt')
    assert A.AlexLPIPS(str(tmp_path / 'a.pth'), str(tmp_path / 'l.ckpt')).widths == SMALL


def test_input_checks_come_before_the_gpu():
    from transeditor_amd import lpips_alex as A
    m = A.AlexLPIPS(state_dict=R.state_dict(3, SMALL), lin_state_dict=R.lin_state_dict(4, SMALL))
    m = m.to('cpu')
    with pytest.raises(ValueError, match=r'\[N,3,H,W\]'):
        m.pairwise(torch.zeros(2, 1, 32, 32))
    with pytest.raises(ValueError, match='at least 7'):
        m.pairwise(torch.zeros(2, 3, 6, 32))
    with pytest.raises(ValueError, match='at least 2 images'):
        m.group_mean(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match='one shape'):
        m(torch.zeros(2, 3, 32, 32), torch.zeros(3, 3, 32, 32))
    with pytest.raises(RuntimeError, match='AlexLPIPS needs a GPU'):
        m.pairwise(torch.zeros(2, 3, 32, 32))
    with pytest.raises(RuntimeError, match='AlexLPIPS needs a GPU'):
        m(torch.zeros(3, 32, 32), torch.zeros(3, 32, 32))


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_abi_is_declared_bound_and_built():
    from transeditor_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    for name in ('te_alex_stem_fwd_f32', 'te_lpips_unit_f32', 'te_lpips_allpairs_ws_floats', 'te_lpips_allpairs_fwd_f32',
                 'te_lpips_allpairs_dist_f32'):
        assert name in _lib.EXPORTS and name + '(' in header
    assert 'M8' in header and 'metrics/lpips.py:49-82' in header and 'lpips_alex.hip' in build.SOURCES
    assert 'INSIDE the root' in header                                          # the one difference from the VGG head's eps


def test_refusals_are_decided_on_the_host():
    """every refusal returns before a launch, so it can be exercised without a GPU: the pointers below are never dereferenced"""
    from transeditor_amd import _lib
    L = _lib.lib()
    p = C.c_void_p(64)
    stem = lambda N, H, W, Co, out=p, x=p, w=p, b=p: L.te_alex_stem_fwd_f32(out, x, w, b, N, H, W, Co, None)
    for null in ('out', 'x', 'w', 'b'):
        assert stem(1, 32, 32, 64, **{null: None}) == _lib.lib().te_bias_act_f32(None, None, None, None, 3, 0, 0.2, 1.0, 16, 1, 1, None)
    shape = stem(0, 32, 32, 64)
    assert shape != 0 and b'te_alex_stem_fwd_f32' in L.te_last_error_string()
    for bad in ((-1, 32, 32, 64), (65536, 32, 32, 64), (1, 0, 32, 64), (1, 32, -3, 64), (1, 32, 32, 0), (1, 6, 32, 64), (1, 32, 6, 64),
                (1, 32768, 32768, 64)):
        assert stem(*bad) == shape, bad
    assert stem(1, 6, 32, 64) == shape and b'does not fit' in L.te_last_error_string()
    assert L.te_lpips_unit_f32(None, p, 1, 1, 1, None) != 0 and L.te_lpips_unit_f32(p, p, 0, 1, 1, None) == shape
    assert L.te_lpips_unit_f32(p, p, 1, 0, 1, None) == shape and L.te_lpips_unit_f32(p, p, 1, 1, 0, None) == shape
    assert L.te_lpips_unit_f32(p, p, 65536, 1, 1, None) == shape and L.te_lpips_unit_f32(p, p, 1, 2, 2 ** 30, None) == shape
    assert L.te_lpips_allpairs_fwd_f32(p, p, None, 2, 1, 1, None) != 0 and L.te_lpips_allpairs_fwd_f32(p, p, p, 65536, 1, 1, None) == shape
    assert L.te_lpips_allpairs_fwd_f32(p, p, p, 0, 1, 1, None) == shape and L.te_lpips_allpairs_fwd_f32(p, p, p, 2, 1, 65535 * 256 + 1, None) == shape
    ptrs, cs, hw = (C.c_void_p * 1)(64), (C.c_int * 1)(5), (C.c_int64 * 1)(9)
    dist = L.te_lpips_allpairs_dist_f32
    assert dist(p, ptrs, cs, hw, 0, 2, None) == shape and dist(p, ptrs, cs, hw, 9, 2, None) == shape
    assert dist(p, ptrs, cs, hw, 1, 65536, None) == shape and dist(None, ptrs, cs, hw, 1, 2, None) != 0
    assert dist(p, (C.c_void_p * 1)(None), cs, hw, 1, 2, None) != 0 and dist(p, ptrs, None, hw, 1, 2, None) != 0
    assert dist(p, ptrs, (C.c_int * 1)(0), hw, 1, 2, None) == shape and dist(p, ptrs, cs, (C.c_int64 * 1)(0), 1, 2, None) == shape
    # the workspace: upper-triangle tiles of 8 x 8 images, blocks of 256 pixels, slices of 32 channels, 64 floats each
    ws = L.te_lpips_allpairs_ws_floats
    assert ws(1, 1, 1) == 64 and ws(8, 32, 256) == 64 and ws(9, 33, 257) == 3 * 2 * 2 * 64 and ws(40, 64, 3969) == 15 * 16 * 2 * 64
    assert ws(40, 384, 225) == 15 * 1 * 12 * 64
    assert ws(0, 1, 1) < 0 and ws(65536, 1, 1) < 0 and ws(2, 1, 0) < 0 and ws(2, 0, 1) < 0


def test_existing_entry_points_keep_their_limits():
    """the stem's 11 x 11 / stride 4 are its own: te_conv2d_f32 and te_conv2d_res_f32 refuse them as before"""
    from transeditor_amd import _lib
    L = _lib.lib()
    p = C.c_void_p(64)
    ok = lambda kh, s: L.te_conv2d_f32(p, p, p, p, 1, 3, 8, 32, 32, kh, kh, s, 2, 2, 8, 0, 1, None)
    unsupported = ok(11, 1)
    assert unsupported != 0 and b'1 <= kh, kw <= 7' in L.te_last_error_string()
    assert ok(7, 4) == unsupported and b'stride must be 1 or 2' in L.te_last_error_string()
    assert ok(8, 2) == unsupported and ok(7, 3) == unsupported
    assert L.te_conv2d_res_f32(p, p, p, p, p, 1, 3, 8, 32, 32, 11, 11, 4, 2, 2, 1, None) == unsupported


# ------------------------------------------------------------------------------------------------------- evaluate_diversity
class _ToyGenerator(torch.nn.Module):
    """image = a fixed linear map of (z, p); records what it was called with"""
    layer_noise_injection = False

    def __init__(self, latent=8, para_num=2):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.wz = torch.nn.Parameter(torch.randn(latent * para_num, 3 * 4 * 4, generator=g))
        self.wp = torch.nn.Parameter(torch.randn(latent * para_num, 3 * 4 * 4, generator=g))
        self.calls = []

    def forward(self, z, p):
        self.calls.append((z.clone(), p.clone()))
        return (z.flatten(1) @ self.wz + p.flatten(1) @ self.wp).view(-1, 3, 4, 4), None, None


class _ToyLPIPS:
    def __init__(self):
        self.seen = []

    def group_mean(self, img):
        self.seen.append(img.clone())
        return torch.pdist(img.flatten(1)).mean()


def test_evaluate_diversity_names_and_draw_order():
    """the random stream written out by hand: per iteration (p, z) of 'all', (one p, z) of 'same_p', (p, one z) of 'same_z', in that
    order, each a single randn call of the shape the reference's samplers draw (evaluate_query.py:108-124, utils/sample.py)"""
    from transeditor_amd import metrics
    from transeditor_amd.inference import GeneratorSampler
    n_iter, group, latent, para = 2, 3, 8, 2
    G, lp = _ToyGenerator(latent, para), _ToyLPIPS()
    s = GeneratorSampler(G, use_graph=False)
    state = torch.random.get_rng_state()
    out = metrics.evaluate_diversity(s, lp, n_iter=n_iter, group=group, seed=7, latent=latent, para_num=para)
    assert torch.equal(torch.random.get_rng_state(), state)                    # a seeded run leaves the global state alone
    assert set(out) == {'all', 'same_p', 'same_z', 'per_iteration'} and set(out['per_iteration']) == {'all', 'same_p', 'same_z'}
    assert [n for n, _, _ in metrics.DIVERSITY_GROUPS] == ['all', 'same_p', 'same_z']
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        want = []
        for _ in range(n_iter):
            p = torch.randn(group, latent, para)                                 # 'spatial'
            z = torch.randn(group, latent, para)                                 # 'query'
            want.append(('all', z, p))
            p = torch.randn(latent, para).repeat(group, 1, 1)                    # 'spatial_same': ONE p for the group
            z = torch.randn(group, latent, para)
            want.append(('same_p', z, p))
            p = torch.randn(group, latent, para)
            z = torch.randn(latent, para).repeat(group, 1, 1)                    # 'query_same': ONE z for the group
            want.append(('same_z', z, p))
    assert len(G.calls) == 3 * n_iter == len(lp.seen)
    values = {'all': [], 'same_p': [], 'same_z': []}
    for (name, z, p), (gz, gp), img in zip(want, G.calls, lp.seen):
        assert torch.equal(gz, z) and torch.equal(gp, p), name
        values[name].append(torch.pdist(img.flatten(1)).mean())
    for gz, gp in G.calls[1::3]:
        assert torch.equal(gp[0], gp[1]) and torch.equal(gp[0], gp[2]) and not torch.equal(gz[0], gz[1])       # same_p: p shared, z varies
    for gz, gp in G.calls[2::3]:
        assert torch.equal(gz[0], gz[1]) and torch.equal(gz[0], gz[2]) and not torch.equal(gp[0], gp[1])       # same_z
    for name, v in values.items():
        v = torch.stack(v)
        assert out['per_iteration'][name].dtype == np.float32 and np.array_equal(out['per_iteration'][name], v.numpy())
        assert out[name] == float(v.mean()) and isinstance(out[name], float)
    # truncation multiplies both codes (evaluate_query.py:108-109); another seed gives other figures; argument checks
    G.calls.clear()
    metrics.evaluate_diversity(s, _ToyLPIPS(), n_iter=1, group=group, truncation=0.5, seed=7, latent=latent, para_num=para)
    assert torch.equal(G.calls[0][0], want[0][1] * 0.5) and torch.equal(G.calls[0][1], want[0][2] * 0.5)
    assert metrics.evaluate_diversity(s, _ToyLPIPS(), n_iter=2, group=group, seed=8, latent=latent, para_num=para)['all'] != out['all']
    with pytest.raises(ValueError, match='group >= 2'):
        metrics.evaluate_diversity(s, _ToyLPIPS(), n_iter=1, group=1)
    with pytest.raises(ValueError, match='n_iter >= 1'):
        metrics.evaluate_diversity(s, _ToyLPIPS(), n_iter=0)


def test_docstring_says_which_printed_number_is_which():
    from transeditor_amd import metrics
    flat = lambda text: ' '.join(text.split())
    assert 'the first is `all`, the second `same_p`, the third `same_z`' in flat(metrics.__doc__) and 'same_p' in metrics.evaluate_diversity.__doc__
    assert 'the first is `all`, the second `same_p`, the third `same_z`' in flat(open(os.path.join(ROOT, 'INTEGRATION.md')).read())


# ------------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_flags_of_the_diversity_score():
    from transeditor_amd.metrics import build_parser, main
    args = vars(build_parser(diversity=True).parse_args([]))
    assert set(args) - set(vars(build_parser().parse_args([]))) == {'alexnet', 'lpips_alex_lin', 'lpips_iters', 'lpips_group'}
    assert args['alexnet'] is None and args['lpips_alex_lin'] is None and args['lpips_iters'] == 1000 and args['lpips_group'] == 40
    a = build_parser(diversity=True).parse_args(['--lpips', '--alexnet', 'a.pth', '--lpips_alex_lin', 'l.ckpt', '--lpips_iters', '3',
                                                 '--lpips_group', '5'])
    assert a.lpips and (a.alexnet, a.lpips_alex_lin, a.lpips_iters, a.lpips_group) == ('a.pth', 'l.ckpt', 3, 5)
    with pytest.raises(SystemExit, match=r'--lpips_alex_lin \(the AlexNet LPIPS head file.*lpips_weights\.ckpt\) is required; nothing is downloaded'):
        main(['--lpips', '--alexnet', 'a.pth'])
    with pytest.raises(SystemExit, match='lpips_alex_lin'):                    # before the PPL's own requirement
        main(['--lpips', '--ppl'])
    with pytest.raises(SystemExit, match='--lpips_lin'):                       # the PPL still needs its VGG heads
        main(['--lpips', '--ppl', '--lpips_alex_lin', 'l.ckpt'])
    with pytest.raises(SystemExit, match='--ppl, --ppl_all or --lpips'):
        main(['--lpips_alex_lin', 'l.ckpt'])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a GPU'):
            main(['--lpips', '--lpips_alex_lin', 'l.ckpt'])


# ------------------------------------------------------------------------------------------------- restatement against the reference
def test_restatement_matches_the_reference_class(golden_ref):
    """the reference's own LPIPS, run pair by pair in fp32 on the CPU (tools/lpips_alex_golden.py), against the fp32 restatement: both
    are fp32 evaluations of one formula, each about 1e-7 from fp64 (LPIPS_ALEX_REPORT.txt: 8.5e-8 and 9.4e-8 rel_l2), so they agree
    to 4 x the larger of the two; the fp64 restatement regenerated here equals the stored one to fp64 rounding"""
    g = golden_ref
    assert {k: int(g[k]) for k in ('seed', 'image_seed', 'N', 'S')} == R.GOLDEN
    x, sd = R.images(R.GOLDEN['image_seed'], R.GOLDEN['N'], R.GOLDEN['S']), R.state_dict(R.GOLDEN['seed'])
    lin = {f'lpips_weights.{l}.main.1.weight': torch.from_numpy(g[f'lin{l}']).view(1, -1, 1, 1) for l in range(5)}
    assert [g[f'lin{l}'].shape[0] for l in range(5)] == list(R.WIDTHS)
    d_ref, d64 = torch.from_numpy(g['d_ref']), torch.from_numpy(g['d64'])
    assert d_ref.shape == (15,) and d_ref.dtype == torch.float32 and d64.dtype == torch.float64
    D64 = R.pairwise(x, sd, lin, torch.float64)
    assert torch.equal(D64, D64.t()) and float(D64.diagonal().abs().max()) == 0.0
    assert R.rel_l2(R.triu(D64), d64) < 1e-13
    D32 = R.pairwise(x, sd, lin, torch.float32)
    yard = R.rel_l2(d_ref, d64)
    assert 0 < yard < 1e-6
    assert R.rel_l2(R.triu(D32), d64) <= max(4 * yard, 2.0 ** -20)
    assert R.rel_l2(R.triu(D32), d_ref) <= max(4 * yard, 2.0 ** -20)
    assert 0.05 < float(d64.min()) and float(d64.max()) < 0.2 and len(set(d_ref.tolist())) == 15     # distinct pairs, not degenerate


def test_module_form_has_torchvisions_layout():
    m = R.alexnet()
    assert [n for n, _ in m.named_children()] == ['features', 'avgpool', 'classifier'] and len(m.features) == 13
    convs = [i for i, l in enumerate(m.features) if isinstance(l, torch.nn.Conv2d)]
    assert tuple(convs) == R.CONVS and [m.features[i].out_channels for i in convs] == list(R.WIDTHS)
    assert [(m.features[i].kernel_size[0], m.features[i].stride[0], m.features[i].padding[0]) for i in convs] == list(R.GEOMETRY)
    assert [i for i, l in enumerate(m.features) if isinstance(l, torch.nn.MaxPool2d)] == [2, 5, 12]
    sd = R.state_dict(1)
    m.features.load_state_dict({k[len('features.'):]: v for k, v in sd.items()})
    x = R.images(5, 2, 64)                                                      # (the last pool needs a 3 x 3 plane)
    h, got = R.scale(x, torch.float32), []
    for layer in m.features:
        h = layer(h)
        if isinstance(layer, torch.nn.ReLU):
            got.append(h)
    for a, b in zip(got, R.taps(x, sd, torch.float32)):
        assert torch.equal(a, b)

"""CPU checks of the PPL host logic (transeditor_amd.metrics; metrics/evaluate_query.py:27-43, :135-249, :256-288): the percentile
filter, batch splitting, the crop / resize rule, the latent interpolation and the command line.  The two kernel bindings the host
code calls are replaced by torch restatements."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------------------ percentile filter
def _filter_mean_restated(d):
    """'lower' / 'higher' written out: the sorted values at floor / ceil of the fractional rank (n - 1) * q"""
    s = np.sort(d)
    n = len(s)
    lo = s[int(math.floor((n - 1) * 0.01))]
    hi = s[int(math.ceil((n - 1) * 0.99))]
    return d[(lo <= d) & (d <= hi)].mean()


FILTER_CASES = {
    'n1000': np.random.RandomState(0).rand(1000).astype(np.float32) * 100,
    'n10000': np.random.RandomState(1).lognormal(size=10000).astype(np.float32),
    'n99': np.random.RandomState(2).rand(99).astype(np.float32),
    'n7': np.array([5, 1, 9, 3, 7, 2, 8], dtype=np.float32),
    'n1': np.array([4.5], dtype=np.float32),
    'ties_low': np.array([1] * 30 + list(range(2, 300)), dtype=np.float32),
    'ties_high': np.array(list(range(300)) + [299] * 25, dtype=np.float32),
    'all_equal': np.full(250, 3.25, dtype=np.float32),
    'n101': np.arange(101, dtype=np.float32)[::-1].copy(),
    'n201': np.random.RandomState(3).permutation(201).astype(np.float32),
}


@pytest.mark.parametrize('name', sorted(FILTER_CASES))
def test_filter_mean_matches_numpy_percentile(name):
    from transeditor_amd.metrics import filter_mean
    d = FILTER_CASES[name]
    lo = np.percentile(d, 1, method='lower')
    hi = np.percentile(d, 99, method='higher')
    ref = np.extract(np.logical_and(lo <= d, d <= hi), d).mean()
    got = filter_mean(d)
    assert isinstance(got, float)
    assert got == float(ref)
    assert got == float(_filter_mean_restated(d))


def test_filter_drops_the_tails_and_keeps_ties():
    from transeditor_amd.metrics import filter_mean
    d = np.arange(1000, dtype=np.float32)                # rank 9.99 -> lower 9, rank 989.01 -> higher 990
    assert filter_mean(d) == float(np.arange(9, 991, dtype=np.float32).mean())
    d = FILTER_CASES['ties_low']                         # the 1st percentile falls inside a run of equal values: all of them stay
    assert filter_mean(d) == float(d[d <= np.sort(d)[int(math.ceil((len(d) - 1) * 0.99))]].mean())


# -------------------------------------------------------------------------------------------------------------- batch splitting
def test_batch_sizes():
    from transeditor_amd.metrics import batch_sizes
    assert batch_sizes(10000, 64) == [64] * 156 + [16]
    assert batch_sizes(128, 64) == [64, 64]              # the reference appends a remainder of 0 here; it is skipped
    assert batch_sizes(64, 64) == [64]
    assert batch_sizes(10, 64) == [10]
    assert batch_sizes(70, 64) == [64, 6]
    assert batch_sizes(0, 64) == []
    for n, b in ((10000, 64), (128, 64), (10, 64), (70, 64), (1, 1), (999, 7)):
        s = batch_sizes(n, b)
        assert sum(s) == n and all(0 < x <= b for x in s) and all(x == b for x in s[:-1])
    with pytest.raises(ValueError):
        batch_sizes(10, 0)


# ------------------------------------------------------------------------------------------------------------- crop / resize rule
def _reference_lpips_input(image, crop):                 # :222-232
    if crop:
        c = image.shape[2] // 8
        image = image[:, :, c * 3: c * 7, c * 2: c * 6]
    factor = image.shape[2] // 256
    if factor > 1:
        image = F.interpolate(image, size=(256, 256), mode='bilinear', align_corners=False)
    return image


def _crop_resize_restated(img, y0, x0, hc, wc, h, w):
    win = img[:, :, y0:y0 + hc, x0:x0 + wc]
    return win.clone() if (hc, wc) == (h, w) else F.interpolate(win, size=(h, w), mode='bilinear', align_corners=False)


WINDOWS = {   # (size, crop): (y0, x0, hc, wc, h, w)
    (256, False): (0, 0, 256, 256, 256, 256), (256, True): (96, 64, 128, 128, 128, 128),
    (512, False): (0, 0, 512, 512, 256, 256), (512, True): (192, 128, 256, 256, 256, 256),
    (1024, False): (0, 0, 1024, 1024, 256, 256), (1024, True): (384, 256, 512, 512, 256, 256),
    (64, False): (0, 0, 64, 64, 64, 64), (64, True): (24, 16, 32, 32, 32, 32),
}


@pytest.mark.parametrize('size,crop', sorted(WINDOWS))
def test_crop_and_factor_rule(monkeypatch, size, crop):
    from transeditor_amd import _lib, metrics
    assert metrics.lpips_window(size, crop) == WINDOWS[(size, crop)]
    calls = []

    def fake(img, *a):
        calls.append(a)
        return _crop_resize_restated(img, *a)
    monkeypatch.setattr(_lib, 'crop_resize_bilinear', fake)
    img = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(size + crop))
    out = metrics.lpips_input(img, crop)
    ref = _reference_lpips_input(img, crop)
    assert out.shape == ref.shape and torch.equal(out, ref)
    y0, x0, hc, wc, h, w = WINDOWS[(size, crop)]
    if (y0, x0, hc, wc) == (0, 0, h, w):
        assert calls == [] and out is img                # nothing to do: the generator's output goes to LPIPS as it is
    else:
        assert calls == [WINDOWS[(size, crop)]]


# --------------------------------------------------------------------------------------------------------- latent interpolation
def _ref_normalize(x):                                   # :27-28
    return x / torch.sqrt(x.pow(2).sum(-1, keepdim=True))


def _ref_slerp(a, b, t):                                 # :31-39
    a = _ref_normalize(a)
    b = _ref_normalize(b)
    d = (a * b).sum(-1, keepdim=True)
    p = t * torch.acos(d)
    c = _ref_normalize(b - d * a)
    d = a * torch.cos(p) + c * torch.sin(p)
    return _ref_normalize(d)


def _ref_lerp(a, b, t):                                  # :42-43
    return a + (b - a) * t


@pytest.mark.parametrize('t0', [0.0, 0.37])
def test_lerp_and_slerp_are_the_reference_expressions_bit_for_bit(t0):
    from transeditor_amd import metrics
    g = torch.Generator().manual_seed(11)
    x = torch.randn(8, 512, 16, generator=g)
    a, b = x[::2], x[1::2]
    eps = 1e-4
    t = torch.full((1,), t0)
    for ours, ref in ((metrics.lerp, _ref_lerp), (metrics.slerp, _ref_slerp)):
        assert torch.equal(ours(a, b, t), ref(a, b, t))
        assert torch.equal(ours(a, b, t + eps), ref(a, b, t + eps))
    assert torch.equal(metrics.normalize(x), _ref_normalize(x))
    for use_slerp, ref in ((False, _ref_lerp), (True, _ref_slerp)):
        got = metrics._interpolated(x, use_slerp, t, eps)            # :190: torch.stack([e0, e1], 1).view(*inputs.shape)
        assert got.shape == x.shape
        assert torch.equal(got[::2], ref(a, b, t)) and torch.equal(got[1::2], ref(a, b, t + eps))
    assert (t + eps).dtype == torch.float32 and float(torch.zeros(1) + eps) == float(np.float32(1e-4))
    if t0 == 0.0:
        assert torch.equal(metrics.lerp(a, b, t), a)


# ------------------------------------------------------------------------------------------- one batch on a stand-in generator
class _ToyGenerator(torch.nn.Module):
    """image = a fixed linear map of (z, p); the mapped codes are 2 z and 3 p"""
    layer_noise_injection = False

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.wz = torch.nn.Parameter(torch.randn(512 * 16, 3 * 16 * 16, generator=g) / 90)
        self.wp = torch.nn.Parameter(torch.randn(512 * 16, 3 * 16 * 16, generator=g) / 90)
        self.calls = []

    def forward(self, z, p, return_mapped_codes=False, use_style_mapping=True, use_spatial_mapping=True):
        self.calls.append((return_mapped_codes, use_style_mapping, use_spatial_mapping))
        if return_mapped_codes:
            return 2 * z, 3 * p
        z = 2 * z if use_style_mapping else z
        p = 3 * p if use_spatial_mapping else p
        return (z.flatten(1) @ self.wz + p.flatten(1) @ self.wp).view(-1, 3, 16, 16), None, None


class _ToyPercept:
    def pair_distance(self, x):
        return (x[::2] - x[1::2]).pow(2).mean([1, 2, 3])


@pytest.mark.parametrize('space', ['all', 'z', 'p'])
@pytest.mark.parametrize('eval_plus', [False, True])
def test_ppl_distances_flow(space, eval_plus):
    from transeditor_amd import metrics
    from transeditor_amd.inference import GeneratorSampler
    G = _ToyGenerator()
    s = GeneratorSampler(G, use_graph=False)
    g = torch.Generator().manual_seed(3)
    z, p = torch.randn(6, 512, 16, generator=g), torch.randn(6, 512, 16, generator=g)
    if space == 'z':
        p = p[:1].repeat(6, 1, 1)
    if space == 'p':
        z = z[:1].repeat(6, 1, 1)
    eps = 1e-4
    d = metrics.ppl_distances(s, z, p, space=space, eval_plus=eval_plus, use_slerp=False, crop=False, percept=_ToyPercept(), eps=eps)
    assert d.shape == (3,)
    assert G.calls == ([(True, True, True), (False, False, False)] if eval_plus else [(False, True, True)])
    zm, pm = 2 * z, 3 * p
    t = torch.zeros(1)
    dz = _ref_lerp(zm[::2], zm[1::2], t + eps) - zm[::2] if space in ('all', 'z') else torch.zeros_like(zm[::2])
    dp = _ref_lerp(pm[::2], pm[1::2], t + eps) - pm[::2] if space in ('all', 'p') else torch.zeros_like(pm[::2])
    dimg = (dz.flatten(1).double() @ G.wz.double() + dp.flatten(1).double() @ G.wp.double())
    ref = dimg.pow(2).mean(1) / eps ** 2
    assert torch.allclose(d.double(), ref, rtol=2e-2)        # (the toy image difference is formed in fp32: a few digits)
    with pytest.raises(ValueError, match='space'):
        metrics.ppl_distances(s, z, p, space='w', eval_plus=False, use_slerp=False, crop=False, percept=_ToyPercept())
    with pytest.raises(ValueError, match='2B'):
        metrics.ppl_distances(s, z[:5], p[:5], space='all', eval_plus=False, use_slerp=False, crop=False, percept=_ToyPercept())


def test_evaluate_ppl_on_the_toy_generator_is_seeded_and_splits_batches():
    from transeditor_amd import metrics
    from transeditor_amd.inference import GeneratorSampler
    G = _ToyGenerator()
    s = GeneratorSampler(G, use_graph=False)
    state = torch.random.get_rng_state()
    a, da = metrics.evaluate_ppl(s, _ToyPercept(), space='all', n_sample=10, batch=4, seed=5)
    assert torch.equal(torch.random.get_rng_state(), state)          # a seeded run leaves the global state alone
    assert len(G.calls) == 3 and da.shape == (10,) and da.dtype == np.float32
    b, db = metrics.evaluate_ppl(s, _ToyPercept(), space='all', n_sample=10, batch=4, seed=5)
    assert a == b and np.array_equal(da, db) and a == metrics.filter_mean(da)
    c, _ = metrics.evaluate_ppl(s, _ToyPercept(), space='all', n_sample=10, batch=4, seed=6)
    assert c != a
    G.calls.clear()
    metrics.evaluate_ppl(s, _ToyPercept(), space='z', n_sample=8, batch=4, seed=5)
    assert len(G.calls) == 2                                          # no empty remainder batch
    with pytest.raises(ValueError):
        metrics.evaluate_ppl(s, _ToyPercept(), n_sample=0)
    with pytest.raises(ValueError, match='sampling'):
        metrics.evaluate_ppl(s, _ToyPercept(), sampling='middle')


# ------------------------------------------------------------------------------------------------------------------------ CLI
REFERENCE_FLAGS = {        # metrics/evaluate_query.py:256-288
    'truncation': 1, 'truncation_mean': 4096, 'batch': 64, 'n_sample': 50000, 'start_num': 0, 'size': 256, 'inception': None,
    'ckpt': './checkpoint', 'dataset': 'ffhq', 'para_num': 16, 'output_dir': './new_generation', 'channel_multiplier': 2,
    'inject_noise': False, 'num_region': 1, 'no_spatial_map': False, 'num_trans': 8, 'no_trans': False, 'pixel_norm_op_dim': 1,
    'fid': False, 'lpips': False, 'ppl_all': False, 'ppl': False}


def test_cli_flags_and_defaults():
    from transeditor_amd.metrics import build_parser
    args = vars(build_parser().parse_args([]))
    for k, v in REFERENCE_FLAGS.items():
        assert args[k] == v, k
    assert set(REFERENCE_FLAGS) | {'vgg16', 'lpips_lin', 'ppl_n_sample', 'seed'} == set(args)
    assert args['vgg16'] is None and args['lpips_lin'] is None and args['ppl_n_sample'] == 10000 and args['seed'] is None
    args = build_parser().parse_args(['--ckpt', 'c.pt', '--ppl', '--ppl_all', '--vgg16', 'v.pth', '--lpips_lin', 'l.pth', '--batch', '8'])
    assert args.ppl and args.ppl_all and args.ckpt == 'c.pt' and args.batch == 8


def test_cli_configurations():
    from transeditor_amd.metrics import build_parser, ppl_configurations
    p = build_parser()
    assert ppl_configurations(p.parse_args([])) == []
    assert ppl_configurations(p.parse_args(['--ppl'])) == [('all', True, False, True), ('p', True, False, True), ('z', True, False, True)]
    every = ppl_configurations(p.parse_args(['--ppl_all']))
    assert len(every) == 24 and len(set(every)) == 24
    assert every[0] == ('all', True, True, True) and every[-1] == ('z', False, False, False)     # :367-379: crop, slerp, plus, space
    assert len(ppl_configurations(p.parse_args(['--ppl', '--ppl_all']))) == 27


def test_cli_names_what_is_missing(tmp_path):
    from transeditor_amd.metrics import checkpoints, main
    with pytest.raises(SystemExit, match='Inception'):
        main(['--fid'])
    with pytest.raises(SystemExit, match='AlexNet'):
        main(['--lpips'])
    with pytest.raises(SystemExit, match='--ppl'):
        main([])
    with pytest.raises(SystemExit, match='lpips_lin'):
        main(['--ppl'])
    for n in (5, 20, 100):
        (tmp_path / f'{n}.pt').write_bytes(b'')
    assert [x.split('/')[-1] for x in checkpoints(str(tmp_path), 10)] == ['100.pt', '20.pt']      # :301-304: sorted as strings
    assert checkpoints('a/b.pt', 0) == ['a/b.pt']

"""Perceptual path length (transeditor_amd.metrics; metrics/evaluate_query.py:135-249): the paired LPIPS head and the crop / resize
kernel against fp64 restatements, PPL distances against the fp64 CPU oracle with the fp32 reference's own deviation as the yardstick
(tests/golden/ppl64.json, written by tools/ppl_golden.py), and evaluate_ppl / the command line end to end."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_restated as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZE = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def golden_ppl():
    with open(os.path.join(GOLDEN, 'ppl64.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def setup(tmp_path_factory, golden_ppl):
    from transeditor_amd import synth
    from transeditor_amd.inference import GeneratorSampler
    from transeditor_amd.lpips import PerceptualLoss
    from transeditor_amd.model_spatial_query import Generator
    assert golden_ppl['size'] == SIZE
    tmp = tmp_path_factory.mktemp('ppl')
    vp, lp = R.write_weights(tmp, seed=golden_ppl['lpips_seed'])
    G = Generator(SIZE, 512, 512, 2 * (int(np.log2(SIZE)) - 1), n_trans=8, pixel_norm_op_dim=1)
    sd = G.state_dict()
    synth.fill_state_dict(sd, golden_ppl['generator_seed'])
    G.load_state_dict(sd)
    G = G.to(DEV)
    return dict(G=G, sampler=GeneratorSampler(G), sd=sd, percept=PerceptualLoss(vgg_path=vp, lin_path=lp), vgg=vp, lin=lp, tmp=tmp,
                vgg_sd={k: v.double() for k, v in torch.load(vp).items()}, lin_sd={k: v.double() for k, v in torch.load(lp).items()})


# ---------------------------------------------------------------------------------------------------------- (a) the paired head
TAP_SHAPES = [(64, 256), (128, 128), (256, 64), (512, 32), (512, 16),      # relu1_2 ... relu5_3 of a 256 x 256 input
              (64, 128), (128, 64), (256, 32), (512, 16), (512, 8)]        # ... of a 128 x 128 input (cropped 256 px model)


def _head64(f, w):
    """networks_basic.py:65-73 for one layer in float64 on pairs (2n, 2n+1) -> [N]"""
    f = f.double()
    a, b = R.normalize_tensor(f[::2]), R.normalize_tensor(f[1::2])
    return ((a - b) ** 2 * w.double().view(1, -1, 1, 1)).sum(1).mean([1, 2])


def _head32(f, w):
    """the same formula in plain fp32 torch: what fp32 can give on these inputs"""
    a, b = R.normalize_tensor(f[::2]), R.normalize_tensor(f[1::2])
    return ((a - b) ** 2 * w.view(1, -1, 1, 1)).sum(1).mean([1, 2])


def _pair_head(f, w):
    from transeditor_amd import _lib
    return _lib.lpips_dist([_lib.lpips_pair_head_fwd(f, w)], [f.shape[2] * f.shape[3]])


def _tap_features(C, S, kind, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(4, C, S, S, generator=g) + 0.3) * 1.7           # ReLU outputs: non-negative, a third exact zeros
    if kind == 'close':
        f[1::2] = f[::2] * (1 + 1e-4 * torch.randn(2, C, S, S, generator=g))
    f[:, :, 0, 0] = 0                                                          # a pixel of norm 0 on both sides: 0 / 1e-10 = 0
    w = torch.rand(C, generator=g) * 0.1
    return f.to(DEV), w.to(DEV)


@pytest.mark.parametrize('kind', ['unrelated', 'close'])
@pytest.mark.parametrize('C,S', TAP_SHAPES)
def test_pair_head_against_fp64(C, S, kind):
    """Bar: 1e-6 relative to the distance itself (the bar tests/test_gpu_lpips.py holds for distances).  For the pairs 1e-4 apart the
    products f * inv carry half an fp32 ulp each, 6e-4 of a difference of 1e-4: where 1e-6 is out of reach of the number format the
    bar is twice what the plain fp32 torch restatement of the same formula loses on the same inputs, and never tighter than 1e-6.
    Observed on the MI355X, pairs 1e-4 apart (kernel / fp32 torch): 7.1e-7 / 7.2e-7 at 64 x 256^2, 3.9e-7 / 6.5e-7 at 128 x 128^2,
    1.4e-6 / 3.6e-6 at 256 x 64^2, 3.3e-6 / 6.6e-6 at 512 x 32^2, 5.6e-6 / 3.6e-6 at 512 x 16^2, 2.5e-6 / 3.3e-6 at 64 x 128^2,
    4.8e-6 / 4.5e-6 at 128 x 64^2, 8.0e-6 / 4.5e-6 at 256 x 32^2 (the closest to the bar: 1.78 of 2), 2.4e-5 / 1.4e-5 at 512 x 8^2;
    unrelated pairs: kernel <= 2.5e-7."""
    f, w = _tap_features(C, S, kind, 100 * C + S)
    d = _pair_head(f, w)
    ref = _head64(f, w)
    e = float(((d.double() - ref).abs() / ref.abs()).max())
    e32 = float(((_head32(f, w).double() - ref).abs() / ref.abs()).max())
    print(f'pair head C={C} {S}x{S} {kind}: kernel rel err {e:.2e}, fp32 torch restatement {e32:.2e}, distance {float(ref[0]):.3e}')
    assert d.shape == (2,)
    assert e < (1e-6 if kind == 'unrelated' else max(1e-6, 2 * e32))


def test_pair_head_identical_pair_is_zero_and_runs_are_bit_identical():
    for C, S in ((64, 128), (512, 16), (512, 8), (96, 12)):                    # (96 channels, 144 pixels: the tails of both splits)
        f, w = _tap_features(C, S, 'unrelated', 7 * C + S)
        same = f.clone()
        same[1::2] = same[::2]
        assert float(_pair_head(same, w).abs().max()) == 0.0
        a, b = _pair_head(f, w), _pair_head(f, w)
        assert torch.equal(a, b)
        ref = _head64(f, w)
        assert float(((a.double() - ref).abs() / ref.abs()).max()) < 1e-6


def test_pair_distance_against_forward_and_fp64(setup):
    """pair_distance runs the trunk over 2N images at once, forward() over N twice, so the convolutions may take different routes:
    each is within 1e-6 of fp64 (the existing bar), hence within 2e-6 of the other."""
    percept = setup['percept']
    g = torch.Generator().manual_seed(23)
    for size in (128, 64):
        x = (torch.rand(4, 3, size, size, generator=g) * 2 - 1)
        xd = x.to(DEV)
        d = percept.pair_distance(xd)
        fwd = percept(xd[::2].contiguous(), xd[1::2].contiguous()).view(-1)
        ref = R.lpips(x[::2].double(), x[1::2].double(), setup['vgg_sd'], setup['lin_sd']).view(-1)
        e64 = float(((d.double().cpu() - ref).abs() / ref.abs()).max())
        efw = float(((d - fwd).abs() / fwd.abs()).max())
        print(f'pair_distance {size}^2: vs fp64 {e64:.2e}, vs forward() {efw:.2e}')
        assert d.shape == (2,)
        assert e64 < 1e-6 and efw < 2e-6
        assert torch.equal(d, percept.pair_distance(xd))
        same = xd.clone()
        same[1::2] = same[::2]
        assert float(percept.pair_distance(same).abs().max()) == 0.0
    with pytest.raises(ValueError, match='2N'):
        percept.pair_distance(xd[:3])


# ------------------------------------------------------------------------------------------------------------ (b) crop / resize
@pytest.mark.parametrize('size,window,out', [
    (256, (96, 64, 128, 128), 128),        # 256 px, crop: factor 0, a windowed copy
    (512, (192, 128, 256, 256), 256),      # 512 px, crop: factor 1, a windowed copy
    (1024, (384, 256, 512, 512), 256),     # 1024 px, crop: factor 2
    (512, (0, 0, 512, 512), 256),          # 512 px whole: factor 2
    (1024, (0, 0, 1024, 1024), 256),       # 1024 px whole: factor 4
    (1024, (384, 256, 512, 512), 128),     # factor 4 on a window
    (64, (24, 16, 32, 32), 32),            # the 64 px model of the PPL check
])
def test_crop_resize_against_interpolate_fp64(size, window, out):
    from transeditor_amd import _lib
    y0, x0, hc, wc = window
    g = torch.Generator().manual_seed(size + out)
    img = torch.randn(2, 3, size, size, generator=g)
    got = _lib.crop_resize_bilinear(img.to(DEV), y0, x0, hc, wc, out, out)
    win = img[:, :, y0:y0 + hc, x0:x0 + wc].double()
    ref = win if hc == out else F.interpolate(win, size=(out, out), mode='bilinear', align_corners=False)
    e = float((got.double().cpu() - ref).norm() / ref.norm())
    print(f'crop/resize {size} px window {window} -> {out}: rel L2 {e:.2e}')
    assert got.shape == (2, 3, out, out)
    assert e < 1e-6
    if hc == out:
        assert torch.equal(got.cpu(), img[:, :, y0:y0 + hc, x0:x0 + wc])


def test_crop_resize_refuses_a_window_outside_the_image():
    from transeditor_amd import _lib
    img = torch.zeros(1, 3, 64, 64, device=DEV)
    with pytest.raises(RuntimeError):
        _lib.crop_resize_bilinear(img, 40, 16, 32, 32, 32, 32)
    with pytest.raises(RuntimeError):
        _lib.crop_resize_bilinear(img, 0, 0, 48, 48, 32, 32)


def test_lpips_input_follows_the_reference_rule(setup):
    from transeditor_amd.metrics import lpips_input
    g = torch.Generator().manual_seed(2)
    for size in (256, 512):
        img = torch.randn(2, 3, size, size, generator=g)
        for crop in (False, True):
            x = img
            if crop:
                c = size // 8
                x = x[:, :, c * 3:c * 7, c * 2:c * 6]
            if x.shape[2] // 256 > 1:
                x = F.interpolate(x.double(), size=(256, 256), mode='bilinear', align_corners=False)
            got = lpips_input(img.to(DEV), crop)
            assert got.shape == x.shape and got.is_contiguous()
            assert float((got.double().cpu() - x.double()).norm() / x.double().norm()) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- the PPL check
def _endpoint_codes(space, paths, seed):
    """as tools/ppl_golden.py draws them (evaluate_query.py:154-162): the code a space holds fixed is one code repeated"""
    from transeditor_amd import synth
    z, p = synth.latents(2 * paths, seed)
    if space == 'z':
        p = p[:1].repeat(2 * paths, 1, 1)
    if space == 'p':
        z = z[:1].repeat(2 * paths, 1, 1)
    return z, p


def test_ppl_distances_against_fp64_oracle(setup, golden_ppl):
    """Every sample of all 24 configurations against the fp64 CPU oracle (oracle.te_oracle.generator_forward +
    lpips_restated.lpips in float64 from the same endpoint codes; stored by tools/ppl_golden.py).  Yardstick: the same restatement run
    in float32 on the CPU deviates from its float64 run by up to golden['fp32_max_rel_dev'] (2.19e-2 on this input set: the image
    difference sits four digits below the image, two above fp32's resolution); the library may deviate by at most twice that.
    Observed on the MI355X: library 1.99e-2 at most, bar 4.38e-2."""
    from transeditor_amd.metrics import ppl_distances
    bar = 2 * golden_ppl['fp32_max_rel_dev']
    worst, worst_ref = 0.0, 0.0
    failures = []
    for c in golden_ppl['configs']:
        z, p = _endpoint_codes(c['space'], golden_ppl['paths'], golden_ppl['latent_seed'])
        d = ppl_distances(setup['sampler'], z.to(DEV), p.to(DEV), space=c['space'], eval_plus=c['eval_plus'], use_slerp=c['use_slerp'],
                          crop=c['crop'], percept=setup['percept'], eps=golden_ppl['eps'])
        ref = torch.tensor(c['fp64'], dtype=torch.float64)
        dev = ((d.double().cpu() - ref) / ref).abs()
        assert d.shape == ref.shape
        print(f"PPL {c['space']:3s} plus={c['eval_plus']!s:5s} slerp={c['use_slerp']!s:5s} crop={c['crop']!s:5s}: library rel dev "
              f"{[f'{float(x):.2e}' for x in dev]}  fp32 reference {[f'{x:.2e}' for x in c['fp32_rel_dev']]}")
        worst, worst_ref = max(worst, float(dev.max())), max(worst_ref, max(c['fp32_rel_dev']))
        if float(dev.max()) > bar:
            failures.append((c['space'], c['eval_plus'], c['use_slerp'], c['crop'], float(dev.max())))
    print(f'PPL check: library max rel dev {worst:.3e}, fp32 reference max rel dev {worst_ref:.3e}, bar {bar:.3e}')
    assert worst_ref == golden_ppl['fp32_max_rel_dev']
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------- end to end
def test_evaluate_ppl_and_cli_end_to_end(setup, capsys):
    from transeditor_amd import metrics
    kw = dict(space='all', eval_plus=True, use_slerp=False, crop=True, n_sample=10, batch=4, seed=3)
    a, da = metrics.evaluate_ppl(setup['sampler'], setup['percept'], **kw)
    b, db = metrics.evaluate_ppl(setup['sampler'], setup['percept'], **kw)
    assert a == b and np.array_equal(da, db)
    assert da.shape == (10,) and da.dtype == np.float32 and np.isfinite(da).all() and (da > 0).all()
    assert a == metrics.filter_mean(da)
    assert len(setup['sampler']._graphs) <= 4          # this module's sampler: (batch 8, batch 4 | this test: 8, 4) x (mapped, plain)
    fresh = metrics.GeneratorSampler(setup['G'])
    c, _ = metrics.evaluate_ppl(fresh, setup['percept'], **kw)
    assert c == a and len(fresh._graphs) == 2          # one run: the full batch and the remainder
    e, _ = metrics.evaluate_ppl(fresh, setup['percept'], **dict(kw, sampling='full'))
    assert np.isfinite(e)
    ck = setup['tmp'] / 'tiny.pt'
    torch.save({'g_ema': setup['sd']}, str(ck))
    capsys.readouterr()
    res = metrics.main(['--ckpt', str(ck), '--size', str(SIZE), '--ppl', '--ppl_n_sample', '10', '--batch', '4', '--seed', '3',
                        '--vgg16', setup['vgg'], '--lpips_lin', setup['lin']])
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
    assert lines == res and [x['space'] for x in lines] == ['all', 'p', 'z']
    assert all(x['eval_plus'] and x['crop'] and not x['use_slerp'] and x['metric'] == 'ppl' for x in lines)
    assert lines[0]['value'] == a

"""What the tests of the frozen scorers and feature extractors share: the small generator they sample from, the byte levels the
drop-ins hand over, and the plumbing checks (fit_boundaries, score_sweeps, the input checks of a cropping scorer) that are the same
for every scorer.  Importable without a GPU; what differs between two scorers stays in their own test modules."""
import numpy as np
import pytest
import torch


def small_generator(device, seed=5):
    """the 64 px generator with synthetic weights"""
    from transeditor_amd import synth
    from transeditor_amd.model_spatial_query import Generator
    G = Generator(64, 512, 512, 2 * (int(np.log2(64)) - 1), n_trans=8, pixel_norm_op_dim=1)
    sd = G.state_dict()
    synth.fill_state_dict(sd, seed)
    G.load_state_dict(sd)
    return G.to(device)


def levels(x):
    """RGB in [-1, 1] -> BGR byte levels, the preprocessing of the whole image: what the editing scripts hand over"""
    return torch.stack([x[:, 2], x[:, 1], x[:, 0]], 1).clamp(-1, 1).add(1).div(2).mul(255).round()


def check_fit_boundaries(fit_boundaries, generator, scorer, *, score_range=None):
    """40 samples in batches of 16, 16 and 8, 7 + 7 training rows: the result's keys, the scores, both unit boundaries and both reports,
    and a second run that gives all of them again.  score_range = (lo, hi, closed): where the scorer's scores must lie."""
    kw = dict(n_sample=40, batch=16, ratio=0.25, seed=4)
    res = fit_boundaries(generator, scorer, **kw)
    assert set(res) == {'z_boundary', 'p_boundary', 'z_report', 'p_report', 'scores'}
    assert res['scores'].shape == (40, 1) and res['scores'].is_cuda and bool(torch.isfinite(res['scores']).all())
    assert float(res['scores'].std()) > 0
    if score_range is not None:
        lo, hi, closed = score_range
        smin, smax = float(res['scores'].min()), float(res['scores'].max())
        assert (lo <= smin and smax <= hi) if closed else (lo < smin and smax < hi)
    for k in ('z_boundary', 'p_boundary'):
        b = res[k]
        assert b.ndim == 2 and b.shape[0] == 1 and b.shape[1] % 512 == 0 and b.dtype == np.float32
        assert abs(float(np.linalg.norm(b.astype(np.float64))) - 1.0) < 1e-6
    for k in ('z_report', 'p_report'):
        assert res[k]['n_train'] == 14 and res[k]['n_val'] == 6 and res[k]['chosen_num'] == 10
    again = fit_boundaries(generator, scorer, **kw)
    assert torch.equal(again['scores'], res['scores'])
    assert np.array_equal(again['z_boundary'], res['z_boundary']) and np.array_equal(again['p_boundary'], res['p_boundary'])
    assert again['z_report'] == res['z_report'] and again['p_report'] == res['p_report']


def check_score_sweeps(name, scorer, *, size, bitwise, in_unit_range):
    """score_sweeps of 2 origins and 2 x 7 swept images per space in batches of 4, 4, 4 and 2: the origin in the middle, the rest equal to
    one call over the whole sweep - bitwise, or to rtol 1e-5 where another batch split reorders the sums"""
    from transeditor_amd.edit_eval import score_sweeps
    g = torch.Generator().manual_seed(12)
    dev = 'cuda'
    origin = (0.6 * torch.randn(2, 3, size, size, generator=g)).to(dev)
    sweeps = {k: (0.6 * torch.randn(2, 7, 3, size, size, generator=g)).to(dev) for k in ('p', 'z', 'pz')}
    res = score_sweeps({name: scorer}, origin, sweeps, batch=4)
    want = scorer(origin).cpu().numpy()
    for space in ('p', 'z', 'pz'):
        got = res[name][space]
        assert got.shape == (2, 8) and got.dtype == np.float32
        assert np.array_equal(got[:, 3], want)                                                # the origin, in the middle
        each = scorer(sweeps[space].flatten(0, 1)).view(2, 7).cpu().numpy()
        rest = np.delete(got, 3, axis=1)
        assert np.array_equal(rest, each) if bitwise else np.allclose(rest, each, rtol=1e-5, atol=0)
        if in_unit_range:
            assert 0.0 < float(got.min()) and float(got.max()) < 1.0 and float(got.std()) > 0


def check_crop_scorer_inputs(scorer, crop):
    """the refusals of a scorer that crops the centre of a square image, and the smallest image it takes: S == crop, offset 0"""
    dev = 'cuda'
    with pytest.raises(ValueError, match='square'):
        scorer(torch.zeros(1, 3, 2 * crop, 2 * crop - 16, device=dev))
    with pytest.raises(ValueError, match=f'S >= {crop}'):
        scorer(torch.zeros(1, 3, crop - 2, crop - 2, device=dev))
    with pytest.raises(ValueError, match='even'):
        scorer(torch.zeros(1, 3, 2 * crop - 1, 2 * crop - 1, device=dev))
    with pytest.raises(ValueError, match=r'\[B,3,S,S\]'):
        scorer(torch.zeros(1, 1, 2 * crop, 2 * crop, device=dev))
    with pytest.raises(RuntimeError, match='needs a GPU'):
        scorer(torch.zeros(1, 3, 2 * crop, 2 * crop))
    assert scorer(torch.zeros(2, 3, crop, crop, device=dev)).shape == (2,)


def rows_told_apart(s64, bars):
    """the scores of the fp64 restatement lie further apart, row from row, than 100 x the largest bar: the rows are told apart far above it"""
    gaps = (s64.view(-1, 1) - s64.view(1, -1)).abs() + torch.eye(s64.shape[0], dtype=torch.float64) * 1e30
    assert float(gaps.min()) > 100 * float(bars.max())

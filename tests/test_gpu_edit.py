"""transeditor_amd.edit on the GPU: the three kernels of csrc/svm.hip at the binding level against float64, the solver's result
against the optimality conditions of the problem it was given (path-independent), train_boundary end to end against the reference's own
boundaries (tests/golden/boundary_ref.npz, boundary_ref_large.npz), edit_sweep / sample_codes against the GeneratorSampler, and the
command line.  Above 1024 rows a thread of the one-workgroup solver owns several rows (smo_kernel<R>, R = 2 .. 8; the default run
is R = 5): every R against the optimality conditions, and the lowest-index tie rule at each of its three levels on hand-placed ties."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import svm_restated as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ['a', 'b', 'c']
C, EPS = 1.0, 1e-3


@pytest.fixture(scope='module')
def golden():
    out = {}
    for name in ('boundary_ref.npz', 'boundary_ref_large.npz'):                  # cases a, b, c and li_*; case d
        with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    return out


@pytest.fixture(scope='module')
def problems(golden):
    """name -> (x [n,D] float32, y [n] int8): the training sets of the three fixture cases, and n = 2 with one row per class"""
    out = {case: R.training_set(golden[f'{case}_codes'], golden[f'{case}_scores'], R.CASES[case][2]) for case in CASES}
    out['two'] = (np.array([[1.0, 0.5, 0.0], [-1.0, 0.25, 2.0]], np.float32), np.array([1, -1], np.int8))
    return out


@pytest.fixture(scope='module')
def solved(problems):
    """name -> (K float64 numpy: the Gram matrix THE KERNEL returned, alpha, rho, info), one solve each, shared and left unchanged"""
    from transeditor_amd import _lib
    out = {}
    for name, (x, y) in problems.items():
        K = _lib.gram(torch.from_numpy(x).to(DEV))
        alpha, rho, info = _lib.svm_smo(K, y, C, EPS)
        out[name] = (K.cpu().numpy().astype(np.float64), alpha.cpu().numpy(), float(rho.item()), info.cpu().numpy(), K)
    return out


# ---------------------------------------------------------------------------------------------------------- te_gram_f32
def test_gram_against_fp64_symmetric_and_reproducible():
    """Bar: the fp32 fma chain bound of tests/test_gpu_prdc.py for these widths, |K_ij - fp64| <= 2e-6 (|x_i|^2 + |x_j|^2)."""
    from transeditor_amd import _lib
    rng = np.random.default_rng(5)
    worst = 0.0
    for n in (1, 2, 63, 64, 65, 130):
        for D in (1, 7, 36, 96):
            x = rng.standard_normal((n, D)).astype(np.float32)
            xd = torch.from_numpy(x).to(DEV)
            K = _lib.gram(xd)
            again = _lib.gram(xd)
            assert K.shape == (n, n) and K.dtype == torch.float32
            assert torch.equal(K, K.T), (n, D)                                   # the same bits in both triangles
            assert torch.equal(K, again), (n, D)
            x64 = x.astype(np.float64)
            nx = (x64 ** 2).sum(1)
            bar = 2e-6 * (nx[:, None] + nx[None, :])
            err = np.abs(K.cpu().numpy().astype(np.float64) - x64 @ x64.T)
            worst = max(worst, float((err / bar).max()))
            assert np.all(err <= bar), (n, D)
    print(f'gram: max |gpu - fp64| / bar {worst:.3f}')


def test_gram_on_an_unaligned_base():
    from transeditor_amd import _lib
    rng = np.random.default_rng(6)
    buf = torch.from_numpy(rng.standard_normal(1 + 70 * 36).astype(np.float32)).to(DEV)
    x = buf[1:].view(70, 36)                                                     # D % 4 == 0 but the base is 4 bytes off: scalar loads
    assert x.data_ptr() % 16 != 0
    assert torch.equal(_lib.gram(x), _lib.gram(x.clone()))


# ---------------------------------------------------------------------------------------------------------- te_svm_smo_f64
@pytest.mark.parametrize('name', CASES + ['two'])
def test_smo_meets_the_optimality_conditions_of_its_problem(problems, solved, name):
    """Nothing here depends on the solver's path: feasibility exactly, and the violation Gmax - Gmin recomputed in float64 from the
    returned alpha and the Gram matrix the kernel was given; only the float64 rounding of the incremental gradient is left."""
    _, y = problems[name]
    K, alpha, rho, info, _ = solved[name]
    n = len(y)
    assert alpha.dtype == np.float64 and alpha.shape == (n,)
    assert alpha.min() >= 0.0 and alpha.max() <= C
    assert abs(float(alpha @ y.astype(np.float64))) <= n * C * 2.0 ** -52
    viol = R.violation(K, y, alpha, C)
    want_alpha, want_rho, want_it, conv = R.smo(K, y, C, EPS)
    print(f'{name}: n {n}, {info[0]} iterations (restatement on the same Gram: {want_it}), violation {viol:.6e}, rho {rho:.6f} '
          f'(restatement {want_rho:.6f}), {int((alpha >= C).sum())} alphas at C, {int((alpha > 0).sum())} support vectors')
    assert viol < EPS * (1 + 1e-6)
    assert info[1] == 1 and conv
    assert want_it / 2 <= info[0] <= want_it * 2
    gmax, gmin = R.extremes(K, y, alpha, C)                                      # calculate_rho: a mean or a midpoint of values in [-Gmax, -Gmin]
    assert -gmax - 1e-9 <= rho <= -gmin + 1e-9
    if name == 'b':
        assert (alpha >= C).sum() > 20


def test_smo_is_bit_reproducible(solved):
    from transeditor_amd import _lib
    for name in ('b', 'two'):
        K, alpha, rho, info, Kd = solved[name]
        y = np.concatenate([np.ones(len(alpha) // 2, np.int8), -np.ones(len(alpha) // 2, np.int8)])
        a2, r2, i2 = _lib.svm_smo(Kd, y, C, EPS)
        assert a2.cpu().numpy().tobytes() == alpha.tobytes() and float(r2.item()) == rho and np.array_equal(i2.cpu().numpy(), info)


def test_smo_stops_at_max_iter_and_the_wrapper_warns(golden, problems, solved):
    from transeditor_amd import _lib, edit
    _, y = problems['b']
    alpha, rho, info = _lib.svm_smo(solved['b'][4], y, C, EPS, max_iter=5)
    alpha = alpha.cpu().numpy()
    assert info.tolist() == [5, 0] and np.isfinite(float(rho.item()))
    assert alpha.min() >= 0.0 and alpha.max() <= C and abs(float(alpha @ y.astype(np.float64))) <= len(y) * C * 2.0 ** -52
    assert (alpha > 0).sum() >= 2
    with pytest.warns(RuntimeWarning, match='max_iter'):
        boundary, report = edit.train_boundary(golden['b_codes'], golden['b_scores'], R.CASES['b'][2], split_ratio=1.0, max_iter=5)
    assert report['converged'] is False and report['iterations'] == 5 and boundary.shape == (1, 8)


def test_smo_refuses_bad_arguments_before_any_launch(solved):
    from transeditor_amd import _lib
    L = _lib.lib()
    Kd = solved['a'][4]
    n = Kd.shape[0]
    alpha = torch.full((n,), -7.0, device=DEV, dtype=torch.float64)
    rho = torch.full((1,), -7.0, device=DEV, dtype=torch.float64)
    info = torch.full((2,), -7, device=DEV, dtype=torch.int32)
    y = np.concatenate([np.ones(8192, np.int8), -np.ones(1, np.int8)])
    st = torch.cuda.current_stream().cuda_stream
    call = lambda yy, nn: L.te_svm_smo_f64(alpha.data_ptr(), rho.data_ptr(), info.data_ptr(), Kd.data_ptr(), yy.ctypes.data, nn, C, EPS, 10, st)
    assert call(y, 1) == -2                                                      # TE_ERR_SHAPE
    assert call(y, 8193) == -2
    assert call(np.ones(n, np.int8), n) == -2 and call(-np.ones(n, np.int8), n) == -2        # a single class
    torch.cuda.synchronize()
    assert bool((alpha == -7.0).all()) and float(rho.item()) == -7.0 and info.tolist() == [-7, -7]      # nothing ran
    with pytest.raises(RuntimeError, match='both labels'):
        _lib.svm_smo(Kd, np.ones(n, np.int8), C, EPS)


# ---------------------------------------------------------------------------------------------------------- above 1024 rows
# (n, hardest rows last): every instantiation R = ceil(n / 1024) = 2 .. 8, the edges 1025 / 2048 / 2049 / 8192 and the default run's
# 4200.  Hardest last: every support vector, so every selected i and j, lies in the last slots; the random order puts them in all.
LARGE = [(1025, True), (2048, True), (2049, True), (4096, True), (4200, True), (4200, False), (5121, True), (7000, True), (8192, True)]


@pytest.mark.parametrize('n,hardest_last', LARGE)
def test_smo_above_1024_rows_meets_the_optimality_conditions_of_its_problem(n, hardest_last):
    """test_smo_meets_the_optimality_conditions_of_its_problem where thread t owns the rows t, t + 1024, ...: D = 16, margin 0.5, label
    noise 0.3 (svm_restated.margin_problem), C = 1, eps = 1e-3.  The restatement runs on the Gram matrix the kernel was given."""
    from transeditor_amd import _lib
    x, y = R.margin_problem(n, hardest_last=hardest_last)
    Kd = _lib.gram(torch.from_numpy(x).to(DEV))
    alpha, rho, info = _lib.svm_smo(Kd, y, C, EPS)
    alpha, rho, info = alpha.cpu().numpy(), float(rho.item()), info.cpu().numpy()
    K = Kd.cpu().numpy().astype(np.float64)                                      # the one float64 copy of this case
    del Kd
    slots = (n + R.SLOT - 1) // R.SLOT
    assert alpha.dtype == np.float64 and alpha.shape == (n,)
    assert alpha.min() >= 0.0 and alpha.max() <= C
    assert abs(float(alpha @ y.astype(np.float64))) <= n * C * 2.0 ** -52
    viol = R.violation(K, y, alpha, C)
    want_alpha, want_rho, want_it, conv = R.smo(K, y, C, EPS)
    sv, want_sv = np.nonzero(alpha > 0)[0], np.nonzero(want_alpha > 0)[0]
    print(f'n {n} R {slots} {"hardest last" if hardest_last else "random order"}: {info[0]} iterations (restatement on the same Gram: '
          f'{want_it}), violation {viol:.6e}, rho {rho:.6f} (restatement {want_rho:.6f}), {int((alpha >= C).sum())} alphas at C, '
          f'{len(sv)} support vectors in slots {R.slots(sv)} (restatement {len(want_sv)} in {R.slots(want_sv)})')
    assert viol < EPS * (1 + 1e-6)
    assert info[1] == 1 and conv
    assert want_it / 2 <= info[0] <= want_it * 2
    gmax, gmin = R.extremes(K, y, alpha, C)
    assert -gmax - 1e-9 <= rho <= -gmin + 1e-9
    if hardest_last:                                                             # a property of the input: the top slot is in use
        assert want_sv.max() >= R.SLOT * (slots - 1) and sv.max() >= R.SLOT * (slots - 1)
    else:
        assert R.slots(want_sv) == list(range(slots)) and R.slots(sv) == list(range(slots))
    del K


@pytest.mark.parametrize('C_', [1.0, 0.125])
@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('layout', list(R.TIE_LAYOUTS))
def test_smo_ties_go_to_the_lowest_index_at_every_level(layout, flip, C_):
    """svm_restated.tie_problem: K is built on the host from two rows, so all rows of a class are the same bits and every selection is a
    tie among all candidates of a class; the layouts put the two lowest candidates where a wrong preference per thread, across lanes
    or across waves would pick the other (flip: the placed class is -1, so selection B meets the tie that selection A met).  C = 1:
    one iteration, two support vectors; C = 0.125: the box fills the four lowest rows of each class in order."""
    from transeditor_amd import _lib
    K, y = R.tie_problem(layout, flip)
    Kd = torch.from_numpy(K).to(DEV)
    runs = []
    for _ in range(2):
        alpha, rho, info = _lib.svm_smo(Kd, y, C_, EPS)
        runs.append((alpha.cpu().numpy(), float(rho.item()), info.cpu().numpy()))
    alpha, rho, info = runs[0]
    want_alpha, want_rho, want_it, conv = R.smo(K, y, C_, EPS)
    support, k = R.tie_support(y, C_)
    assert conv and want_it == k and np.nonzero(want_alpha > 0)[0].tolist() == support   # the restatement gives the hand-derived answer
    print(f'{layout} flip {flip} C {C_}: support {np.nonzero(alpha > 0)[0].tolist()} (restatement {support}), {info[0]} iterations '
          f'({want_it}), max |alpha - restatement| {np.abs(alpha - want_alpha).max():.2e}, rho {rho!r} ({want_rho!r})')
    assert np.nonzero(alpha > 0)[0].tolist() == support
    assert info.tolist() == [want_it, 1]
    assert np.abs(alpha - want_alpha).max() <= 1e-12 and abs(rho - want_rho) <= 1e-12
    assert runs[1][0].tobytes() == alpha.tobytes() and runs[1][1] == rho and np.array_equal(runs[1][2], info)


def test_smo_at_4200_rows_is_bit_reproducible_and_stops_at_max_iter():
    from transeditor_amd import _lib
    x, y = R.margin_problem(4200, hardest_last=False)
    Kd = _lib.gram(torch.from_numpy(x).to(DEV))
    a1, r1, i1 = _lib.svm_smo(Kd, y, C, EPS)
    a2, r2, i2 = _lib.svm_smo(Kd, y, C, EPS)
    assert i1.tolist()[1] == 1 and i1.tolist()[0] > 1000
    assert a1.cpu().numpy().tobytes() == a2.cpu().numpy().tobytes() and r1.cpu().numpy().tobytes() == r2.cpu().numpy().tobytes()
    assert i1.cpu().numpy().tobytes() == i2.cpu().numpy().tobytes()
    alpha, rho, info = _lib.svm_smo(Kd, y, C, EPS, max_iter=7)
    alpha = alpha.cpu().numpy()
    assert info.tolist() == [7, 0] and np.isfinite(float(rho.item()))
    assert alpha.min() >= 0.0 and alpha.max() <= C and abs(float(alpha @ y.astype(np.float64))) <= len(y) * C * 2.0 ** -52
    assert (alpha > 0).sum() >= 2


@pytest.mark.parametrize('D', [16, 33])
@pytest.mark.parametrize('n', [1025, 4200])
def test_gram_above_1024_rows_against_fp64_symmetric_and_reproducible(n, D):
    """9 and 33 tiles per side, the 16-byte (D = 16) and the scalar (D = 33) loads; the bar of
    test_gram_against_fp64_symmetric_and_reproducible."""
    from transeditor_amd import _lib
    x = np.random.default_rng(100 * n + D).standard_normal((n, D)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    K = _lib.gram(xd)
    again = _lib.gram(xd)
    assert K.shape == (n, n) and K.dtype == torch.float32
    assert torch.equal(K, K.T)
    assert torch.equal(K, again)
    x64 = x.astype(np.float64)
    nx = (x64 ** 2).sum(1)
    bar = 2e-6 * (nx[:, None] + nx[None, :])
    err = np.abs(K.cpu().numpy().astype(np.float64) - x64 @ x64.T)
    print(f'gram n {n} D {D}: max |gpu - fp64| / bar {float((err / bar).max()):.3f}')
    assert np.all(err <= bar)


def test_coef_at_8192_rows_within_one_ulp_of_the_fp64_sum():
    from transeditor_amd import _lib
    rng = np.random.default_rng(9)
    n, D = 8192, 65
    x = rng.standard_normal((n, D)).astype(np.float32)
    kind = rng.random(n)                                                         # as a solve leaves them: most 0, some at C, a few free
    alpha = np.where(kind < 0.8, 0.0, np.where(kind < 0.95, 1.0, rng.random(n)))
    assert (alpha == 0).sum() > 6000 and (alpha == 1).sum() > 1000 and alpha[-1024:].any()
    y = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int8)
    w = _lib.svm_coef(torch.from_numpy(x).to(DEV), torch.from_numpy(alpha).to(DEV), y).cpu().numpy()
    want = ((alpha * y) @ x.astype(np.float64)).astype(np.float32)
    assert w.dtype == np.float32 and w.shape == (D,)
    assert np.all(np.abs(w.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------- te_svm_coef_f32
def test_coef_within_one_ulp_of_the_fp64_sum():
    from transeditor_amd import _lib
    rng = np.random.default_rng(8)
    for n, D in ((1, 1), (130, 65), (200, 96), (57, 300)):
        x = rng.standard_normal((n, D)).astype(np.float32)
        alpha = rng.random(n) * (rng.random(n) < 0.6)                             # some exact zeros, as a solve leaves them
        y = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int8)
        w = _lib.svm_coef(torch.from_numpy(x).to(DEV), torch.from_numpy(alpha).to(DEV), y).cpu().numpy()
        want = ((alpha * y) @ x.astype(np.float64)).astype(np.float32)
        assert w.dtype == np.float32 and w.shape == (D,)
        assert np.all(np.abs(w.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)), (n, D)


# ---------------------------------------------------------------------------------------------------------- train_boundary
@pytest.mark.parametrize('case', CASES + ['d'])
def test_train_boundary_end_to_end(golden, case):
    """1 - cos to the stored float64 optimum: at most 4x the larger of the reference's and the restatement's own value on this case.
    All three are eps = 1e-3 solutions of one strictly convex problem; 4x in 1 - cos is 2x in angle, the room for two eps-optimal
    solutions on opposite sides of the optimum.  The value is printed before it is asserted."""
    from transeditor_amd import edit
    codes, scores, ratio = golden[f'{case}_codes'], golden[f'{case}_scores'], R.CASES[case][2]
    boundary, report = edit.train_boundary(codes, scores, ratio, split_ratio=1.0)
    assert boundary.shape == (1, codes.shape[1]) and boundary.dtype == np.float32
    assert abs(float(np.linalg.norm(boundary.astype(np.float64))) - 1.0) <= 1e-6
    assert float(boundary[0].astype(np.float64) @ golden[f'{case}_boundary'][0].astype(np.float64)) > 0
    gap = R.one_minus_cos(boundary, golden[f'{case}_optimum'])
    bar = 4 * max(float(golden[f'{case}_gap_ref']), float(golden[f'{case}_gap_restated']))
    print(f'case {case}: 1 - cos GPU boundary to the fp64 optimum {gap:.2e} (bar {bar:.2e}), to the reference '
          f'{R.one_minus_cos(boundary, golden[f"{case}_boundary"]):.2e}; report {report}')
    assert gap <= bar
    x, y = R.training_set(codes, scores, ratio)
    f = x.astype(np.float64) @ boundary[0].astype(np.float64) - report['rho'] / report['norm']
    assert report['train_accuracy'] == float(((f > 0) == (y > 0)).mean()) and report['val_accuracy'] is None
    assert report['converged'] is True and report['n_train'] == len(y) and report['n_val'] == 0
    assert 0 < report['n_support'] <= len(y) and report['iterations'] > 0
    if case in ('a', 'c'):                                                       # b and d are not separable
        assert report['train_accuracy'] == 1.0
    # a validation split, and device tensors in place of numpy: the same bits
    b1, r1 = edit.train_boundary(codes, scores, ratio, split_ratio=0.7, seed=4)
    b2, r2 = edit.train_boundary(torch.from_numpy(codes).to(DEV), torch.from_numpy(scores).to(DEV), ratio, split_ratio=0.7, seed=4)
    assert b1.tobytes() == b2.tobytes() and r1 == r2
    sel = edit.select_extremes(codes, scores, ratio, split_ratio=0.7, seed=4)
    val = np.concatenate([codes[sel['val_pos'].numpy()], codes[sel['val_neg'].numpy()]]).astype(np.float64)
    fv = val @ b1[0].astype(np.float64) - r1['rho'] / r1['norm']
    nv = sel['val_pos'].numel()
    assert r1['n_val'] == 2 * nv and r1['val_accuracy'] == float(((fv[:nv] > 0).sum() + (fv[nv:] <= 0).sum()) / (2 * nv))


# ---------------------------------------------------------------------------------------------------------- the generator loops
@pytest.fixture(scope='module')
def sampler():
    from transeditor_amd import synth
    from transeditor_amd.inference import GeneratorSampler
    from transeditor_amd.model_spatial_query import Generator
    G = Generator(32, 512, 512, 8, n_trans=8, pixel_norm_op_dim=1)
    sd = G.state_dict()
    synth.fill_state_dict(sd, 21)
    G.load_state_dict(sd)
    return GeneratorSampler(G.to(DEV)), sd


def _unit(D, seed):
    b = torch.randn(1, D, generator=torch.Generator().manual_seed(seed))
    return (b / b.norm()).to(DEV)


def test_edit_sweep_equals_the_sampler_on_the_same_codes(sampler):
    from transeditor_amd import edit
    g, _ = sampler
    count, steps, batch, latent = 2, 3, 4, 512
    gen = torch.Generator().manual_seed(3)
    z_plus, p_plus = torch.randn(count, latent, 16, generator=gen).to(DEV), torch.randn(count, latent, 16, generator=gen).to(DEV)
    zb, pb = _unit(16 * latent, 1), _unit(16 * latent, 2)
    out = edit.edit_sweep(g, z_plus, p_plus, zb.cpu().numpy(), pb, z_distance=3.0, p_distance=(-1.0, 2.0), steps=steps, batch=batch)
    assert set(out) == {'p', 'z', 'pz'}

    def codes(mapped, boundary, start, end):                                     # built here, with the fixture-checked interpolation
        rows = [edit.linear_interpolate(mapped[i:i + 1].transpose(1, 2).reshape(1, -1), boundary, start, end, steps) for i in range(count)]
        return torch.cat(rows).reshape(count * steps, 16, latent).transpose(1, 2).contiguous()
    zm, pm = codes(z_plus, zb, -3.0, 3.0), codes(p_plus, pb, -1.0, 2.0)
    zs, ps = z_plus.repeat_interleave(steps, 0), p_plus.repeat_interleave(steps, 0)
    assert not torch.equal(zm, zs.contiguous())
    for name, (z, p) in {'p': (zs, pm), 'z': (zm, ps), 'pz': (zm, pm)}.items():
        want = torch.cat([g(z[at:at + batch].contiguous(), p[at:at + batch].contiguous(), use_style_mapping=False,
                            use_spatial_mapping=False)[0] for at in range(0, count * steps, batch)])
        assert out[name].shape == (count, steps, 3, 32, 32) and out[name].is_cuda
        assert torch.equal(out[name].flatten(0, 1), want), name
    # the W+ form at distance 0 in both spaces: the unedited image
    still = edit.edit_sweep(g, z_plus, p_plus, _unit(latent, 5), _unit(latent, 6), z_distance=0.0, p_distance=0.0, steps=steps, batch=batch)
    plain = torch.cat([g(zs[at:at + batch].contiguous(), ps[at:at + batch].contiguous(), use_style_mapping=False,
                         use_spatial_mapping=False)[0] for at in range(0, count * steps, batch)])
    assert torch.equal(still['pz'].flatten(0, 1), plain)
    moved = edit.edit_sweep(g, z_plus, p_plus, _unit(latent, 5), _unit(latent, 6), z_distance=2.0, p_distance=0.0, steps=steps, batch=batch)
    assert torch.equal(moved['p'].flatten(0, 1), plain)
    assert not torch.equal(moved['z'][:, 0], still['z'][:, 0])


def test_sample_codes_shapes_device_and_rng(sampler):
    from transeditor_amd import edit
    g, _ = sampler
    score = lambda image: image[:, 1].mean((1, 2))
    state = torch.cuda.get_rng_state()
    z, p, s = edit.sample_codes(g, score, n_sample=10, batch=4, seed=5)
    assert torch.equal(state, torch.cuda.get_rng_state())                        # the seed idiom leaves the global state alone
    assert z.shape == (10, 16 * 512) and p.shape == (10, 16 * 512) and s.shape == (10, 1)
    assert z.is_cuda and p.is_cuda and s.is_cuda and z.dtype == p.dtype == s.dtype == torch.float32
    z2, p2, s2 = edit.sample_codes(g, score, n_sample=10, batch=4, seed=5)
    assert torch.equal(z, z2) and torch.equal(p, p2) and torch.equal(s, s2)
    # the layout: row i holds token 0's 512 values first; the scores are those of the images rendered from the mapped codes
    image = g(edit.unflatten_codes(z[:4], 512), edit.unflatten_codes(p[:4], 512), use_style_mapping=False, use_spatial_mapping=False)[0]
    assert torch.equal(score(image).view(4, 1), s[:4])
    with pytest.raises(ValueError):
        edit.sample_codes(g, score, n_sample=0, batch=4)


# ---------------------------------------------------------------------------------------------------------- CLI
def test_command_line_boundary_mode(tmp_path, capsys, golden):
    from transeditor_amd import edit
    cp, sp, bp = str(tmp_path / 'c.npy'), str(tmp_path / 's.npy'), str(tmp_path / 'b.npy')
    np.save(cp, golden['c_codes'])
    np.save(sp, golden['c_scores'][:, 0])
    direct, report = edit.train_boundary(golden['c_codes'], golden['c_scores'], 0.1, 0.7, seed=2)
    capsys.readouterr()
    edit.main(['--codes', cp, '--scores', sp, '--write_boundary', bp, '--ratio', '0.1', '--seed', '2'])
    lines = [x for x in capsys.readouterr().out.splitlines() if x.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out['mode'] == 'boundary' and out['n'] == 600 and out['dim'] == 33 and {k: out[k] for k in report} == report
    assert np.load(bp).tobytes() == direct.tobytes()


def test_command_line_sweep_mode(tmp_path, capsys, sampler):
    from transeditor_amd import edit
    _, sd = sampler
    ck, zp, pp, op = (str(tmp_path / n) for n in ('1.pt', 'z.npy', 'p.npy', 'sweep.npz'))
    torch.save({'g_ema': sd}, ck)
    np.save(zp, _unit(16 * 512, 1).cpu().numpy())
    np.save(pp, _unit(16 * 512, 2).cpu().numpy())
    capsys.readouterr()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        edit.main(['--ckpt', ck, '--size', '32', '--z_boundary', zp, '--p_boundary', pp, '--z_distance', '3', '--p_distance', '2',
                   '--steps', '3', '--n', '2', '--seed', '1', '--batch', '4', '--out', op])
    lines = [x for x in capsys.readouterr().out.splitlines() if x.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out['mode'] == 'sweep' and out['n'] == 2 and out['steps'] == 3 and out['wrote'] == op
    with np.load(op) as z:
        assert set(z.files) == {'origin', 'p', 'z', 'pz'}
        assert z['origin'].shape == (2, 32, 32, 3) and z['origin'].dtype == np.uint8
        assert all(z[k].shape == (2, 3, 32, 32, 3) and z[k].dtype == np.uint8 for k in ('p', 'z', 'pz'))
        assert not np.array_equal(z['z'][:, 0], z['z'][:, 2])

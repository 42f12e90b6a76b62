"""The form table of the FIR kernels (tests/fir_forms.py) against the library's own plan, without a GPU: every entry lands on the key it
declares, the table has the coverage that REQUIRED lists, no kernel that the query can name over the host-plan grid lacks an entry, the
act entries stay off the kink, and the four instruments are proven on a plain-torch model of the kernels (tests/fir_model.py): they pass
on the model and each planted defect fails the instrument named for it.
"""
import dataclasses

import pytest
import torch

import fir_forms as ff
import fir_model
import host_plans as hp
from fp64_check import KINK_CAP, U32
from transeditor_amd import _lib

IDS = lambda e: e.name


@pytest.mark.parametrize('entry', ff.TABLE, ids=IDS)
def test_entry_lands_on_its_key(entry):
    ff.check(entry)


def test_table_has_the_required_coverage():
    missing = [what for what, pred in ff.REQUIRED if not any(pred(e) for e in ff.TABLE)]
    assert not missing, f'no entry for: {missing}'
    assert len({e.key for e in ff.TABLE if e.key[0] == 'blur44'}) == 24
    for e in ff.TABLE:
        assert e.H != e.W and e.pad[:2] != e.pad[2:] and e.planes in (1, 5, 11) and e.bias in (0, ff.SIZE_B)
        assert max(e.H, e.W) <= 140, f'{e.name}: too big for a form test'


def test_query_names_no_kernel_without_an_entry():
    """te_fir_form over the FIR grid of tests/host_plans.py under the three ops: every (kernel, MODE, D, EXT) it names has an entry, and
    the older queries are views of the same plan"""
    L = _lib.lib()
    have = {e.key for e in ff.TABLE}
    seen, lacking = set(), {}
    grids = [(0, g) for g in hp.fir_grid()] + [(op, (m, h, w, 1, kh, kw, 1, 1, 1, 1, *pads)) for op in (1, 2) for m, h, w, kh, kw, *pads in hp.blur_grid()]
    plan = {0: L.te_upfirdn2d_plan, 1: L.te_blur_actgrad_plan, 2: L.te_blur_gradact_plan}
    for op, g in grids:
        rc, *form = hp._fir_form(L, op, *g)
        if rc:
            assert all(v == -1 for v in form), (op, g)
            continue
        f = dict(zip(_lib.FIR_FORM, form))
        key = (_lib.FIR_KERNELS[f['kernel']], f['mode'], f['D'], f['ext'])
        seen.add(key)
        if key not in have:
            lacking.setdefault(key, (op, g))
        walks = f['kernel'] != 0
        args = g if op == 0 else (g[0], g[1], g[2], g[4], g[5], *g[10:])
        assert hp._two(plan[op], *args) == (0, f['zgroups'], f['tiles_x'] * f['tiles_y']), (op, g, f)
        if op and walks:
            assert L.te_blur_actgrad_tiles(*args[1:]) == f['tiles_x'] * f['tiles_y']
        assert f['ext'] == (f['ext_x'] or f['ext_y']) and f['threads'] == 256
    assert not lacking, f'kernels without an entry (first problem each): {lacking}'
    assert len(seen) >= 20


def test_refusals_are_the_launch_s_and_leave_the_form_alone():
    L = _lib.lib()
    for op, args in ((3, (5, 8, 9, 1, 4, 4, 1, 1, 1, 1, 2, 1, 1, 2)), (1, (5, 8, 9, 1, 4, 4, 1, 1, 1, 1, -1, 2, 1, 2)), (2, (5, 8, 3, 1, 4, 4, 1, 1, 1, 1, 2, 1, 1, 2)),
                     (1, (5, 8, 9, 1, 3, 3, 1, 1, 1, 1, 2, 1, 1, 2)), (0, (0, 8, 9, 1, 4, 4, 1, 1, 1, 1, 2, 1, 1, 2)), (2, (1 << 30, 8, 9, 1, 4, 4, 1, 1, 1, 1, 2, 1, 1, 2)),
                     (0, (5, 8, 9, 1, 4, 4, 1, 1, 1, 1, 0, 0, -9, 0))):
        rc, *form = hp._fir_form(L, op, *args)
        assert rc < 0 and all(v == -1 for v in form), (op, args, rc, form)
    assert L.te_fir_form(0, 5, 8, 9, 1, 4, 4, 1, 1, 1, 1, 2, 1, 1, 2, None) < 0


ACT = [e for e in ff.TABLE if e.act]


@pytest.mark.parametrize('entry', ACT, ids=IDS)
def test_act_entries_stay_off_the_kink(entry):
    share = ff.kink_share(entry, ff.check(entry))
    assert share <= KINK_CAP, f'{entry.name}: {share:.2e} of the elements sit on the kink: give the entry another data key'


def _all_instruments(e, f, launch):
    ops, opx = ff.operands(e), ff.operands(e, exact=True)
    run, runx = launch(e, f, ops), launch(e, f, opx)
    R, Rx = ff.reference(e, f, ops), ff.reference(e, f, opx)
    ff.guards(e, run)
    ff.guards(e, runx)
    ff.elementwise(e, R, run)
    ff.per_tile(e, R, run)
    ff.exact(e, Rx, runx)


@pytest.mark.parametrize('entry', ff.TABLE, ids=IDS)
def test_instruments_pass_on_the_model(entry):
    _all_instruments(entry, ff.check(entry), fir_model.launch)


def _entry(op, tag, **where):
    found = [e for e in ff.TABLE if e.op == op and e.name.endswith('_' + tag) and all(getattr(e, k) == v for k, v in where.items())]
    assert found, (op, tag, where)
    return found[0]


def _fails(instrument, e, f, defect, exact=False):
    ops = ff.operands(e, exact=exact)
    run = fir_model.launch(e, f, ops, defect)
    R = ff.reference(e, f, ops)
    with pytest.raises(AssertionError):
        instrument(e, R, run) if instrument is not ff.guards else ff.guards(e, run)


@pytest.mark.parametrize('defect', ('swap_pads', 'flip_x', 'transpose', 'shift'))
@pytest.mark.parametrize('op', (ff.UP, ff.AG, ff.GA))
def test_elementwise_bound_catches(op, defect):
    """pads that differ between the axes, taps that equal neither their transpose nor a flip, a right-edge group that is shifted (s = 3)"""
    e = _entry(op, 'ext', sit=('both', '1x1', 3, 'plain'))
    _fails(ff.elementwise, e, ff.check(e), defect)


def _summed_bias_figure(defect, one_plane=False):
    """max err / bound of the summed bias gradient as tests/test_gpu_loop_trips.py::test_blur_actgrad checks it, at its 4-tile shape
    (4 x 409 x 40 x 70, gpad (1, 2, 1, 2)), for the model with `defect` in every plane or in plane 0 only"""
    B, Cn = 4, 409
    e = ff.Entry('summed', ff.AG, B * Cn, 40, 70, (1, 2, 1, 2), 'k44', 0, 0, 0, 'float32', (1, 1), (1, 1), 1, ('blur44', 1, 3, 0), (), '')
    f = ff.answer(e)
    assert (f['tiles_x'], f['tiles_y']) == (2, 2)
    ops = ff.operands(e)
    part = fir_model.launch(e, f, ops, defect).part
    if one_plane:
        sound = fir_model.launch(e, f, ops).part
        assert not torch.equal(sound[0], part[0])
        sound[0] = part[0]
        part = sound
    gb = part.view(B, Cn, 4).sum(dim=(0, 2))
    s = (ops.x.double() * ff.slope64(ops.ref, *ff.slopes(ops))).view(B, Cn, 40, 70)
    L = B * 40 * 70
    return float(((gb.double() - s.sum(dim=(0, 2, 3))).abs() / ((L + 1) * U32 * s.abs().sum(dim=(0, 2, 3)))).max())


@pytest.mark.parametrize('defect', ('double_own', 'drop_halo'))
def test_per_tile_instruments_catch_ownership_defects(defect):
    """the gap that the per-tile instruments close, written down.  The loop-trip test holds the SUMMED bias gradient to (L + 1) u sum |s|,
    about 5.0 at its 4-tile shape.  An element owned twice at a tile border, or the last tile's rows of the halo column dropped, in one
    plane of a channel stays inside that bound; the same defect in every plane exceeds it only through the worst of the 409 channels
    (both figures are printed).  On the table's entries the exact per-tile check fails for either defect wherever there are two tiles along
    x, in every plane; the dropped column also fails the per-tile bound on the normal operands."""
    assert _summed_bias_figure(None) < 0.1
    one, every = _summed_bias_figure(defect, one_plane=True), _summed_bias_figure(defect)
    print(f'{defect}: summed bias gradient max err / bound {one:.3f} with the defect in one plane, {every:.3f} in every plane')
    assert 0.01 < one <= 1.0, f'the summed bound does catch it in a single plane ({one:.3f}); the docstring is out of date'
    for tag in ('four', 'past', 'ext4', 'tx'):
        e = _entry(ff.AG, tag)
        _fails(ff.exact, e, ff.check(e), defect, exact=True)
    if defect == 'drop_halo':
        e = _entry(ff.AG, 'four')
        _fails(ff.per_tile, e, ff.check(e), defect)


@pytest.mark.parametrize('op', (ff.UP, ff.AG, ff.GA))
def test_guards_catch_the_ext_column_under_the_row_s_flag(op):
    """ext x only: the 65th column is never written; ext y only: a 41st element is written past every row of the last tile"""
    for out_hw in ((20, 65), (33, 40)):
        e = [t for t in ff.TABLE if t.op == op and t.name.endswith('_ext') and ff.out_hw(t) == out_hw][0]
        _fails(ff.guards, e, ff.check(e), 'ext_flag')


def test_exact_operands_are_exact_in_any_order():
    """every product and partial sum of the EXACT set is a multiple of 1/2 below 2^23: an fp32 sum in random order equals the fp64 one"""
    e = _entry(ff.GA, 'ext4')
    f = ff.check(e)
    Rx = ff.reference(e, f, ff.operands(e, exact=True))
    for t, r, c in ff.owned(e, f):
        terms = Rx['y'][0, r, c].reshape(-1)
        terms = terms[torch.randperm(terms.numel(), generator=torch.Generator().manual_seed(t))].float()
        acc = torch.zeros((), dtype=torch.float32)
        for v in terms:
            acc = acc + v
        assert float(acc) == float(Rx['part'][0, t])


def test_one_plane_twin_of_an_entry_is_the_same_form():
    for e in ff.TABLE:
        if e.planes == 11 and e.key[0] != 'direct':
            f, f1 = ff.answer(e), ff.answer(dataclasses.replace(e, planes=1))
            assert all(f[k] == f1[k] for k in _lib.FIR_FORM if k not in ('zgroups', 'grid_x')), e.name

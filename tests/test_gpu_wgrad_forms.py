"""Every form of the fp32 weight-gradient kernel (tests/wgrad_forms.py) against fp64, slab by slab and elementwise, launched directly:
_lib.wgrad_slabs with the entry's own S and NB, so that no planner chooses the chunking.  Each test re-asserts its entry's key
(kind, nwp, wino, vec, db) and per-block facts through te_wgrad_form before it compares numbers.

Reference: a plain restatement from slices in fp64 on the operands' device (wgrad_forms.reference),
    3x3, 1x1   slab[co, ci, ky, kx] = sum_p g[co, p] xpad[ci, p + (ky, kx)]
    T2         slab[co, ci, ky, kx] = sum_ij g[co, 2i + ky, 2j + kx] x[ci, i, j]
restricted to the chunk by zeroing the cell-side operand (g; x for T2) outside the tiles [n_tiles s / S, n_tiles (s + 1) / S) of the group,
with the tile geometry the query reports.  Every slab [group][s] is compared on its own; there is no activation, so no element is left out.

Bound, elementwise, from the arithmetic, untuned; u = 2^-24.
  Direct form: (n + kstride) u sum |g| |x|, the same sums over absolute values.  n = cells of the chunk, i.e. the products of an element
  that can be nonzero: the fp32 accumulation chain of the matrix pipe in any order, each product rounded once; kstride (that of the
  element's channel block, 1 on the 4-wave tile) for the additions of the LDS combine of the K-split partial tiles.
  Pair form (header comment of csrc/wgrad.hip): the cells are taken as (even, odd) column pairs of the image - tiles start at even columns,
  so this needs no tile geometry.  For the pair (g0, g1) and the inputs e0 .. e3 under it in tap row ky
      u = [g0, g0 + g1, g0 - g1, -g1]     t = [e0 - e2, e1 + e2, e2 - e1, e1 - e3]     m_c = sum over pairs u_c t_c
      dW[ky][0] = m0 + (m1 + m2) / 2      dW[ky][1] = (m1 - m2) / 2                    dW[ky][2] = (m1 + m2) / 2 + m3
  Each computed u_c, t_c carries one rounding, |fl(u_c)| <= (1 + u) |u_c|abs with the absolute values expanded through the pre-additions:
  |u|abs = [|g0|, |g0| + |g1|, |g0| + |g1|, |g1|], |t|abs = [|e0| + |e2|, |e1| + |e2|, |e2| + |e1|, |e1| + |e3|].  With
  A_c = sum over pairs |u_c|abs |t_c|abs and P pairs in the chunk (n / 2 accumulation steps), to first order |fl(m_c) - m_c| <= (P + 2) u A_c.
  The fold: hs = fl((m1 + m2) / 2) (the halving is exact), then one addition or subtraction per tap - at most three roundings on the way to
  any tap, each of a value bounded by the tap's own sum of A_c.  So
      tap 0: (P + 5) u (A_0 + (A_1 + A_2) / 2)     tap 1: (P + 5) u (A_1 + A_2) / 2     tap 2: (P + 5) u ((A_1 + A_2) / 2 + A_3)
max err / bound per entry and the worst per key are printed at the end of the module; MEASURED below is a copy of that report from the
MI355X, which nothing asserts.

Untouched memory: the slabs are a view inside a buffer prefilled with PATTERN, GUARD elements on either side (tests/fp64_check.py).  After the launch no slab
element holds the pattern (every element is written, the zeros of an empty chunk included: an empty chunk's slab is exactly 0) and both
guards still do.

Bitwise: a second run gives the same bits; the 4-bytes-off copy of a vec-eligible entry gives the bits of the aligned run (both staging
paths fill the same LDS image, the k-steps are the same); with NB = 1, sample b of the batch launch equals the launch of sample b alone
under the same S.  An S > 1 entry equals nothing bitwise but stays within the bound of its own chunks; the S = 1 entries of the same
shapes are in the table.
"""
import dataclasses

import pytest
import torch

import fp64_check
import wgrad_forms as wf
from transeditor_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RESULTS = []
IDS = lambda e: e.name

# worst max err / bound per key (kind, nwp, wino, vec, db); MI355X (a record, nothing asserts it)
MEASURED = {('1x1', 2, 0, 0, 0): 0.4959, ('1x1', 2, 0, 1, 0): 0.0537, ('1x1', 4, 0, 0, 0): 0.4934, ('1x1', 4, 0, 1, 0): 0.0612,
            ('3x3', 2, 0, 0, 0): 0.4989, ('3x3', 2, 0, 1, 0): 0.0777, ('3x3', 4, 0, 0, 1): 0.5510, ('3x3', 4, 1, 0, 1): 0.2878,
            ('3x3', 4, 1, 1, 1): 0.0413, ('t2', 2, 0, 0, 0): 0.4971, ('t2', 2, 0, 1, 0): 0.1343, ('t2', 4, 0, 0, 1): 0.5041,
            ('t2', 4, 0, 1, 1): 0.1605}


_report = fp64_check.report_fixture('max err / bound per entry (tests/test_gpu_wgrad_forms.py):', RESULTS, lambda name: wf.BY_NAME[name].key,
                                    'worst per key (kind, nwp, wino, vec, db):', widths=(56, 12))


def launch(e, g, x):
    """the entry's launch under its switch into a guarded buffer -> slabs [B / NB, S, Co, Ci, taps]"""
    shape = (e.B // e.NB, e.S, e.Co, e.Ci, 1 if e.kind == wf.K1 else 9)
    numel = 1
    for d in shape:
        numel *= d
    buf, inner = fp64_check.guarded(numel, DEV)
    out = inner.view(shape)
    assert (g.data_ptr() % 16, x.data_ptr() % 16) == (e.off, e.off), 'the operands have the alignment the table says'
    with wf.switch(e.sw):
        got = _lib.wgrad_slabs(g, x, wf.KIND[e.kind], e.H, e.W, S=e.S, NB=None if e.NB == 1 else e.NB, out=out)
    assert got.data_ptr() == out.data_ptr()
    fp64_check.untouched(e.name, 'the slabs', buf, numel, torch.ones(numel, dtype=torch.bool, device=DEV))         # every element is written
    return out


@pytest.mark.parametrize('entry', wf.TABLE, ids=IDS)
def test_form_against_fp64(entry):
    e = entry
    f = wf.check(e)
    with torch.no_grad():
        g, x = wf.operands(e, device=DEV)
        got = launch(e, g, x)
        ref, bound = wf.reference(e, f, g, x)
        assert got.shape == ref.shape == bound.shape
        for s, t in enumerate(e.trips):
            if t == 0:
                assert bool((got[:, s] == 0).all()), f'{e.name}: the slab of empty chunk {s} is not all zeros'
        fp64_check.within(e.name, 'slabs', got, ref, bound, results=RESULTS)
        again = launch(e, g, x)
    assert torch.equal(got, again), f'{e.name}: a second run gives other bits ({int((got != again).sum())} elements)'


OFF = [e for e in wf.TABLE if e.off]


@pytest.mark.parametrize('entry', OFF, ids=IDS)
def test_four_bytes_off_gives_the_aligned_bits(entry):
    """the scalar staging path against the 16-byte one: the aligned twin (switch off where the split kernel would take it) is asserted to
    run the same instantiation with vec on"""
    e = entry
    twin = dataclasses.replace(e, off=0, sw=0)
    f, ft = wf.check(e), wf.answer(twin)
    assert f['vec'] == 0 and ft['vec'] == 1 and ft['form6'] == 0
    assert all(f[k] == ft[k] for k in _lib.WGRAD_FORM if k not in ('vec', 'form6')), (f, ft)
    with torch.no_grad():
        got = launch(e, *wf.operands(e, device=DEV))
        want = launch(twin, *wf.operands(e, device=DEV, off=0))
    assert torch.equal(got, want), f'{e.name}: the 4-bytes-off launch differs from the aligned one in {int((got != want).sum())} elements'


PER_SAMPLE = [e for e in wf.TABLE if e.NB == 1 and e.B > 1 and e.name not in wf.LARGE]


@pytest.mark.parametrize('entry', PER_SAMPLE, ids=IDS)
def test_sample_of_a_batch_launch_equals_its_own_launch(entry):
    e = entry
    one = dataclasses.replace(e, B=1)
    f, f1 = wf.check(e), wf.answer(one)
    assert all(f[k] == f1[k] for k in _lib.WGRAD_FORM if k != 'grid_x') and f1['grid_x'] == e.S, (f, f1)
    with torch.no_grad():
        g, x = wf.operands(e, device=DEV)
        got = launch(e, g, x)
        for b in range(e.B):
            gb, xb = g[b:b + 1].clone(), x[b:b + 1].clone()         # (clones: 16-byte aligned, as the entries with B > 1 are)
            alone = launch(one, gb, xb)
            assert torch.equal(got[b:b + 1], alone), f'{e.name}: sample {b} of the batch launch differs from its own launch'

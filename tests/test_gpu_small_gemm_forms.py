"""Every form of the small dense kernel (tests/small_gemm_forms.py) against fp64, elementwise, called directly: _lib.small_gemm,
_lib.small_gemm_batched and _lib.small_gemm_splitk with the table's strides, so that no autograd wrapper chooses the layout.  Each test
re-asserts its entry's key (nw, av, bv) through te_small_gemm_form before it compares numbers.

Reference: fp64 torch on the same operands, taken through as_strided with the very strides handed to the kernel (small_gemm_forms.
reference).  Bound, elementwise, from the arithmetic, untuned; u = 2^-24, P = sum_k |A| |B| in fp64:
    pre      (K + NW + 1) u |alpha| P + u |beta bias| + u |ref|     K for the fp32 chain of a wave in any order, NW for the LDS combine, one
             each for the alpha product, the bias product and the final add
    act 3    times the slope and sqrt 2 at the element, + 2 u |out|;      residual: + u |out + res|
    split-K  Kc + NW per partial, S for the finish sum, then the epilogue terms: (Kc + NW + S + 1) u |alpha| P + ...
    row sums (K + 2 NW + 1) u |rs_scale| sum_k |A|
    GELU     with pre: c against the fp64 GELU of the kernel's own pre, 4 u |gelu| + 0.5 |pre| 17 u (three products and one add; erf
             to the 16 ulp of OpenCL's accuracy table, one more for the rounded argument since |t erf'(t)| < 0.5); without pre:
             1.13 (= sup |gelu'|) times the pre bound plus the same term
max err / bound per entry and the worst per form key are printed at the end of the module.  Measured on the MI355X, worst entry per
key (any entry point, any output): MEASURED below, copied from that report; the bound is not tuned to it.  By output: c 0.481, pre 0.482,
c against the GELU of the kernel's own pre 0.488, row sums 0.250, the last row sum of a ragged I 0.082; left out at most 8.2e-4.

Leaky-ReLU kink: elements whose fp64 pre-activation lies within its own bound of 0 are left out; at most KINK_CAP = 0.1 % of an entry (tests/fp64_check.py),
none of an entry with fewer than 1000 outputs (tests/test_small_gemm_forms_cpu.py holds the table to that on the CPU).

Untouched memory: c, pre, the row sums and the split-K workspace are views inside larger buffers prefilled with PATTERN; after the launch
every element outside the addressed set still holds it, the gaps that (zc, sci, scj) leave in the batched layouts included.

Bitwise: a second run gives the same bits; the 4-bytes-off copy of an operand gives the bits of the aligned one, and the transposed copy
of a K-edge entry the bits of the 16-byte one (the forms differ in their loads only; row sums too); row i (column j) of a launch equals
the one-row (one-column) launch of that row, and slice z of a batched launch the single launch of that slice, whenever the query gives
both the same key.  Two checks carry their name in the failure: the clamped-row check (the row sum of the last valid row of a ragged I, on
its own first: a padded row leaking into it) and the column-0 check (with J > 32 the row sums are those of a one-column-block launch).
"""
import dataclasses

import pytest
import torch

import fp64_check
import small_gemm_forms as sf
from fp64_check import U32 as U, guarded, untouched
from transeditor_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RESULTS = []
IDS = lambda e: e.name

# worst max err / bound per form key (nw, av, bv), any entry point, any output; MI355X (a record, nothing asserts it)
MEASURED = {(1, 0, 0): 0.4815, (1, 0, 1): 0.2947, (1, 1, 0): 0.2781, (1, 1, 1): 0.4233, (2, 0, 0): 0.1910, (2, 0, 1): 0.0489, (2, 1, 0): 0.1700,
            (2, 1, 1): 0.1952, (4, 0, 0): 0.1063, (4, 0, 1): 0.0178, (4, 1, 0): 0.1462, (4, 1, 1): 0.4878, (8, 0, 0): 0.0045, (8, 0, 1): 0.0038,
            (8, 1, 0): 0.1174, (8, 1, 1): 0.1323, (16, 0, 0): 0.1238, (16, 0, 1): 0.0014, (16, 1, 0): 0.0972, (16, 1, 1): 0.2320}


_report = fp64_check.report_fixture('max err / bound per entry (tests/test_gpu_small_gemm_forms.py):', RESULTS, lambda name: sf.BY_NAME[name].key,
                                    'worst per form key (nw, av, bv):', widths=(52, 34))


def _bases(e, o, g, a_shift=0, b_shift=0):
    a, b = o['a'][g.a_off + a_shift:], o['b'][g.b_off + b_shift:]
    return a, b, a.data_ptr() % 16, b.data_ptr() % 16


def launch(e, o, g=None):
    """the entry's launch into guarded buffers -> {'c': [nz, I, J], 'pre': ... | None, 'rs': [nz, I] | None}"""
    g = g or sf.geom(e)
    alpha, beta, rs = sf.scalars(e)
    a, b, am, bm = _bases(e, o, g)
    assert (am, bm) == (4 * g.a_off % 16, 4 * g.b_off % 16), 'the base pointers have the alignment the table says'
    I, J, K = e.I, e.J, e.K
    if e.ep in ('single', 'splitk'):
        cb, c = guarded(I * J, DEV)
        pb, pre = guarded(I * J, DEV) if e.pre else (None, None)
        out = {'rs': None}
        if e.ep == 'single':
            rb, rsv = guarded(I, DEV) if rs is not None else (None, None)
            _lib.small_gemm(I, J, K, a, g.sai, g.sak, b, g.sbk, g.sbj, o['bias'], o['res'], alpha, beta, e.act, want_pre=bool(e.pre), rowsum_scale=rs,
                            out=(c.view(I, J), pre.view(I, J) if e.pre else None, rsv))
            if rs is not None:
                untouched(e.name, 'row sums', rb, I, torch.ones(I, dtype=torch.bool, device=DEV))
                out['rs'] = rsv[None]
        else:
            wb, ws = guarded(e.nz * I * J, DEV)
            _lib.small_gemm_splitk(I, J, K, e.nz, a, g.sai, g.sak, b, g.sbk, g.sbj, o['bias'], o['res'], alpha, beta, e.act, want_pre=bool(e.pre),
                                   out=(c.view(I, J), pre.view(I, J) if e.pre else None, ws.view(e.nz, I, J)))
            untouched(e.name, 'workspace', wb, e.nz * I * J, torch.ones(e.nz * I * J, dtype=torch.bool, device=DEV))
        untouched(e.name, 'c', cb, I * J, torch.ones(I * J, dtype=torch.bool, device=DEV))
        if e.pre:
            untouched(e.name, 'pre', pb, I * J, torch.ones(I * J, dtype=torch.bool, device=DEV))
        out.update(c=c.view(1, I, J), pre=pre.view(1, I, J) if e.pre else None)
        return out
    cb, c = guarded(g.c_numel, DEV)
    tab = e.ep == 'table'
    _lib.small_gemm_batched(c, a, b, o['bias'], e.nz, g.za, g.zc, I, J, K, g.sai, g.sak, g.sbk, g.sbj, g.sci, g.scj, zb=g.zb, zbias=g.zbias,
                            b_tab=list(g.b_tab) if tab else None, bias_tab=list(g.bias_tab) if tab else None, alpha=alpha, beta=beta, act=e.act)
    view = (e.nz, I, J), (g.zc, g.sci, g.scj)
    addressed = torch.zeros(g.c_numel, dtype=torch.bool, device=DEV)
    addressed.as_strided(*view).fill_(True)
    assert int(addressed.sum()) == e.nz * I * J
    untouched(e.name, 'c', cb, g.c_numel, addressed)
    return {'c': c.as_strided(*view), 'pre': None, 'rs': None}


def _within(e, what, got, ref, bound, keep=None):
    fp64_check.within(e.name, what, got, ref, bound, keep, results=RESULTS)
    if keep is not None and keep.numel() < 1000:
        assert bool(keep.all()), f'{e.name} {what}: an entry of fewer than 1000 outputs leaves none out'


def _same_bits(e, what, x, y):
    for k in ('c', 'pre', 'rs'):
        assert (x[k] is None) == (y[k] is None)
        if x[k] is not None:
            assert torch.equal(x[k], y[k]), f'{e.name}: {what} gives other bits in {k} ({int((x[k] != y[k]).sum())} elements)'


@pytest.mark.parametrize('entry', sf.TABLE, ids=IDS)
def test_form_against_fp64(entry):
    e, g = entry, sf.geom(entry)
    nw = sf.check(e)[0]
    with torch.no_grad():
        o = sf.operands(e, device=DEV, g=g)
        got = launch(e, o, g)
        r = sf.reference(e, o, nw, g)
        if got['rs'] is not None:
            if e.I % 32:
                _within(e, 'clamped-row check: last row sum', got['rs'][:, -1:], r['rs'][:, -1:], r['rs_bound'][:, -1:])
            _within(e, 'row sums', got['rs'], r['rs'], r['rs_bound'])
        if e.pre:
            _within(e, 'pre', got['pre'], r['pre'], r['pre_bound'])
        if e.act == 1 and e.pre:
            own = got['pre'].double()
            ref, bound = sf.gelu64(own), sf.gelu_term(own)
            if o['res'] is not None:
                ref = ref + o['res'].double()
                bound = bound + U * ref.abs()
            _within(e, 'c from own pre', got['c'], ref, bound)
        else:
            _within(e, 'c', got['c'], r['out'], r['out_bound'], r['keep'])
        _same_bits(e, 'a second run', got, launch(e, o, g))


def _seed(e):
    return 2000 + sf.TABLE.index(e)


def _twin_bits(e, **change):
    """the entry against the same matrices in another layout, under the same wave count"""
    twin = dataclasses.replace(e, name=e.name, **change)
    ans, tans = sf.check(e), sf.answer(twin)
    assert tans[0] == ans[0] and tans[3:] == ans[3:], f'{e.name}: the twin has another wave count or grid'
    with torch.no_grad():
        got = launch(e, sf.operands(e, device=DEV))
        other = launch(twin, sf.operands(twin, seed=_seed(e), device=DEV))
    _same_bits(e, f'the copy with {change}', got, other)
    return ans, tans


@pytest.mark.parametrize('entry', [e for e in sf.TABLE if 'off4' in (e.la, e.lb)], ids=IDS)
def test_four_bytes_off_gives_the_aligned_bits(entry):
    ans, tans = _twin_bits(entry, la=entry.la.replace('off4', 'dense'), lb=entry.lb.replace('off4', 'dense'))
    if entry.K % 4 == 0:
        assert (tans[1], tans[2]) == (1, 1) and ans[1:3] == (int(entry.la != 'off4'), int(entry.lb != 'off4'))


@pytest.mark.parametrize('entry', [e for e in sf.TABLE if e.name.endswith('kedge') and e.key[1:] == (1, 1)], ids=IDS)
def test_scalar_loads_give_the_bits_of_the_16_byte_loads(entry):
    """float4 path plus scalar tail against the scalar form of the same matrices, at every K edge"""
    ans, tans = _twin_bits(entry, la='trans', lb='trans')
    assert ans[1:3] == (1, 1) and tans[1:3] == (0, 0)


SMALL_SINGLE = [e for e in sf.TABLE if e.ep == 'single' and e.name not in sf.LARGE]


@pytest.mark.parametrize('entry', SMALL_SINGLE, ids=IDS)
def test_one_row_and_one_column_launches_give_the_same_bits(entry):
    e, g = entry, sf.geom(entry)
    ans = sf.check(e)
    alpha, beta, rs = sf.scalars(e)
    with torch.no_grad():
        o = sf.operands(e, device=DEV, g=g)
        got = launch(e, o, g)
        for i in sorted({0, e.I - 1}):
            a, b, am, bm = _bases(e, o, g, a_shift=i * g.sai)
            if _lib.small_gemm_form(1, e.J, e.K, 1, g.sai, g.sak, g.sbk, g.sbj, a_mod16=am, b_mod16=bm)[:3] != ans[:3]:
                continue
            res = o['res'][i:i + 1].contiguous() if e.res else None
            c, pre, rsv = _lib.small_gemm(1, e.J, e.K, a, g.sai, g.sak, b, g.sbk, g.sbj, o['bias'], res, alpha, beta, e.act, want_pre=bool(e.pre), rowsum_scale=rs)
            one = {'c': c[None], 'pre': pre[None] if e.pre else None, 'rs': rsv[None] if rs is not None else None}
            row = {k: (v[:, i:i + 1] if v is not None else None) for k, v in got.items()}
            _same_bits(e, f'the one-row launch of row {i}', row, one)
        for j in sorted({0, e.J - 1}):
            a, b, am, bm = _bases(e, o, g, b_shift=j * g.sbj)
            if _lib.small_gemm_form(e.I, 1, e.K, 1, g.sai, g.sak, g.sbk, g.sbj, a_mod16=am, b_mod16=bm)[:3] != ans[:3]:
                continue
            res = o['res'][:, j:j + 1].contiguous() if e.res else None
            bias = o['bias'][j:j + 1].contiguous() if e.bias else None
            c, pre, rsv = _lib.small_gemm(e.I, 1, e.K, a, g.sai, g.sak, b, g.sbk, g.sbj, bias, res, alpha, beta, e.act, want_pre=bool(e.pre), rowsum_scale=rs)
            one = {'c': c[None], 'pre': pre[None] if e.pre else None, 'rs': rsv[None] if rs is not None else None}
            col = {'c': got['c'][:, :, j:j + 1], 'pre': got['pre'][:, :, j:j + 1] if e.pre else None, 'rs': got['rs']}
            _same_bits(e, f'the one-column launch of column {j}', col, one)


@pytest.mark.parametrize('entry', [e for e in sf.TABLE if e.ep in ('uniform', 'table')], ids=IDS)
def test_slice_of_a_batched_launch_equals_its_single_launch(entry):
    e, g = entry, sf.geom(entry)
    ans = sf.check(e)
    alpha, beta, _ = sf.scalars(e)
    with torch.no_grad():
        o = sf.operands(e, device=DEV, g=g)
        got = launch(e, o, g)
        for z in sorted({0, e.nz - 1}):
            a, b, am, bm = _bases(e, o, g, a_shift=z * g.za, b_shift=g.b_starts[z])
            if _lib.small_gemm_form(e.I, e.J, e.K, 1, g.sai, g.sak, g.sbk, g.sbj, a_mod16=am, b_mod16=bm)[:3] != ans[:3]:
                continue
            bias = o['bias'][g.bias_starts[z]:g.bias_starts[z] + e.J].contiguous() if e.bias else None
            c = _lib.small_gemm(e.I, e.J, e.K, a, g.sai, g.sak, b, g.sbk, g.sbj, bias, None, alpha, beta, e.act)[0]
            assert torch.equal(got['c'][z], c), f'{e.name}: slice {z} of the batched launch differs from its single launch'


@pytest.mark.parametrize('entry', [e for e in sf.TABLE if e.rs is not None and e.J > 32], ids=IDS)
def test_row_sums_come_from_column_block_0(entry):
    """column-0 check: with more than one column block the row sums are, bit for bit, those of the launch that has block column 0 only"""
    e = entry
    one = dataclasses.replace(e, J=min(e.J, 32))
    assert sf.answer(one)[0] == sf.check(e)[0] and sf.answer(one)[3] == 1 < sf.answer(e)[3]
    with torch.no_grad():
        got = launch(e, sf.operands(e, device=DEV))                      # (launch() has checked that every row sum was written, none outside)
        ref = launch(one, sf.operands(one, seed=_seed(e), device=DEV))     # the same A: the generator draws it first
    assert torch.equal(got['rs'], ref['rs']), f'{e.name}: column-0 check: the row sums of a {sf.answer(e)[3]}-column-block launch differ from block column 0 alone'

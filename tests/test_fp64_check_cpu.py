"""tests/fp64_check.py on the CPU: every way in which the shared elementwise check, the guard bands and the misaligned operand must fail
does fail, so that a later edit of the helper cannot quietly turn a GPU test's check off."""
import math

import pytest
import torch

import fp64_check as fc

CPU = 'cpu'


def _case(n=8):
    ref = torch.arange(n, dtype=torch.float64) / 4 - 1                      # dyadic values: adding a bound of 2^-20 is exact
    return ref, torch.full_like(ref, 2.0 ** -20)


def test_within_passes_at_the_bound_and_fails_one_ulp_above():
    ref, bound = _case()
    got = ref.clone()
    got[3] = ref[3] + bound[3]
    assert float((got - ref).abs()[3]) == float(bound[3])                   # err == bound exactly
    results = []
    assert fc.within('case', 'y', got, ref, bound, results=results) == (1.0, 0.0)
    assert results == [('case', 'y', 1.0, 0.0)]
    tight = bound.clone()
    tight[3] = math.nextafter(float(bound[3]), 0.0)                          # the error is now one ulp above its bound
    with pytest.raises(AssertionError, match='max err / bound'):
        fc.within('case', 'y', got, ref, tight)
    assert fc.within('case', 'y', got.float(), ref, bound)[0] <= 1.0        # (an fp32 result is compared in fp64)


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_within_fails_on_a_value_that_is_not_finite_even_where_keep_excludes_it(bad):
    ref, bound = _case()
    got = ref.clone()
    got[5] = bad
    with pytest.raises(AssertionError):
        fc.within('case', 'y', got, ref, bound)
    keep = torch.ones_like(ref, dtype=torch.bool)
    keep[5] = False
    with pytest.raises(AssertionError, match='not finite'):
        fc.within('case', 'y', got, ref, bound, keep, cap=1.0)
    got[5] = 1e3                                                            # finite and left out: only then does it pass
    assert fc.within('case', 'y', got, ref, bound, keep, cap=1.0) == (0.0, 1.0 - 7 / 8)


def test_within_caps_the_left_out_share():
    ref, bound = _case(100000)
    keep = torch.ones_like(ref, dtype=torch.bool)
    keep[:101] = False                                                      # 1.01e-3 of the elements: just above the default cap
    with pytest.raises(AssertionError, match='on the kink'):
        fc.within('case', 'y', ref, ref, bound, keep)
    keep[99:101] = True                                                     # 0.99e-3: just below
    assert fc.within('case', 'y', ref, ref, bound, keep)[1] == pytest.approx(9.9e-4)
    with pytest.raises(AssertionError, match='on the kink'):
        fc.within('case', 'y', ref, ref, bound, keep, cap=9.8e-4)           # an explicit cap holds in the same way
    assert fc.within('case', 'y', ref, ref, bound, keep, cap=0.01)[1] <= 1e-3


def test_within_holds_the_yardstick_to_the_bound_and_to_its_own_share():
    ref, bound = _case(4000)
    theirs = ref.clone()
    assert fc.within('case', 'y', ref, ref, bound, yardstick=(theirs, 0.0)) == (0.0, 0.0)
    theirs[7] += 2 * bound[7]                                               # only the yardstick breaks the bound
    with pytest.raises(AssertionError, match='torch in fp32 misses the bound'):
        fc.within('case', 'y', ref, ref, bound, yardstick=(theirs, 0.0))
    keep = torch.ones_like(ref, dtype=torch.bool)
    keep[7] = False                                                         # left out: both pass, 2.5e-4 of the elements are left out
    assert fc.within('case', 'y', ref, ref, bound, keep, yardstick=(theirs, 3e-4))[1] == pytest.approx(2.5e-4)
    with pytest.raises(AssertionError, match='the yardstick leaves out'):
        fc.within('case', 'y', ref, ref, bound, keep, yardstick=(theirs, 2e-4))            # under the cap, above the yardstick's own


def test_within_at_a_bound_of_zero():
    ref, bound = _case()
    assert float(ref[4]) == 0.0
    bound[4] = 0.0
    assert fc.within('case', 'y', ref, ref, bound) == (0.0, 0.0)
    got = ref.clone()
    got[4] += 2.0 ** -60
    with pytest.raises(AssertionError, match='max err / bound'):
        fc.within('case', 'y', got, ref, bound)


def test_kink_keep_and_where64():
    pre = torch.tensor([-1.0, -1e-9, 0.0, 1e-9, 1.0], dtype=torch.float64)
    keep = fc.kink_keep(pre, torch.full_like(pre, 1e-9))
    assert keep.tolist() == [True, False, False, False, True]
    g = fc.where64(pre > 0, fc.S32, fc.AS32)
    assert g.dtype == torch.float64 and g.tolist() == [fc.AS32] * 3 + [fc.S32] * 2
    assert fc.U32 == 2.0 ** -24 and fc.A32 != fc.ALPHA and fc.AS32 != fc.A32 * fc.S32       # the constants as fp32 has them


def test_untouched_sees_a_write_in_either_guard():
    buf, inner = fc.guarded(10, CPU)
    assert buf.numel() == 10 + 2 * fc.GUARD and inner.data_ptr() == buf.data_ptr() + 4 * fc.GUARD and bool((buf == fc.PATTERN).all())
    inner.fill_(1.0)
    everything = torch.ones(10, dtype=torch.bool)
    fc.untouched('case', 'c', buf, 10)
    fc.untouched('case', 'c', buf, 10, everything)
    for at in (0, fc.GUARD - 1, fc.GUARD + 10, buf.numel() - 1):
        dirty = buf.clone()
        dirty[at] = 0.0
        with pytest.raises(AssertionError, match='outside its buffer'):
            fc.untouched('case', 'c', dirty, 10, everything)
        with pytest.raises(AssertionError, match='outside its buffer'):
            fc.untouched('case', 'c', dirty, 10)


def test_untouched_sees_a_write_between_and_a_miss_among_the_addressed_elements():
    buf, inner = fc.guarded(10, CPU)
    addressed = torch.zeros(10, dtype=torch.bool)
    addressed[::2] = True
    inner[::2] = 1.0
    fc.untouched('case', 'c', buf, 10, addressed)
    inner[3] = 1.0                                                          # a gap of the layout
    with pytest.raises(AssertionError, match='between the addressed elements'):
        fc.untouched('case', 'c', buf, 10, addressed)
    inner[3] = fc.PATTERN
    inner[4] = fc.PATTERN                                                   # an addressed element that nothing wrote
    with pytest.raises(AssertionError, match='1 addressed elements that were not written'):
        fc.untouched('case', 'c', buf, 10, addressed)


def test_off16_places_the_same_values_at_both_offsets():
    v = torch.randn(3, 5, 7, generator=torch.Generator().manual_seed(1))
    a, b = fc.off16(v, 0, CPU), fc.off16(v, 4, CPU)
    assert (a.data_ptr() % 16, b.data_ptr() % 16) == (0, 4)
    assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape == v.shape
    assert torch.equal(a, v) and torch.equal(b, v)
    with pytest.raises(AssertionError):
        fc.off16(v, 6, CPU)                                                 # not a whole element


def test_report_prints_the_table_and_the_worst_per_key(capsys):
    results = [('a1', 'y', 0.25, 0.0), ('b1', 'dx', 0.5, 1e-4), ('a2', 'y', 0.125, 0.0)]
    fc.print_report('title:', results, key_of=lambda name: name[0], key_title='worst per key:', widths=(4, 3))
    assert capsys.readouterr().out == ('\ntitle:\n  a1   y     0.2500   left out 0.0e+00\n  b1   dx    0.5000   left out 1.0e-04\n'
                                       '  a2   y     0.1250   left out 0.0e+00\nworst per key:\n  a: 0.2500\n  b: 0.5000\n')
    fc.print_report('title:', results[:1])
    assert capsys.readouterr().out == '\ntitle:\n  a1                     y                    0.2500   left out 0.0e+00\n'

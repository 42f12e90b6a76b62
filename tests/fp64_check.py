"""What the GPU tests share when they hold a kernel to an fp64 reference: the round-off constants, the elementwise check with its
kink cap, the guard bands around an output, the operand placed off 16-byte alignment and the end-of-module report.  A new GPU test takes
these from here; no test module imports another one for a helper.  Importable without a GPU and without the library;
tests/test_fp64_check_cpu.py pins the behaviour of every check below.

The elementwise check: |got - ref| <= bound wherever `keep`, bound worked out from the arithmetic by the caller.  Under an activation
with a kink at 0 the elements whose fp64 pre-activation lies within its own bound of 0 are left out (kink_keep: the kernel may
legitimately take the other slope there), and the left-out share of a case is capped, by KINK_CAP = 0.1 % unless the caller says otherwise.
"""
import numpy as np
import pytest
import torch

U = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.float64: 2.0 ** -53}          # unit round-off per number format
U32 = U[torch.float32]
ALPHA, SCALE = 0.2, 2 ** 0.5
A32, S32 = float(np.float32(ALPHA)), float(np.float32(SCALE))            # the constants as the fp32 kernels receive them
AS32 = float(np.float32(ALPHA) * np.float32(SCALE))                      # alpha * scale, formed in fp32 by the FIR kernels
KINK_CAP = 1e-3
SENTINEL = -777.25                                                       # prefill of an output that a refused call must leave alone
GUARD = 256                                                              # elements of PATTERN on either side of a guarded output
PATTERN = -12345.5


def within(name, what, got, ref, bound, keep=None, *, cap=KINK_CAP, results=None, yardstick=None):
    """assert |got - ref| <= bound elementwise (where `keep`) for output `what` of case `name`, after printing max err / bound and the
    left-out share and recording them as (name, what, worst, left) in `results`, the list behind a module's report.  got must be
    finite everywhere, the left-out share at most `cap`.  yardstick = (tensor, share_cap): torch's own fp32 result must meet the same
    bound on the same elements, with at most share_cap left out.  got and the yardstick may live on another device than ref; the
    comparison runs where ref is.  Returns (worst, left)."""
    err = (got.double().to(ref.device) - ref).abs()
    floor = bound.clamp_min(1e-300)
    ratio = err / floor
    left = 0.0
    if keep is not None:
        left = 1.0 - float(keep.double().mean())
        ratio = torch.where(keep, ratio, torch.zeros_like(ratio))
    worst = float(ratio.max())
    if results is not None:
        results.append((name, what, worst, left))
    line = f'{name} {what}: max err / bound {worst:.4f}, left out {left:.1e}'
    if yardstick is not None:
        theirs, share_cap = yardstick
        yard = (theirs.double().to(ref.device) - ref).abs() / floor
        theirs_worst = float((yard if keep is None else torch.where(keep, yard, torch.zeros_like(yard))).max())
        line += f' (torch fp32 on the CPU {theirs_worst:.4f})'
    print(line)
    assert torch.isfinite(got).all(), f'{name} {what}: the output is not finite'
    assert left <= cap, f'{name} {what}: {left:.2e} of the elements sit on the kink'
    assert worst <= 1.0, f'{name} {what}: max err / bound {worst:.3f}'
    if yardstick is not None:
        assert left <= share_cap, f'{name} {what}: the yardstick leaves out {left:.2e} of the elements'
        assert theirs_worst <= 1.0, f'{name} {what}: torch in fp32 misses the bound itself, max err / bound {theirs_worst:.3f}'
    return worst, left


def kink_keep(pre, bound):
    """the elements off the kink by more than the pre-activation's own bound"""
    return pre.abs() > bound


def where64(mask, a, b):
    return torch.where(mask, torch.tensor(a, dtype=torch.float64, device=mask.device), torch.tensor(b, dtype=torch.float64, device=mask.device))


def guarded(numel, device):
    """(buf, inner): numel elements with GUARD elements on either side, all prefilled with PATTERN"""
    buf = torch.full((GUARD + numel + GUARD,), PATTERN, device=device)
    return buf, buf[GUARD:GUARD + numel]


def untouched(name, what, buf, numel, addressed=None):
    """everything of buf outside the addressed set still holds the pattern, and every addressed element was written (addressed: bool
    mask over the numel inner elements; None: only the guards are looked at)"""
    assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + numel:] == PATTERN).all()), f'{name}: {what} written outside its buffer'
    if addressed is not None:
        inner = buf[GUARD:GUARD + numel]
        assert bool((inner[~addressed] == PATTERN).all()), f'{name}: {what} written between the addressed elements'
        missed = int((inner[addressed] == PATTERN).sum())
        assert missed == 0, f'{name}: {what} has {missed} addressed elements that were not written'


def off16(values, off_bytes, device):
    """the same values as a contiguous tensor on `device` that begins off_bytes past a 16-byte boundary"""
    size = values.element_size()
    assert 0 <= off_bytes < 16 and off_bytes % size == 0
    buf = torch.zeros(values.numel() + 16 // size, dtype=values.dtype, device=device)
    t = buf[off_bytes // size:off_bytes // size + values.numel()].view(values.shape)
    t.copy_(values)
    assert t.is_contiguous() and t.data_ptr() % 16 == off_bytes
    return t


def print_report(title, results, key_of=None, key_title=None, widths=(22, 18)):
    """`results` as a table under `title`; with key_of (case name -> key) also the worst ratio per key, under key_title"""
    print('\n' + title)
    worst = {}
    for name, what, ratio, left in results:
        print(f'  {name:{widths[0]}s} {what:{widths[1]}s} {ratio:8.4f}   left out {left:.1e}')
        if key_of is not None:
            worst[key_of(name)] = max(worst.get(key_of(name), 0.0), ratio)
    if key_of is not None:
        print(key_title)
        for k in sorted(worst):
            print(f'  {k}: {worst[k]:.4f}')


def report_fixture(title, results, key_of=None, key_title=None, *, widths=(22, 18)):
    """a module-scoped autouse fixture that prints the table of print_report after the module's tests; widths: those of the name and
    the output column.  Bind it to a module attribute: _report = report_fixture(...)."""
    @pytest.fixture(scope='module', autouse=True)
    def _report():
        yield
        print_report(title, results, key_of, key_title, widths)
    return _report

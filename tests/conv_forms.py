"""Form table of the fp32 direct convolution kernel: the smallest shapes that land on every form of
conv_mfma_kernel<KIND, TC, HAS_ISC, MS, OCC, FAST, EPI> (csrc/conv.hip) and of its host-side launch geometry.

One route of tests/conv_routes.py (FWD/3X3, FWD/S2, FWD/T2, FWD/1X1 and their data-gradient packs) is about a hundred instantiations
and a dozen geometry rules below the selectors: tile class, FAST or general staging, multi-sample tiles, split-K, the T2 regions, the
banded block-to-tile mapping.  Which of them a launch takes is decided by launch constants; te_conv_form (include/te_hip.h) reports
the plan that te_conv_res_f32 itself makes and then launches.  An entry names a kind, a shape (B, K, M, H, W - H, W the low-resolution
size), the operands that matter to the form (style scales, residual / mask epilogue, workspace), an activation, and the form it is
expected to land on.  The expected form is data; what a launch does comes from the query, never from constants restated here.
tests/test_conv_forms_cpu.py checks the table against the query and sweeps the query for forms the table lacks;
tests/test_gpu_conv_forms.py runs every entry against fp64 after re-asserting its form.

The form of an entry is the tuple FORM_FIELDS:
    tc        tile class that launches (0, 1, 2; 3 = the deep-stage 1x1)          fast      the FAST kernel
    ms        the kernel's multi-sample template flag                              multi     a tile holds several samples (run-time fact)
    occ       waves per SIMD the kernel is compiled for                            split     ksplit > 1
    nreg      cell regions (3: T2 body + last column + last row)                   nsv_cut   region 0 stages fewer samples than its tile holds
    th_cut    the staging budget halved the tile rows of region 0
and its form KEY is (kind, has_isc, epi given) + that tuple.  The list of keys with their entries: `python tests/conv_forms.py`.
An entry's name spells its key: kind_tcN_{fast|gen}[_multi][_isc][_epi][_split][_r3][_nsv][_th], then a tag for what else it is about.

K is as small as the form allows: 16 for FAST (64 for the deep-stage class), 12 where the general form comes from K % KC != 0, 24 where
it comes from K != Kp, 56 / 120 for a ragged K that still splits, 64 / 128 for a FAST split.  What the query showed while the table was
written, and the table therefore says differently from a first guess:
* W = 3 gives TW = 4 (the tile width is the next power of two), so it is FAST-capable; at small heights its tile holds two samples,
  which is what makes it general.  TW < 4 needs W <= 2: the `w2` entries.
* The staging budget halves the tile rows of region 0 in the FAST form only (every general tile of region 0 fits the budget of its
  kind).  In the general form it halves the rows of T2's last-column region (TW = 1, 128 rows wanted): `edgeth`, and the large entries.
* The deep-stage class 3 does fall back to class 0: the plan promotes on the first guess of the tile (one sample, no split, K % 64 == 0)
  and a 2-column image then has TW < 4, which FAST refuses: `tc3_fallback` (2 x 64 x 8192 x 2).
* T2 at class 0 is never split and never multi-sample: class 0 needs more than T2_TC1_LIMIT cells, which fill the chip.
The four class-0 T2 entries (FAST / general, with / without style scales) are the large ones: 2 x 96 x 385 x 385 outputs, no activation.
"""
import os
import sys
from dataclasses import dataclass, field

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from transeditor_amd import _lib  # noqa: E402

FORM_FIELDS = ('tc', 'fast', 'ms', 'multi', 'occ', 'split', 'nreg', 'nsv_cut', 'th_cut')
KINDS = {'3X3': _lib.CONV_3X3, 'T2': _lib.CONV_T2, 'S2': _lib.CONV_S2, '1X1': _lib.CONV_1X1}
EPIS = ('none', 'res', 'mask', 'both')


@dataclass(frozen=True)
class Form:
    name: str
    kind: str        # '3X3', 'T2', 'S2', '1X1'
    shape: tuple     # (B, K, M, H, W)
    has_isc: int
    epi: str         # 'none', 'res', 'mask', 'both'
    act: int         # 0 linear, 3 lrelu * sqrt(2), 4 lrelu
    with_ws: int     # 1: the split-K workspace is handed over whenever the plan splits (te_conv_ws_f32), 0: never (te_conv_f32)
    form: tuple      # FORM_FIELDS
    expect: dict = field(default_factory=dict)      # further answers of the query this entry is about (see answer_fields)

    def __hash__(self):
        return hash(self.name)


def form_name(kind, has_isc, epi, form):
    tc, fast, ms, multi, occ, split, nreg, nsv, th = form
    return f'{kind.lower()}_tc{tc}_' + ('fast' if fast else 'gen') + ('_multi' if multi else '') + ('_isc' if has_isc else '') \
        + ('_epi' if epi != 'none' else '') + ('_split' if split else '') + ('_r3' if nreg == 3 else '') + ('_nsv' if nsv else '') + ('_th' if th else '')


def E(kind, shape, has_isc, epi, act, with_ws, form, tag='', **expect):
    return Form(form_name(kind, has_isc, epi, form) + ('_' + tag if tag else ''), kind, shape, has_isc, epi, act, with_ws, form, expect)


# ---- one entry per form key: the smallest shape of a sweep of the query that lands on it
PER_KEY = [
    E('1X1', (2, 12, 96, 9, 5), 0, 'none', 3, 1, (0, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 96, 9, 5), 0, 'none', 4, 1, (0, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 96, 9, 5), 0, 'both', 0, 1, (0, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 96, 9, 5), 0, 'res', 3, 1, (0, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 96, 9, 5), 1, 'none', 4, 1, (0, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 96, 9, 5), 1, 'none', 0, 1, (0, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 96, 1, 1), 0, 'none', 3, 1, (0, 0, 0, 1, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 96, 1, 1), 0, 'none', 4, 1, (0, 0, 0, 1, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 96, 1, 1), 0, 'both', 0, 1, (0, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 96, 1, 1), 0, 'res', 3, 1, (0, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 96, 1, 1), 1, 'none', 4, 1, (0, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 96, 1, 1), 1, 'none', 0, 1, (0, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 48, 9, 9), 0, 'none', 3, 1, (1, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 48, 9, 9), 0, 'none', 4, 1, (1, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 48, 9, 9), 0, 'both', 0, 1, (1, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 48, 9, 9), 0, 'res', 3, 1, (1, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 48, 9, 9), 1, 'none', 4, 1, (1, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 48, 9, 9), 1, 'none', 0, 1, (1, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 48, 1, 1), 0, 'none', 3, 1, (1, 0, 0, 1, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 48, 1, 1), 0, 'none', 4, 1, (1, 0, 0, 1, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 48, 1, 1), 0, 'both', 0, 1, (1, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 48, 1, 1), 0, 'res', 3, 1, (1, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 48, 1, 1), 1, 'none', 4, 1, (1, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 48, 1, 1), 1, 'none', 0, 1, (1, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 8, 9, 9), 0, 'none', 3, 1, (2, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 8, 9, 9), 0, 'none', 4, 1, (2, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 8, 9, 9), 0, 'both', 0, 1, (2, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 8, 9, 9), 0, 'res', 3, 1, (2, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 8, 9, 9), 1, 'none', 4, 1, (2, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 8, 9, 9), 1, 'none', 0, 1, (2, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 8, 1, 1), 0, 'none', 3, 1, (2, 0, 0, 1, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 8, 1, 1), 0, 'none', 4, 1, (2, 0, 0, 1, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 8, 1, 1), 0, 'both', 0, 1, (2, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 8, 1, 1), 0, 'res', 3, 1, (2, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('1X1', (2, 12, 8, 1, 1), 1, 'none', 4, 1, (2, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('1X1', (2, 56, 8, 1, 1), 1, 'none', 0, 1, (2, 0, 1, 1, 2, 1, 1, 0, 0)),
    # the deep-stage class: 256 tiles fill the chip, so the plan does not split
    E('1X1', (2, 64, 128, 128, 128), 0, 'none', 3, 1, (3, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 64, 128, 128, 128), 0, 'res', 4, 1, (3, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('1X1', (2, 64, 128, 128, 128), 1, 'none', 0, 1, (3, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 96, 9, 5), 0, 'none', 3, 1, (0, 0, 0, 0, 3, 0, 1, 0, 0)),
    E('3X3', (2, 56, 96, 9, 5), 0, 'none', 4, 1, (0, 0, 0, 0, 3, 1, 1, 0, 0)),
    E('3X3', (2, 12, 96, 9, 5), 0, 'both', 0, 1, (0, 0, 0, 0, 3, 0, 1, 0, 0)),
    E('3X3', (2, 56, 96, 9, 5), 0, 'res', 3, 1, (0, 0, 0, 0, 3, 1, 1, 0, 0)),
    E('3X3', (2, 12, 96, 9, 5), 1, 'none', 4, 1, (0, 0, 0, 0, 3, 0, 1, 0, 0)),
    E('3X3', (2, 56, 96, 9, 5), 1, 'none', 0, 1, (0, 0, 0, 0, 3, 1, 1, 0, 0)),
    E('3X3', (2, 12, 96, 2, 2), 0, 'none', 3, 1, (0, 0, 0, 1, 3, 0, 1, 0, 0)),
    E('3X3', (2, 12, 96, 1, 1), 0, 'none', 4, 1, (0, 0, 0, 1, 3, 0, 1, 1, 0)),
    E('3X3', (2, 56, 96, 2, 2), 0, 'none', 0, 1, (0, 0, 0, 1, 3, 1, 1, 0, 0)),
    E('3X3', (2, 56, 96, 1, 1), 0, 'none', 3, 1, (0, 0, 0, 1, 3, 1, 1, 1, 0)),
    E('3X3', (2, 12, 96, 2, 2), 0, 'mask', 4, 1, (0, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 96, 1, 1), 0, 'both', 0, 1, (0, 0, 1, 1, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 96, 2, 2), 0, 'res', 3, 1, (0, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 96, 1, 1), 0, 'mask', 4, 1, (0, 0, 1, 1, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 96, 2, 2), 1, 'none', 0, 1, (0, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 96, 1, 1), 1, 'none', 3, 1, (0, 0, 1, 1, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 96, 2, 2), 1, 'none', 4, 1, (0, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 96, 1, 1), 1, 'none', 0, 1, (0, 0, 1, 1, 2, 1, 1, 1, 0)),
    E('3X3', (2, 16, 96, 3, 17), 0, 'none', 3, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0)),
    E('3X3', (2, 16, 96, 9, 5), 0, 'none', 4, 1, (0, 1, 0, 0, 3, 0, 1, 1, 1)),
    E('3X3', (2, 64, 96, 3, 17), 0, 'none', 0, 1, (0, 1, 0, 0, 3, 1, 1, 0, 0)),
    E('3X3', (2, 64, 96, 9, 5), 0, 'none', 3, 1, (0, 1, 0, 0, 3, 1, 1, 1, 1)),
    E('3X3', (2, 16, 96, 3, 17), 0, 'mask', 4, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0)),
    E('3X3', (2, 16, 96, 9, 5), 0, 'both', 0, 1, (0, 1, 0, 0, 3, 0, 1, 1, 1)),
    E('3X3', (2, 64, 96, 3, 17), 0, 'res', 3, 1, (0, 1, 0, 0, 3, 1, 1, 0, 0)),
    E('3X3', (2, 64, 96, 9, 5), 0, 'mask', 4, 1, (0, 1, 0, 0, 3, 1, 1, 1, 1)),
    E('3X3', (2, 16, 96, 3, 17), 1, 'none', 0, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0)),
    E('3X3', (2, 16, 96, 9, 5), 1, 'none', 3, 1, (0, 1, 0, 0, 3, 0, 1, 1, 1)),
    E('3X3', (2, 64, 96, 3, 17), 1, 'none', 4, 1, (0, 1, 0, 0, 3, 1, 1, 0, 0)),
    E('3X3', (2, 64, 96, 9, 5), 1, 'none', 0, 1, (0, 1, 0, 0, 3, 1, 1, 1, 1)),
    E('3X3', (2, 12, 48, 9, 9), 0, 'none', 3, 1, (1, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 48, 33, 2), 0, 'none', 4, 1, (1, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 48, 9, 9), 0, 'none', 0, 1, (1, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 48, 33, 2), 0, 'none', 3, 1, (1, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 48, 9, 9), 0, 'mask', 4, 1, (1, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 48, 33, 2), 0, 'both', 0, 1, (1, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 48, 9, 9), 0, 'res', 3, 1, (1, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 48, 33, 2), 0, 'mask', 4, 1, (1, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 48, 9, 9), 1, 'none', 0, 1, (1, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 48, 33, 2), 1, 'none', 3, 1, (1, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 48, 9, 9), 1, 'none', 4, 1, (1, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 48, 33, 2), 1, 'none', 0, 1, (1, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 48, 3, 5), 0, 'none', 3, 1, (1, 0, 0, 1, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 48, 1, 1), 0, 'none', 4, 1, (1, 0, 0, 1, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 48, 3, 5), 0, 'none', 0, 1, (1, 0, 0, 1, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 48, 1, 1), 0, 'none', 3, 1, (1, 0, 0, 1, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 48, 3, 5), 0, 'mask', 4, 1, (1, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 48, 1, 1), 0, 'both', 0, 1, (1, 0, 1, 1, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 48, 3, 5), 0, 'res', 3, 1, (1, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 48, 1, 1), 0, 'mask', 4, 1, (1, 0, 1, 1, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 48, 3, 5), 1, 'none', 0, 1, (1, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 48, 1, 1), 1, 'none', 3, 1, (1, 0, 1, 1, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 48, 3, 5), 1, 'none', 4, 1, (1, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 48, 1, 1), 1, 'none', 0, 1, (1, 0, 1, 1, 2, 1, 1, 1, 0)),
    E('3X3', (2, 16, 48, 9, 9), 0, 'none', 3, 1, (1, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 16, 48, 17, 5), 0, 'none', 4, 1, (1, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('3X3', (2, 64, 48, 9, 9), 0, 'none', 0, 1, (1, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 64, 48, 17, 5), 0, 'none', 3, 1, (1, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('3X3', (2, 16, 48, 9, 9), 0, 'mask', 4, 1, (1, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 16, 48, 17, 5), 0, 'both', 0, 1, (1, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('3X3', (2, 64, 48, 9, 9), 0, 'res', 3, 1, (1, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 64, 48, 17, 5), 0, 'mask', 4, 1, (1, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('3X3', (2, 16, 48, 9, 9), 1, 'none', 0, 1, (1, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 16, 48, 17, 5), 1, 'none', 3, 1, (1, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('3X3', (2, 64, 48, 9, 9), 1, 'none', 4, 1, (1, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 64, 48, 17, 5), 1, 'none', 0, 1, (1, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('3X3', (2, 12, 8, 9, 9), 0, 'none', 3, 1, (2, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 8, 33, 2), 0, 'none', 4, 1, (2, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 8, 9, 9), 0, 'none', 0, 1, (2, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 8, 33, 2), 0, 'none', 3, 1, (2, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 8, 9, 9), 0, 'mask', 4, 1, (2, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 8, 33, 2), 0, 'both', 0, 1, (2, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 8, 9, 9), 0, 'res', 3, 1, (2, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 8, 33, 2), 0, 'mask', 4, 1, (2, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 8, 9, 9), 1, 'none', 0, 1, (2, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 8, 33, 2), 1, 'none', 3, 1, (2, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 8, 9, 9), 1, 'none', 4, 1, (2, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 8, 33, 2), 1, 'none', 0, 1, (2, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 8, 3, 5), 0, 'none', 3, 1, (2, 0, 0, 1, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 8, 1, 1), 0, 'none', 4, 1, (2, 0, 0, 1, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 8, 3, 5), 0, 'none', 0, 1, (2, 0, 0, 1, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 8, 1, 1), 0, 'none', 3, 1, (2, 0, 0, 1, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 8, 3, 5), 0, 'mask', 4, 1, (2, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 8, 1, 1), 0, 'both', 0, 1, (2, 0, 1, 1, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 8, 3, 5), 0, 'res', 3, 1, (2, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 8, 1, 1), 0, 'mask', 4, 1, (2, 0, 1, 1, 2, 1, 1, 1, 0)),
    E('3X3', (2, 12, 8, 3, 5), 1, 'none', 0, 1, (2, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('3X3', (2, 12, 8, 1, 1), 1, 'none', 3, 1, (2, 0, 1, 1, 2, 0, 1, 1, 0)),
    E('3X3', (2, 56, 8, 3, 5), 1, 'none', 4, 1, (2, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('3X3', (2, 56, 8, 1, 1), 1, 'none', 0, 1, (2, 0, 1, 1, 2, 1, 1, 1, 0)),
    E('3X3', (2, 16, 8, 9, 9), 0, 'none', 3, 1, (2, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 16, 8, 17, 5), 0, 'none', 4, 1, (2, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('3X3', (2, 64, 8, 9, 9), 0, 'none', 0, 1, (2, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 64, 8, 17, 5), 0, 'none', 3, 1, (2, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('3X3', (2, 16, 8, 9, 9), 0, 'mask', 4, 1, (2, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 16, 8, 17, 5), 0, 'both', 0, 1, (2, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('3X3', (2, 64, 8, 9, 9), 0, 'res', 3, 1, (2, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 64, 8, 17, 5), 0, 'mask', 4, 1, (2, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('3X3', (2, 16, 8, 9, 9), 1, 'none', 0, 1, (2, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('3X3', (2, 16, 8, 17, 5), 1, 'none', 3, 1, (2, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('3X3', (2, 64, 8, 9, 9), 1, 'none', 4, 1, (2, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('3X3', (2, 64, 8, 17, 5), 1, 'none', 0, 1, (2, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('S2', (2, 12, 96, 9, 5), 0, 'none', 3, 1, (0, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 96, 33, 1), 0, 'none', 4, 1, (0, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 96, 9, 5), 0, 'none', 0, 1, (0, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 96, 33, 1), 0, 'none', 3, 1, (0, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('S2', (2, 12, 96, 9, 5), 1, 'none', 4, 1, (0, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 96, 33, 1), 1, 'none', 0, 1, (0, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 96, 9, 5), 1, 'none', 3, 1, (0, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 96, 33, 1), 1, 'none', 4, 1, (0, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('S2', (2, 12, 96, 2, 3), 0, 'none', 0, 1, (0, 0, 0, 1, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 96, 1, 1), 0, 'none', 3, 1, (0, 0, 0, 1, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 96, 2, 3), 0, 'none', 4, 1, (0, 0, 0, 1, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 96, 1, 1), 0, 'none', 0, 1, (0, 0, 0, 1, 2, 1, 1, 1, 0)),
    E('S2', (2, 12, 96, 2, 3), 1, 'none', 3, 1, (0, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 96, 1, 1), 1, 'none', 4, 1, (0, 0, 1, 1, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 96, 2, 3), 1, 'none', 0, 1, (0, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 96, 1, 1), 1, 'none', 3, 1, (0, 0, 1, 1, 2, 1, 1, 1, 0)),
    E('S2', (2, 16, 96, 3, 17), 0, 'none', 4, 1, (0, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 16, 96, 9, 5), 0, 'none', 0, 1, (0, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('S2', (2, 64, 96, 3, 17), 0, 'none', 3, 1, (0, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 64, 96, 9, 5), 0, 'none', 4, 1, (0, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('S2', (2, 16, 96, 3, 17), 1, 'none', 0, 1, (0, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 16, 96, 9, 5), 1, 'none', 3, 1, (0, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('S2', (2, 64, 96, 3, 17), 1, 'none', 4, 1, (0, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 64, 96, 9, 5), 1, 'none', 0, 1, (0, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('S2', (2, 12, 48, 9, 5), 0, 'none', 3, 1, (1, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 48, 33, 1), 0, 'none', 4, 1, (1, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 48, 9, 5), 0, 'none', 0, 1, (1, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 48, 33, 1), 0, 'none', 3, 1, (1, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('S2', (2, 12, 48, 9, 5), 1, 'none', 4, 1, (1, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 48, 33, 1), 1, 'none', 0, 1, (1, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 48, 9, 5), 1, 'none', 3, 1, (1, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 48, 33, 1), 1, 'none', 4, 1, (1, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('S2', (2, 12, 48, 2, 3), 0, 'none', 0, 1, (1, 0, 0, 1, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 48, 1, 1), 0, 'none', 3, 1, (1, 0, 0, 1, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 48, 2, 3), 0, 'none', 4, 1, (1, 0, 0, 1, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 48, 1, 1), 0, 'none', 0, 1, (1, 0, 0, 1, 2, 1, 1, 1, 0)),
    E('S2', (2, 12, 48, 2, 3), 1, 'none', 3, 1, (1, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 48, 1, 1), 1, 'none', 4, 1, (1, 0, 1, 1, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 48, 2, 3), 1, 'none', 0, 1, (1, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 48, 1, 1), 1, 'none', 3, 1, (1, 0, 1, 1, 2, 1, 1, 1, 0)),
    E('S2', (2, 16, 48, 3, 17), 0, 'none', 4, 1, (1, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 16, 48, 9, 5), 0, 'none', 0, 1, (1, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('S2', (2, 64, 48, 3, 17), 0, 'none', 3, 1, (1, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 64, 48, 9, 5), 0, 'none', 4, 1, (1, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('S2', (2, 16, 48, 3, 17), 1, 'none', 0, 1, (1, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 16, 48, 9, 5), 1, 'none', 3, 1, (1, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('S2', (2, 64, 48, 3, 17), 1, 'none', 4, 1, (1, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 64, 48, 9, 5), 1, 'none', 0, 1, (1, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('S2', (2, 12, 8, 9, 9), 0, 'none', 3, 1, (2, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 8, 33, 2), 0, 'none', 4, 1, (2, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 8, 9, 9), 0, 'none', 0, 1, (2, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 8, 33, 2), 0, 'none', 3, 1, (2, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('S2', (2, 12, 8, 9, 9), 1, 'none', 4, 1, (2, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 8, 33, 2), 1, 'none', 0, 1, (2, 0, 0, 0, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 8, 9, 9), 1, 'none', 3, 1, (2, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 8, 33, 2), 1, 'none', 4, 1, (2, 0, 0, 0, 2, 1, 1, 1, 0)),
    E('S2', (2, 12, 8, 3, 5), 0, 'none', 0, 1, (2, 0, 0, 1, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 8, 1, 1), 0, 'none', 3, 1, (2, 0, 0, 1, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 8, 3, 5), 0, 'none', 4, 1, (2, 0, 0, 1, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 8, 1, 1), 0, 'none', 0, 1, (2, 0, 0, 1, 2, 1, 1, 1, 0)),
    E('S2', (2, 12, 8, 3, 5), 1, 'none', 3, 1, (2, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('S2', (2, 12, 8, 1, 1), 1, 'none', 4, 1, (2, 0, 1, 1, 2, 0, 1, 1, 0)),
    E('S2', (2, 56, 8, 3, 5), 1, 'none', 0, 1, (2, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('S2', (2, 56, 8, 1, 1), 1, 'none', 3, 1, (2, 0, 1, 1, 2, 1, 1, 1, 0)),
    E('S2', (2, 16, 8, 9, 9), 0, 'none', 4, 1, (2, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 16, 8, 17, 5), 0, 'none', 0, 1, (2, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('S2', (2, 64, 8, 9, 9), 0, 'none', 3, 1, (2, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 64, 8, 17, 5), 0, 'none', 4, 1, (2, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('S2', (2, 16, 8, 9, 9), 1, 'none', 0, 1, (2, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('S2', (2, 16, 8, 17, 5), 1, 'none', 3, 1, (2, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('S2', (2, 64, 8, 9, 9), 1, 'none', 4, 1, (2, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('S2', (2, 64, 8, 17, 5), 1, 'none', 0, 1, (2, 1, 0, 0, 2, 1, 1, 1, 1)),
    # class 0 kept above T2_TC1_LIMIT: the large entries, no activation
    E('T2', (2, 12, 96, 192, 192), 0, 'none', 0, 1, (0, 0, 0, 0, 2, 0, 3, 0, 0)),
    E('T2', (2, 12, 96, 192, 192), 1, 'none', 0, 1, (0, 0, 0, 0, 2, 0, 3, 0, 0)),
    E('T2', (2, 16, 96, 192, 192), 0, 'none', 0, 1, (0, 1, 0, 0, 2, 0, 3, 0, 0)),
    E('T2', (2, 16, 96, 192, 192), 1, 'none', 0, 1, (0, 1, 0, 0, 2, 0, 3, 0, 0)),
    E('T2', (2, 12, 48, 4, 4), 0, 'none', 3, 1, (1, 0, 0, 0, 3, 0, 1, 0, 0)),
    E('T2', (2, 12, 48, 8, 8), 0, 'none', 4, 1, (1, 0, 0, 0, 3, 0, 3, 0, 0)),
    E('T2', (2, 120, 48, 4, 4), 0, 'none', 0, 1, (1, 0, 0, 0, 3, 1, 1, 0, 0)),
    E('T2', (2, 120, 48, 8, 8), 0, 'none', 3, 1, (1, 0, 0, 0, 3, 1, 3, 0, 0)),
    E('T2', (2, 12, 48, 4, 4), 1, 'none', 4, 1, (1, 0, 0, 0, 3, 0, 1, 0, 0)),
    E('T2', (2, 12, 48, 8, 8), 1, 'none', 0, 1, (1, 0, 0, 0, 3, 0, 3, 0, 0)),
    E('T2', (2, 120, 48, 4, 4), 1, 'none', 3, 1, (1, 0, 0, 0, 3, 1, 1, 0, 0)),
    E('T2', (2, 120, 48, 8, 8), 1, 'none', 4, 1, (1, 0, 0, 0, 3, 1, 3, 0, 0)),
    E('T2', (2, 12, 48, 1, 1), 0, 'none', 0, 1, (1, 0, 0, 1, 3, 0, 1, 0, 0)),
    E('T2', (2, 120, 48, 1, 1), 0, 'none', 3, 1, (1, 0, 0, 1, 3, 1, 1, 0, 0)),
    E('T2', (2, 12, 48, 1, 1), 1, 'none', 4, 1, (1, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('T2', (2, 120, 48, 1, 1), 1, 'none', 0, 1, (1, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('T2', (2, 16, 48, 4, 4), 0, 'none', 3, 1, (1, 1, 0, 0, 3, 0, 1, 0, 0)),
    E('T2', (2, 16, 48, 8, 2), 0, 'none', 4, 1, (1, 1, 0, 0, 3, 0, 1, 1, 1)),
    E('T2', (2, 16, 48, 8, 8), 0, 'none', 0, 1, (1, 1, 0, 0, 3, 0, 3, 0, 0)),
    E('T2', (2, 128, 48, 4, 4), 0, 'none', 3, 1, (1, 1, 0, 0, 3, 1, 1, 0, 0)),
    E('T2', (2, 128, 48, 8, 2), 0, 'none', 4, 1, (1, 1, 0, 0, 3, 1, 1, 1, 1)),
    E('T2', (2, 128, 48, 8, 8), 0, 'none', 0, 1, (1, 1, 0, 0, 3, 1, 3, 0, 0)),
    E('T2', (2, 16, 48, 4, 4), 1, 'none', 3, 1, (1, 1, 0, 0, 3, 0, 1, 0, 0)),
    E('T2', (2, 16, 48, 8, 2), 1, 'none', 4, 1, (1, 1, 0, 0, 3, 0, 1, 1, 1)),
    E('T2', (2, 16, 48, 8, 8), 1, 'none', 0, 1, (1, 1, 0, 0, 3, 0, 3, 0, 0)),
    E('T2', (2, 128, 48, 4, 4), 1, 'none', 3, 1, (1, 1, 0, 0, 3, 1, 1, 0, 0)),
    E('T2', (2, 128, 48, 8, 2), 1, 'none', 4, 1, (1, 1, 0, 0, 3, 1, 1, 1, 1)),
    E('T2', (2, 128, 48, 8, 8), 1, 'none', 0, 1, (1, 1, 0, 0, 3, 1, 3, 0, 0)),
    E('T2', (2, 12, 8, 4, 8), 0, 'none', 3, 1, (2, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('T2', (2, 12, 8, 8, 9), 0, 'none', 4, 1, (2, 0, 0, 0, 2, 0, 3, 0, 0)),
    E('T2', (2, 120, 8, 4, 8), 0, 'none', 0, 1, (2, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('T2', (2, 120, 8, 8, 9), 0, 'none', 3, 1, (2, 0, 0, 0, 2, 1, 3, 0, 0)),
    E('T2', (2, 12, 8, 4, 8), 1, 'none', 4, 1, (2, 0, 0, 0, 2, 0, 1, 0, 0)),
    E('T2', (2, 12, 8, 8, 9), 1, 'none', 0, 1, (2, 0, 0, 0, 2, 0, 3, 0, 0)),
    E('T2', (2, 120, 8, 4, 8), 1, 'none', 3, 1, (2, 0, 0, 0, 2, 1, 1, 0, 0)),
    E('T2', (2, 120, 8, 8, 9), 1, 'none', 4, 1, (2, 0, 0, 0, 2, 1, 3, 0, 0)),
    E('T2', (2, 12, 8, 1, 2), 0, 'none', 0, 1, (2, 0, 0, 1, 2, 0, 1, 0, 0)),
    E('T2', (2, 12, 8, 1, 1), 0, 'none', 3, 1, (2, 0, 0, 1, 2, 0, 1, 1, 0)),
    E('T2', (2, 12, 8, 8, 8), 0, 'none', 4, 1, (2, 0, 0, 1, 2, 0, 3, 0, 0)),
    E('T2', (2, 120, 8, 1, 2), 0, 'none', 0, 1, (2, 0, 0, 1, 2, 1, 1, 0, 0)),
    E('T2', (2, 120, 8, 1, 1), 0, 'none', 3, 1, (2, 0, 0, 1, 2, 1, 1, 1, 0)),
    E('T2', (2, 120, 8, 8, 8), 0, 'none', 4, 1, (2, 0, 0, 1, 2, 1, 3, 0, 0)),
    E('T2', (2, 12, 8, 1, 2), 1, 'none', 0, 1, (2, 0, 1, 1, 2, 0, 1, 0, 0)),
    E('T2', (2, 12, 8, 1, 1), 1, 'none', 3, 1, (2, 0, 1, 1, 2, 0, 1, 1, 0)),
    E('T2', (2, 12, 8, 8, 8), 1, 'none', 4, 1, (2, 0, 1, 1, 2, 0, 3, 0, 0)),
    E('T2', (2, 120, 8, 1, 2), 1, 'none', 0, 1, (2, 0, 1, 1, 2, 1, 1, 0, 0)),
    E('T2', (2, 120, 8, 1, 1), 1, 'none', 3, 1, (2, 0, 1, 1, 2, 1, 1, 1, 0)),
    E('T2', (2, 120, 8, 8, 8), 1, 'none', 4, 1, (2, 0, 1, 1, 2, 1, 3, 0, 0)),
    E('T2', (2, 16, 8, 4, 8), 0, 'none', 0, 1, (2, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('T2', (2, 16, 8, 8, 4), 0, 'none', 3, 1, (2, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('T2', (2, 16, 8, 8, 9), 0, 'none', 4, 1, (2, 1, 0, 0, 2, 0, 3, 0, 0)),
    E('T2', (2, 16, 8, 9, 8), 0, 'none', 0, 1, (2, 1, 0, 0, 2, 0, 3, 1, 1)),
    E('T2', (2, 128, 8, 4, 8), 0, 'none', 3, 1, (2, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('T2', (2, 128, 8, 8, 4), 0, 'none', 4, 1, (2, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('T2', (2, 128, 8, 8, 9), 0, 'none', 0, 1, (2, 1, 0, 0, 2, 1, 3, 0, 0)),
    E('T2', (2, 128, 8, 9, 8), 0, 'none', 3, 1, (2, 1, 0, 0, 2, 1, 3, 1, 1)),
    E('T2', (2, 16, 8, 4, 8), 1, 'none', 4, 1, (2, 1, 0, 0, 2, 0, 1, 0, 0)),
    E('T2', (2, 16, 8, 8, 4), 1, 'none', 0, 1, (2, 1, 0, 0, 2, 0, 1, 1, 1)),
    E('T2', (2, 16, 8, 8, 9), 1, 'none', 3, 1, (2, 1, 0, 0, 2, 0, 3, 0, 0)),
    E('T2', (2, 16, 8, 9, 8), 1, 'none', 4, 1, (2, 1, 0, 0, 2, 0, 3, 1, 1)),
    E('T2', (2, 128, 8, 4, 8), 1, 'none', 0, 1, (2, 1, 0, 0, 2, 1, 1, 0, 0)),
    E('T2', (2, 128, 8, 8, 4), 1, 'none', 3, 1, (2, 1, 0, 0, 2, 1, 1, 1, 1)),
    E('T2', (2, 128, 8, 8, 9), 1, 'none', 4, 1, (2, 1, 0, 0, 2, 1, 3, 0, 0)),
    E('T2', (2, 128, 8, 9, 8), 1, 'none', 0, 1, (2, 1, 0, 0, 2, 1, 3, 1, 1)),
]

# ---- entries about something inside a form: the same keys again, with the further answers of the query they are about
EDGES = [
    # general because K != Kp (24 is a multiple of KC = 8 but not of the channel padding)
    E('3X3', (2, 24, 96, 9, 5), 0, 'none', 3, 1, (0, 0, 0, 0, 3, 0, 1, 0, 0), 'k24'),
    E('S2', (2, 24, 96, 9, 5), 0, 'none', 4, 1, (0, 0, 0, 0, 2, 0, 1, 0, 0), 'k24'),
    E('1X1', (2, 24, 96, 9, 5), 0, 'none', 3, 1, (0, 0, 0, 0, 2, 0, 1, 0, 0), 'k24'),
    E('T2', (2, 24, 48, 4, 4), 0, 'none', 3, 1, (1, 0, 0, 0, 3, 0, 1, 0, 0), 'k24'),
    # the same shape with and without workspace: split and not
    E('3X3', (2, 64, 96, 3, 17), 0, 'none', 3, 0, (0, 1, 0, 0, 3, 0, 1, 0, 0), 'nows', ksplit=1),
    E('3X3', (2, 56, 96, 9, 5), 0, 'none', 3, 0, (0, 0, 0, 0, 3, 0, 1, 0, 0), 'nows', ksplit=1),
    E('3X3', (4, 128, 96, 4, 4), 0, 'none', 3, 1, (0, 0, 0, 1, 3, 1, 1, 0, 0), 'ks4', ksplit=4),
    E('3X3', (4, 128, 96, 4, 4), 0, 'none', 3, 0, (0, 0, 0, 1, 3, 0, 1, 0, 0), 'nows', ksplit=1),
    E('T2', (2, 128, 48, 8, 8), 1, 'none', 0, 0, (1, 1, 0, 0, 3, 0, 3, 0, 0), 'nows', ksplit=1),
    E('S2', (2, 64, 96, 9, 5), 0, 'none', 4, 0, (0, 1, 0, 0, 2, 0, 1, 1, 1), 'nows', ksplit=1),
    E('1X1', (2, 56, 96, 9, 5), 0, 'res', 3, 0, (0, 0, 0, 0, 2, 0, 1, 0, 0), 'nows', ksplit=1),
    # the banded block-to-tile mapping: 1, 7, 8 and 9 body tiles (8 XCD bands; 9 tiles leave 7 of 16 blocks without one), 1 and 2 M blocks
    E('3X3', (1, 16, 128, 4, 32), 0, 'none', 3, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0), 'tiles1', nbody=1, mblocks=1, grid_x=8),
    E('3X3', (1, 16, 128, 28, 32), 0, 'none', 3, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0), 'tiles7', nbody=7, mblocks=1, grid_x=8),
    E('3X3', (1, 16, 128, 32, 32), 0, 'none', 3, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0), 'tiles8', nbody=8, mblocks=1, grid_x=8),
    E('3X3', (1, 16, 128, 36, 32), 0, 'none', 3, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0), 'tiles9', nbody=9, mblocks=1, grid_x=16),
    E('3X3', (1, 16, 129, 28, 32), 0, 'none', 3, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0), 'tiles7_m129', nbody=7, mblocks=2, grid_x=16),
    E('3X3', (1, 16, 129, 36, 32), 1, 'none', 3, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0), 'tiles9_m129', nbody=9, mblocks=2, grid_x=32),
    E('3X3', (1, 12, 129, 36, 32), 0, 'none', 4, 1, (0, 0, 0, 0, 3, 0, 1, 0, 0), 'tiles9_m129', nbody=9, mblocks=2, grid_x=32),
    # geometry inside a form: a partial last tile along x and along y, W = 3 and W = 2 (see the docstring)
    E('3X3', (2, 16, 128, 8, 40), 0, 'none', 3, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0), 'w40', r0_TW=32, r0_tiles_x=2),
    E('3X3', (2, 16, 128, 6, 32), 0, 'none', 3, 1, (0, 1, 0, 0, 3, 0, 1, 0, 0), 'h6', r0_TH=4, r0_tiles_y=2),
    E('S2', (2, 16, 96, 6, 40), 0, 'none', 3, 1, (0, 1, 0, 0, 2, 0, 1, 0, 0), 'h6w40', r0_tiles_x=2, r0_tiles_y=2),
    E('3X3', (2, 16, 96, 9, 3), 0, 'none', 3, 1, (0, 0, 0, 1, 3, 0, 1, 0, 0), 'w3', r0_TW=4, r0_NS=2),
    E('3X3', (2, 16, 96, 64, 3), 0, 'none', 4, 1, (0, 1, 0, 0, 3, 0, 1, 1, 1), 'w3', r0_TW=4),
    E('3X3', (2, 16, 96, 64, 2), 0, 'none', 3, 1, (0, 0, 0, 0, 3, 0, 1, 0, 0), 'w2', r0_TW=2, r0_NS=1),
    E('S2', (2, 16, 96, 64, 2), 1, 'none', 3, 1, (0, 0, 0, 0, 2, 0, 1, 0, 0), 'w2', r0_TW=2, r0_NS=1),
    # T2: the padded single region with only one of H, W small; three regions with 8 and with 9 body tiles; class 0 demoted to class 1
    # under T2_TC1_LIMIT (M = 96 is class 0 by its width); the last-column region's rows halved in the general form
    E('T2', (2, 16, 48, 4, 16), 0, 'none', 3, 1, (1, 1, 0, 0, 3, 0, 1, 0, 0), 'h4', nbody=6),
    E('T2', (2, 16, 48, 16, 4), 0, 'none', 3, 1, (1, 1, 0, 0, 3, 0, 1, 0, 0), 'w4', nbody=6),
    E('T2', (1, 16, 48, 16, 32), 0, 'none', 3, 1, (1, 1, 0, 0, 3, 0, 3, 0, 0), 'body8', nbody=8, ntiles=11, grid_x=16),
    E('T2', (1, 16, 48, 18, 32), 0, 'none', 3, 1, (1, 1, 0, 0, 3, 0, 3, 0, 0), 'body9', nbody=9, ntiles=12, grid_x=24),
    E('T2', (2, 16, 96, 16, 16), 0, 'none', 3, 1, (1, 1, 0, 0, 3, 0, 3, 0, 0), 'demoted', mblocks=2),
    E('T2', (2, 12, 96, 16, 16), 1, 'none', 3, 1, (1, 0, 0, 0, 3, 0, 3, 0, 0), 'demoted', mblocks=2),
    E('T2', (2, 12, 8, 128, 9), 0, 'none', 3, 1, (2, 0, 0, 0, 2, 0, 3, 0, 0), 'edgeth', r1_TW=1, r1_TH=64, r1_TH0=128, r1_tapmask=0x124, r2_tapmask=0x1C0),
    # the deep-stage 1x1 promoted by the plan and refused by FAST (TW = 2): class 0, general form
    E('1X1', (2, 64, 128, 8192, 2), 0, 'none', 3, 1, (0, 0, 0, 0, 2, 0, 1, 0, 0), 'tc3_fallback', r0_TW=2, ksplit=1),
    E('1X1', (2, 64, 128, 8192, 2), 0, 'both', 3, 1, (0, 0, 0, 0, 2, 0, 1, 0, 0), 'tc3_fallback', r0_TW=2, ksplit=1),
]


def _epi_variants():
    """residual, mask and both on the FAST, general single-sample and multi-sample forms of the 3x3 and 1x1 kinds (PER_KEY has one of
    the three per key)"""
    out = []
    for kind, shape, form in (('3X3', (2, 16, 96, 3, 17), (0, 1, 0, 0, 3, 0, 1, 0, 0)), ('3X3', (2, 12, 96, 9, 5), (0, 0, 0, 0, 3, 0, 1, 0, 0)),
                              ('3X3', (2, 12, 96, 2, 2), (0, 0, 1, 1, 2, 0, 1, 0, 0)), ('1X1', (2, 64, 128, 128, 128), (3, 1, 0, 0, 2, 0, 1, 0, 0)),
                              ('1X1', (2, 12, 96, 9, 5), (0, 0, 0, 0, 2, 0, 1, 0, 0)), ('1X1', (2, 12, 96, 1, 1), (0, 0, 1, 1, 2, 0, 1, 0, 0))):
        for i, epi in enumerate(EPIS[1:]):
            out.append(E(kind, shape, 0, epi, (3, 4, 0)[i], 1, form, epi))
    return out


EPI = _epi_variants()
TABLE = PER_KEY + EDGES + EPI
BY_NAME = {e.name: e for e in TABLE}
assert len(BY_NAME) == len(TABLE), 'entry names must be unique'

# (kind, shape, has_isc, epi): the launch refuses these, and so does the query, with TE_ERR_UNSUPPORTED
REFUSED = [('3X3', (2, 16, 96, 9, 5), 1, 'res'), ('1X1', (2, 16, 96, 9, 5), 1, 'both'), ('3X3', (2, 12, 8, 1, 1), 1, 'mask'),
           ('S2', (2, 16, 96, 9, 5), 0, 'res'), ('T2', (2, 16, 96, 9, 5), 0, 'mask')]
# one entry per kind that the GPU test also runs with the data-gradient pack (PACK_DGRAD: 3x3 / 1x1, PACK_SWAP: S2 / T2)
DGRAD = ('3x3_tc0_fast_isc', 's2_tc1_gen_multi_isc', 't2_tc1_fast_isc_r3', '1x1_tc0_gen_multi_isc')


# ------------------------------------------------------------------------------------------------ what the library plans
def answer(entry_or_kind, shape=None, has_isc=0, epi='none', with_ws=1):
    """te_conv_form's answer (dict) for an entry, or for explicit arguments; a negative TE_ERR_* code where the launch refuses"""
    if isinstance(entry_or_kind, Form):
        e = entry_or_kind
        return _lib.conv_form(KINDS[e.kind], *e.shape, e.has_isc, e.epi, e.with_ws)
    return _lib.conv_form(KINDS[entry_or_kind], *shape, has_isc, epi, with_ws)


def form_of(ans):
    """FORM_FIELDS of an answer"""
    r0 = ans['regions'][0]
    return (ans['tc'], ans['fast'], ans['ms'], ans['multi_sample'], ans['occ'], int(ans['ksplit'] > 1), ans['nreg'],
            int(r0['NSv'] < r0['NS']), int(r0['TH'] < r0['TH0']))


def key_of(kind, has_isc, epi, form):
    return (kind, int(has_isc), int(epi != 'none')) + tuple(form)


def key(entry):
    return key_of(entry.kind, entry.has_isc, entry.epi, entry.form)


def answer_fields(ans):
    """the flat namespace of Form.expect: the head fields of the answer, and rN_FIELD for the fields of region N"""
    flat = {k: v for k, v in ans.items() if k != 'regions'}
    for i, r in enumerate(ans['regions']):
        flat.update({f'r{i}_{k}': v for k, v in r.items()})
    return flat


def check(entry):
    """raise AssertionError naming the entry when the library does not plan the declared form for it; returns the answer"""
    ans = answer(entry)
    assert not isinstance(ans, int), f'{entry.name}: te_conv_form refuses {entry.kind} {entry.shape} ({ans})'
    got = form_of(ans)
    assert got == entry.form, f'{entry.name} {entry.kind} {entry.shape}: expected {dict(zip(FORM_FIELDS, entry.form))}, the library plans {dict(zip(FORM_FIELDS, got))}'
    flat = answer_fields(ans)
    for k, v in entry.expect.items():
        assert flat[k] == v, f'{entry.name} {entry.kind} {entry.shape}: expected {k} = {v}, the library plans {flat[k]}'
    return ans


if __name__ == '__main__':
    by_key = {}
    for e in TABLE:
        by_key.setdefault(key(e), []).append(e.name)
    print('kind isc epi | ' + ' '.join(FORM_FIELDS))
    for k in sorted(by_key, key=str):
        print(' '.join(str(v) for v in k[:3]), '|', ' '.join(str(v) for v in k[3:]), ':', ', '.join(by_key[k]))
    print(f'{len(by_key)} keys, {len(TABLE)} entries')

"""Host-plan table: every answer of the library's host-only launch planners over one fixed grid of arguments.

The planners (te_*_plan, te_*_count, te_*_cover, te_conv_packed_numel, te_*_tiles, te_wgrad_pair_form, te_wgrad6_form, te_wgrad_form,
te_conv_split_form, te_fir_form in include/te_hip.h) launch nothing and need no GPU.  Their answers fix the summation partition of the split launches (so every result
bit) and are what the loop-trip and route tests assert their coverage with, yet a planner that drifts from its launch fails no other
test.  table(lib) calls each of them over the grid below and returns {name: int array}; return codes are part of the table.

    python tests/host_plans.py LIB OUT.npz        # the table of any library file

tests/golden/host_plans.npz is the table of the library before the planners were derived from the launch code's own geometry;
tests/test_host_plans_cpu.py asserts that the current library still gives it.  A planner that is added later is recorded next to its
relatives from the library that introduces it, with every older answer unchanged (wgrad_form: the plan of the fp32 weight-gradient launch;
conv_split_form: the plan of the split-bf16 forward launches under three settings of their form hooks; fir_form: the plan of the three
FIR launches, the upfirdn2d grid under op 0 and the blur grid under ops 1 and 2).
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from transeditor_amd import _abi, _lib  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'host_plans.npz')

# ---- the grid
CONV_KINDS = range(0, 9)
BATCHES = (1, 2, 3, 4, 16, 32)
CHANNELS = (3, 32, 48, 64, 96, 128, 512, 513)
SIZES = ((1, 1), (2, 2), (4, 4), (7, 9), (8, 8), (9, 7), (16, 16), (17, 17), (32, 32), (64, 64), (256, 256))      # H x W
PACK_KINDS = range(-1, 14)
PACK_CHANNELS = (5, 6, 32, 48, 128, 256, 513)
KSIZES = (1, 2, 3)
WGRAD_KINDS = (_lib.CONV_3X3, _lib.CONV_T2, _lib.CONV_1X1)
WGRAD_CHANNELS = tuple(itertools.product(CHANNELS, CHANNELS)) + ((32, 32),)                                          # (Co, Ci)
REDUCE = tuple(itertools.product((1, 3, 16), (1, 2, 13), (3, 16, 48, 256, 513), (32, 33, 256), (1, 9, 4)))             # B, S, Co, Ci, taps
REDUCE_WANTS = ((1, 0, 0), (1, 1, 1), (0, 1, 0), (0, 0, 1))

# FIR problems: the shapes of tests/loop_trips.py (planes, H, W), then widths 3, 4, 33, 65, 257 under three heights
FIR_SHAPES = ((7145, 6, 7), (7145, 33, 65), (1636, 40, 70), (13065, 4, 8), (13065, 8, 16), (13065, 4, 3)) + tuple(
    (m, h, w) for m, h in ((1, 4), (7, 33), (300, 257)) for w in (3, 4, 33, 65, 257))
FIR_PADS = ((2, 1), (1, 1), (1, 2), (0, 0), (-1, -1), (-1, 2), (3, 3))                                                # (pad0, pad1) on both axes
FIR_BAD = (     # (major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, four pads): bad arguments and the odd corners
    (0, 8, 8, 1, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1), (-1, 8, 8, 1, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1), (5, 0, 8, 1, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1),
    (5, 8, 0, 1, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1), (5, 8, 8, 0, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1), (5, 8, 8, 1, 0, 4, 1, 1, 1, 1, 2, 1, 2, 1),
    (5, 8, 8, 1, 4, 0, 1, 1, 1, 1, 2, 1, 2, 1), (5, 8, 8, 1, 4, 4, 0, 1, 1, 1, 2, 1, 2, 1), (5, 8, 8, 1, 4, 4, 1, 1, 1, 0, 2, 1, 2, 1),
    (5, 8, 8, 1, 4, 4, 2, 1, 1, 1, 2, 1, 2, 1), (5, 8, 8, 1, 4, 4, 1, 1, 2, 1, 2, 1, 2, 1), (5, 8, 8, 1, 4, 3, 1, 1, 1, 1, 2, 1, 2, 1),
    (5, 2, 2, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0), (5, 8, 8, 1, 4, 4, 1, 1, 1, 1, 2, 1, -9, 1), (1 << 30, 8, 8, 1, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1),
    (5, 40000, 40000, 1, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1))
BLUR_TAPS = ((4, 4), (3, 3), (4, 3))
BLUR_PADS = ((1, 2, 1, 2), (2, 1, 2, 1), (0, 0, 0, 0), (-1, 2, 1, 2), (1, 2, 1, -1), (2, 2, 2, 2), (0, 0, 0, 3), (3, 3, -4, 0))   # x0, x1, y0, y1
BLUR_BAD = (    # (major, in_h, in_w): bad and odd ones, each under every tap / pad combination above
    (0, 8, 8), (-1, 8, 8), (5, 0, 8), (5, 8, 0), (5, 8, -3), (5, 1, 1), (1 << 30, 8, 8), (5, 40000, 40000))
COVER_OUTPUTS = (-1, 0, 1, 255, 256, 257, 1 << 20, (1 << 20) + 1, 1054152, 1 << 31, 1 << 40)


def load(path):
    """CDLL of any libte_hip.so, with the prototypes of include/te_hip.h"""
    L = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _abi.parse(_lib._header_text()).items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


def _two(fn, *args, second=C.c_int):
    """(rc, *a, *b) of a planner with two outputs, which start as -1 so that a refusal shows them untouched"""
    a, b = C.c_int(-1), second(-1)
    rc = fn(*args, C.byref(a), C.byref(b))
    return rc, a.value, b.value


def _conv(L):
    return {'conv_splitk_count': [L.te_conv_splitk_count(kind, B, K, M, H, W)
                                  for kind in CONV_KINDS for B in BATCHES for K in CHANNELS for M in CHANNELS for H, W in SIZES]}


SPLIT_KINDS = (_lib.CONV_3X3W6, _lib.CONV_S2S6, _lib.CONV_T2S6, _lib.CONV_1X1S6)
SPLIT_HOOKS = ((2, 0, 1, 1), (3, 3, 2, 2), (1, 0, 0, 0))          # te_conv_wino6_form, _tiles_per_block, te_conv_s2s6_form, te_conv_t2s6_form


def _split_form(L):
    """(rc, *form) of te_conv_split_form under the default hooks, the forced two-image forms with runs of three, and the ping-pong forms;
    with style scales and scratch, and without; the form starts as -1 so that a refusal shows it untouched"""
    n = len(_lib.CONV_SPLIT_FORM)
    hooks = (L.te_conv_wino6_form, L.te_conv_wino6_tiles_per_block, L.te_conv_s2s6_form, L.te_conv_t2s6_form)
    saved = [h(-1) for h in hooks]
    out = []
    try:
        for values in SPLIT_HOOKS:
            for h, v in zip(hooks, values):
                h(v)
            for kind in SPLIT_KINDS:
                for B in BATCHES:
                    for K in CHANNELS:
                        for M in CHANNELS:
                            for H, W in SIZES:
                                for flag in (0, 1):
                                    form = (C.c_int * n)(*([-1] * n))
                                    out.append((L.te_conv_split_form(kind, B, K, M, H, W, flag, flag, form),) + tuple(form))
    finally:
        for h, v in zip(hooks, saved):
            h(v)
    return {'conv_split_form': out}


def _pack(L):
    grid = [(kind, Co, Ci, ks) for kind in PACK_KINDS for Co in PACK_CHANNELS for Ci in PACK_CHANNELS for ks in KSIZES]
    return {'conv_packed_numel': [L.te_conv_packed_numel(*g) for g in grid],
            'conv_pack_plan': [_two(L.te_conv_pack_plan, *g) for g in grid]}


def _wgrad_form(L, *args):
    """(rc, *form) of te_wgrad_form for aligned operands; the form starts as -1 so that a refusal shows it untouched"""
    form = (C.c_int * len(_lib.WGRAD_FORM))(*([-1] * len(_lib.WGRAD_FORM)))
    return (L.te_wgrad_form(*args, 0, 0, form),) + tuple(form)


def _wgrad(L):
    out = {'wgrad_slab_count': [], 'wgrad_group_plan': [], 'wgrad_pair_form': [], 'wgrad6_form': [], 'wgrad_form': []}
    saved = L.te_wgrad_split_bf16(-1)
    try:
        for on in (0, 1):
            L.te_wgrad_split_bf16(on)
            for kind in WGRAD_KINDS:
                for B in BATCHES:
                    for Co, Ci in WGRAD_CHANNELS:
                        for H, W in SIZES:
                            rc, NB, S = _two(L.te_wgrad_group_plan, kind, B, Co, Ci, H, W)
                            out['wgrad_slab_count'].append(L.te_wgrad_slab_count(kind, B, Co, Ci, H, W))
                            out['wgrad_group_plan'].append((rc, NB, S))
                            out['wgrad_pair_form'].append(L.te_wgrad_pair_form(kind, Co, Ci, H, W))
                            # the kernel of the per-sample launch and of the planned grouped one
                            out['wgrad6_form'].append((L.te_wgrad6_form(kind, B, Co, Ci, H, W, 1), L.te_wgrad6_form(kind, B, Co, Ci, H, W, NB)))
                            # the plan of the same two launches (16-byte aligned operands) with the planners' chunk counts
                            out['wgrad_form'].append(_wgrad_form(L, kind, B, Co, Ci, H, W, out['wgrad_slab_count'][-1], 1) +
                                                     _wgrad_form(L, kind, B, Co, Ci, H, W, S, NB))
    finally:
        L.te_wgrad_split_bf16(saved)
    out['wgrad_slab_count_bad'] = [L.te_wgrad_slab_count(0, *g) for g in ((0, 64, 64, 8, 8), (2, 0, 64, 8, 8), (2, 64, 64, 8, 0))]
    return out


def _reduce(L):
    return {'wgrad_reduce_ws_floats': [L.te_wgrad_reduce_ws_floats(*g, *w) for g in REDUCE for w in REDUCE_WANTS],
            'wgrad_reduce_plan': [_two(L.te_wgrad_reduce_plan, *g, second=C.c_int64) for g in REDUCE]}


def fir_grid():
    g = [(m, h, w, minor, k, k, up, up, down, down, p0, p1, p0, p1)
         for m, h, w in FIR_SHAPES for minor in (1, 2) for k in (3, 4) for up in (1, 2) for down in (1, 2) for p0, p1 in FIR_PADS]
    return g + list(FIR_BAD)


def blur_grid():
    return [(m, h, w, kh, kw, *pads) for m, h, w in FIR_SHAPES + BLUR_BAD for kh, kw in BLUR_TAPS for pads in BLUR_PADS]


def _fir_form(L, op, *args):
    """(rc, *form) of te_fir_form; the form starts as -1 so that a refusal shows it untouched"""
    n = len(_lib.FIR_FORM)
    form = (C.c_int * n)(*([-1] * n))
    return (L.te_fir_form(op, *args, form),) + tuple(form)


def _fir(L):
    blur = blur_grid()
    return {'fir_form': [_fir_form(L, 0, *g) for g in fir_grid()] +
                        [_fir_form(L, op, m, h, w, 1, kh, kw, 1, 1, 1, 1, *pads) for op in (1, 2) for m, h, w, kh, kw, *pads in blur],
            'upfirdn2d_plan': [_two(L.te_upfirdn2d_plan, *g) for g in fir_grid()],
            'blur_actgrad_plan': [_two(L.te_blur_actgrad_plan, *g) for g in blur],
            'blur_gradact_plan': [_two(L.te_blur_gradact_plan, *g) for g in blur],
            'blur_actgrad_tiles': [L.te_blur_actgrad_tiles(*g[1:]) for g in blur],
            'upfirdn2d_direct_cover': [L.te_upfirdn2d_direct_cover(n) for n in COVER_OUTPUTS]}


# the three FIR plans answer a refusal with the launch's own negative code: only the sign of their return code (column 0) is pinned
REFUSAL_CODE_FREE = ('upfirdn2d_plan', 'blur_actgrad_plan', 'blur_gradact_plan')


def table(L):
    """{name: int64 array, one row per grid point} of every planner answer of library L"""
    t = {}
    for part in (_conv, _split_form, _pack, _wgrad, _reduce, _fir):
        t.update(part(L))
    return {k: np.asarray(v, dtype=np.int64) for k, v in t.items()}


def differences(golden, current):
    """{name: rows that differ} between two tables, after the one permitted exception (REFUSAL_CODE_FREE)"""
    assert set(golden) == set(current), f'tables name different planners: {sorted(set(golden) ^ set(current))}'
    diff = {}
    for name in sorted(golden):
        g, c = np.asarray(golden[name], dtype=np.int64), np.asarray(current[name], dtype=np.int64)
        assert g.shape == c.shape, f'{name}: the grid changed ({g.shape} -> {c.shape})'
        bad = g != c
        if name in REFUSAL_CODE_FREE:
            bad[:, 0] = np.where(g[:, 0] < 0, c[:, 0] >= 0, bad[:, 0])       # a refusal stays a refusal, whatever its code
        rows = np.flatnonzero(bad.reshape(len(g), -1).any(axis=1))
        if len(rows):
            diff[name] = rows
    return diff


def answers(t):
    return int(sum(v.size for v in t.values()))


if __name__ == '__main__':
    lib_path, out_path = sys.argv[1:3]
    tab = table(load(lib_path))
    np.savez_compressed(out_path, **{k: v.astype(np.int64 if np.abs(v).max() >= 1 << 31 else np.int32) for k, v in tab.items()})
    print(f'{out_path}: {answers(tab)} answers of {len(tab)} planners, {os.path.getsize(out_path)} bytes')

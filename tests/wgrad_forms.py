"""Form table of the fp32 weight-gradient kernel: the smallest shapes that land on every instantiation of wgrad_mfma_kernel<KIND, NWP, WINO>
(csrc/wgrad.hip), on both staging paths, and on the edges inside a form.

Which kernel a launch runs is decided by the kind, the channel counts (pick_nwp: 2 waves along the plain operand where Co, Ci <= 64, else 4),
the cell tile (pair form of the 3x3 kind: NC % 4 == 0 on the 4-wave tile), the width and the alignment of g and x (vec, the 16-byte staging
path), the split-bf16 switch and te_wgrad_split_supported (whether the kernel runs at all).  te_wgrad_form (include/te_hip.h) reports the
plan that the launch itself makes and then dispatches on.  An entry names the kind, (B, Co, Ci, H, W), S and NB as handed to the launch,
the split switch, the offset of g and x from 16-byte alignment in bytes (0 or 4), and what it is expected to land on: the key
(kind, nwp, wino, vec, db) and its per-block facts - `trips`, the cell tiles of each of the S chunks (= trips of a block's tile loop), and
`ks`, the kstride of every channel block in grid (y, z) order (1 on the 4-wave tile; 1, 2 or 4 on the 2-wave tile, where the waves that would
multiply padding share the cells).  The expected values are data; what a launch does comes from the query: facts() derives trips and ks
from the query's TW, TH, tiles and grid by the kernel's rule (nPB, nQB from min(block, C - c0)).  tests/test_wgrad_forms_cpu.py checks the
table against the query and sweeps the query for keys the table lacks; tests/test_gpu_wgrad_forms.py runs every entry against fp64 after
re-asserting its key.  The list of keys with their entries: `python tests/wgrad_forms.py`.

Cell tile: TW = clamp(pow2ceil(W), 2, 32), TH = clamp(pow2ceil(H), 1, NCELL / TW), NCELL 64 (3x3, 1x1) or 32 (T2); NC = TW TH cells per
stage, NC / 2 k-steps (NC / 4 in the pair form).  vec needs TW = 32, W % 32 = 0, NC = NCELL, H % TH = 0 and aligned operands.

reference() is the fp64 restatement and the elementwise bound of the GPU test; it runs on whatever device the operands are on.
"""
import os
import sys
from dataclasses import dataclass

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from fp64_check import U32 as U, off16  # noqa: E402
from transeditor_amd import _lib  # noqa: E402

K3, KT, K1 = '3x3', 't2', '1x1'
KIND = {K3: _lib.CONV_3X3, KT: _lib.CONV_T2, K1: _lib.CONV_1X1}
NCELL = {K3: 64, KT: 32, K1: 64}


@dataclass(frozen=True)
class Entry:
    name: str
    kind: str
    B: int
    Co: int
    Ci: int
    H: int
    W: int
    S: int
    NB: int
    sw: int              # the split-bf16 switch during the launch
    off: int             # bytes by which g and x miss 16-byte alignment (0 or 4)
    key: tuple           # (kind, nwp, wino, vec, db)
    trips: tuple         # cell tiles of chunk s, s = 0 ... S - 1
    ks: tuple            # kstride of channel block (y, z), y-major

    def __hash__(self):
        return hash(self.name)


TABLE = []


def E(tag, kind, B, Co, Ci, H, W, S, NB, sw, off, key, trips, ks):
    nwp, wino, vec, db = key
    name = (f'{kind}_n{nwp}w{wino}v{vec}_{B}x{Co}x{Ci}x{H}x{W}_s{S}' + (f'g{NB}' if NB > 1 else '') + ('_off4' if off else '') +
            ('' if sw else '_sw0') + f'_{tag}')
    assert all(t.name != name for t in TABLE), name
    e = Entry(name, kind, B, Co, Ci, H, W, S, NB, sw, off, (kind, nwp, wino, vec, db), tuple(trips), tuple(ks))
    TABLE.append(e)
    return e


# the 13 keys as (nwp, wino, vec, db)
PV, PS = (4, 1, 1, 1), (4, 1, 0, 1)                 # 3x3 pair form, vec and scalar
D4 = (4, 0, 0, 1)                                   # 3x3 direct on the 4-wave tile (NC = 2), T2 4-wave scalar
T4V = (4, 0, 1, 1)                                  # T2 4-wave vec
P4V, P4 = (4, 0, 1, 0), (4, 0, 0, 0)                # 1x1 4-wave: a single image
N2V, N2 = (2, 0, 1, 0), (2, 0, 0, 0)                # the 2-wave tile of any kind

# ---- every key.  With whole 64-channel blocks (128 for 1x1) the split kernel takes the vec shapes under the default switch: switch off;
# 96 x 72 and 48 x 48 channels reach the same keys under the default switch (a channel tail on the vec path: rows past pC lie beyond the
# descriptor's range and read 0)
E('key', K3, 1, 128, 64, 2, 32, 1, 1, 0, 0, PV, (1,), (1,))
E('key', K3, 1, 96, 72, 2, 32, 1, 1, 1, 0, PV, (1,), (1, 1))
E('key', K3, 1, 128, 64, 2, 16, 1, 1, 1, 0, PS, (1,), (1,))
E('key', K3, 2, 130, 66, 1, 1, 1, 1, 1, 0, D4, (1,), (1, 1, 1, 1))
E('key', K3, 1, 96, 64, 1, 2, 1, 1, 1, 0, D4, (1,), (1,))
E('key', K3, 1, 64, 64, 2, 32, 1, 1, 0, 0, N2V, (1,), (1,))
E('key', K3, 1, 48, 48, 2, 32, 1, 1, 1, 0, N2V, (1,), (1,))
E('key', K3, 1, 64, 64, 4, 4, 1, 1, 1, 0, N2, (1,), (1,))
E('key', KT, 1, 128, 64, 1, 32, 1, 1, 0, 0, T4V, (1,), (1, 1))
E('key', KT, 1, 96, 72, 1, 32, 1, 1, 1, 0, T4V, (1,), (1, 1))
E('key', KT, 1, 128, 64, 2, 8, 1, 1, 1, 0, D4, (1,), (1, 1))
E('key', KT, 1, 64, 64, 1, 32, 1, 1, 0, 0, N2V, (1,), (1,))
E('key', KT, 1, 48, 48, 1, 32, 1, 1, 1, 0, N2V, (1,), (1,))
E('key', KT, 1, 64, 64, 2, 4, 1, 1, 1, 0, N2, (1,), (1,))
E('key', K1, 1, 128, 128, 2, 32, 1, 1, 0, 0, P4V, (1,), (1, 1))
E('key', K1, 1, 96, 72, 2, 32, 1, 1, 1, 0, P4V, (1,), (1, 1))
E('key', K1, 1, 128, 64, 4, 4, 1, 1, 1, 0, P4, (1,), (1,))
E('key', K1, 1, 64, 64, 2, 32, 1, 1, 1, 0, N2V, (1,), (1,))
E('key', K1, 1, 48, 48, 2, 32, 1, 1, 1, 0, N2V, (1,), (1,))
E('key', K1, 1, 64, 64, 4, 4, 1, 1, 1, 0, N2, (1,), (1,))

# ---- trips of the tile loop by explicit S: chunks of 0, 1, 2, 3 and 4 tiles, chunk boundaries inside a tile row (tiles_x = 2).  W = 64:
# vec, halo columns on both sides; W = 40: the scalar path with a ragged last tile column.  Four tiles (H = 4; T2: H = 2) under S = 1, 3, 5
# and six (H = 6; T2: H = 3) under S = 2.  Per kind a key with two LDS images and one with a single image (1x1 has only the latter).
for kind, Co, Ci, kv, ks_, sw_v, nblk in ((K3, 128, 64, PV, PS, 0, 1), (K3, 64, 64, N2V, N2, 0, 1), (KT, 128, 64, T4V, D4, 0, 2), (KT, 64, 64, N2V, N2, 0, 1),
                                         (K1, 128, 64, P4V, P4, 1, 1), (K1, 64, 64, N2V, N2, 1, 1)):
    h4, h6 = (2, 3) if kind == KT else (4, 6)
    for W, key, sw in ((64, kv, sw_v), (40, ks_, 1)):
        E('trips', kind, 1, Co, Ci, h4, W, 1, 1, sw, 0, key, (4,), (1,) * nblk)
        E('trips', kind, 1, Co, Ci, h4, W, 3, 1, sw, 0, key, (1, 1, 2), (1,) * nblk)
        E('trips', kind, 1, Co, Ci, h4, W, 5, 1, sw, 0, key, (0, 1, 1, 1, 1), (1,) * nblk)
        E('trips', kind, 1, Co, Ci, h6, W, 2, 1, sw, 0, key, (3, 3), (1,) * nblk)

# ---- k-step edges.  NC = 2 (a 1x1 image: one k-step, the quarter and half split points collapse), NC = 4 (2x2: the pair form's single
# step), NC = 32 below NCELL (W = 5, H = 3: TW 8, TH 4; W = 1, H = 9: TW 2, TH 16, the masked second column), full NC with ragged tiles
# (H = 3, W = 32: vec off because H % TH != 0, the second tile row half empty)
E('nc2', K3, 1, 64, 64, 1, 1, 1, 1, 1, 0, N2, (1,), (1,))
E('nc2', KT, 1, 64, 64, 1, 1, 1, 1, 1, 0, N2, (1,), (1,))
E('nc2', KT, 1, 128, 64, 1, 1, 1, 1, 1, 0, D4, (1,), (1, 1))
E('nc2', K1, 1, 128, 64, 1, 1, 1, 1, 1, 0, P4, (1,), (1,))
E('nc2', K1, 1, 64, 64, 1, 1, 1, 1, 1, 0, N2, (1,), (1,))
E('nc4', K3, 1, 128, 64, 2, 2, 1, 1, 1, 0, PS, (1,), (1,))
E('nc4', K3, 1, 64, 64, 2, 2, 1, 1, 1, 0, N2, (1,), (1,))
E('nc4', KT, 1, 128, 64, 2, 2, 1, 1, 1, 0, D4, (1,), (1, 1))
for H, W in ((3, 5), (9, 1)):
    E('nc32', K3, 2, 128, 64, H, W, 1, 1, 1, 0, PS, (1,), (1,))
    E('nc32', K3, 2, 48, 48, H, W, 1, 1, 1, 0, N2, (1,), (1,))
    E('nc32', K1, 2, 128, 64, H, W, 1, 1, 1, 0, P4, (1,), (1,))
    E('nc32', K1, 2, 48, 48, H, W, 1, 1, 1, 0, N2, (1,), (1,))
E('nc32', KT, 2, 128, 64, 3, 5, 1, 1, 1, 0, D4, (1,), (1, 1))          # (T2: 32 cells are its full stage)
E('nc32', KT, 2, 48, 48, 9, 1, 1, 1, 1, 0, N2, (1,), (1,))
E('ragged', K3, 1, 128, 64, 3, 32, 1, 1, 0, 0, PS, (2,), (1,))
E('ragged', K3, 1, 64, 64, 3, 32, 2, 1, 0, 0, N2, (1, 1), (1,))
E('ragged', K1, 1, 128, 64, 3, 32, 1, 1, 1, 0, P4, (2,), (1,))
E('ragged', K1, 1, 64, 64, 3, 32, 2, 1, 1, 0, N2, (1, 1), (1,))
E('ragged', KT, 1, 128, 64, 2, 40, 1, 1, 1, 0, D4, (4,), (1, 1))

# ---- the four K-split cases of the 2-wave tile, (Co, Ci) -> kstride: both sides two 32-channel blocks 1, the plain side one block 2,
# the shifted side one block 2, both one block 4 - and channel tails inside them.  3x3 in full on the scalar path (NC = 32: 16 k-steps) and
# on the vec path; T2 (the plain operand is x: the roles swap) and 1x1 two each.  (32, 32) on a 1x1 image: one k-step for a kstride of 4,
# three waves have no step and first_operands clamps.  (32 x 32 at an even batch is the split sample-pair form: B = 1.)
for (Co, Ci), k in (((64, 64), 1), ((32, 64), 2), ((64, 32), 2), ((32, 32), 4), ((48, 48), 1), ((33, 20), 2), ((8, 8), 4)):
    E('ksplit', K3, 1, Co, Ci, 4, 8, 1, 1, 1, 0, N2, (1,), (k,))
    E('ksplit', K3, 1, Co, Ci, 4, 32, 2, 1, int(Co % 64 != 0 or Ci % 64 != 0), 0, N2V, (1, 1), (k,))
E('ksplit', KT, 1, 32, 64, 4, 8, 1, 1, 1, 0, N2, (1,), (2,))
E('ksplit', KT, 1, 64, 32, 1, 32, 1, 1, 0, 0, N2V, (1,), (2,))
E('ksplit', KT, 1, 32, 32, 2, 32, 2, 1, 1, 0, N2V, (1, 1), (4,))
E('ksplit', KT, 1, 33, 20, 4, 8, 1, 1, 1, 0, N2, (1,), (2,))
E('ksplit', K1, 1, 64, 32, 4, 8, 1, 1, 1, 0, N2, (1,), (2,))
E('ksplit', K1, 1, 8, 8, 2, 32, 1, 1, 1, 0, N2V, (1,), (4,))
E('ksplit', K1, 1, 32, 64, 4, 32, 2, 1, 1, 0, N2V, (1, 1), (2,))
E('nks1', K3, 1, 32, 32, 1, 1, 1, 1, 1, 0, N2, (1,), (4,))
E('nks1', KT, 1, 32, 32, 1, 1, 1, 1, 1, 0, N2, (1,), (4,))
E('nks1', K1, 1, 8, 8, 1, 1, 1, 1, 1, 0, N2, (1,), (4,))
E('nks2', K3, 1, 32, 32, 2, 2, 1, 1, 1, 0, N2, (1,), (4,))             # two k-steps for four shares

# ---- channel tails on the 4-wave tile: 130 x 66 on the scalar path, 96 x 72 on vec (above), grid y and z > 1 on both sides
E('tail', K3, 2, 130, 66, 5, 3, 1, 1, 1, 0, PS, (1,), (1, 1, 1, 1))
E('tail', KT, 2, 130, 66, 5, 3, 1, 1, 1, 0, D4, (1,), (1, 1, 1))
E('tail', K1, 2, 130, 66, 5, 3, 1, 1, 1, 0, P4, (1,), (1, 1, 1, 1))
E('grid', K3, 1, 256, 128, 2, 32, 1, 1, 0, 0, PV, (1,), (1, 1, 1, 1))
E('grid', KT, 1, 128, 256, 1, 32, 1, 1, 0, 0, T4V, (1,), (1, 1, 1, 1))
E('grid', K1, 1, 256, 128, 2, 32, 1, 1, 0, 0, P4V, (1,), (1, 1, 1, 1))

# ---- groups: NB samples share a slab, the tile index maps to (sample, tile).  NB = 2 and 4 under S = 1 and 2 on both paths (one tile per
# sample: the chunk boundaries fall between samples); two tiles per sample, NB = 2, S = 3: boundaries inside sample 0 and between the samples.
# Whole channel blocks, as te_wgrad_group_plan requires - but for one vec entry with NB = 2 and a channel tail: the ABI accepts it, the tail
# lanes of sample 0 read sample 1's first channels (in range of the group's descriptor) into accumulator rows that are never stored.
for NB, S, trips in ((2, 1, (2,)), (2, 2, (1, 1)), (4, 1, (4,)), (4, 2, (2, 2))):
    E('group', K3, 4, 128, 128, 2, 32, S, NB, 0, 0, PV, trips, (1, 1))
    E('group', K3, 4, 128, 128, 4, 4, S, NB, 1, 0, PS, trips, (1, 1))
E('group', K3, 2, 128, 128, 4, 32, 3, 2, 0, 0, PV, (1, 1, 2), (1, 1))
E('group', K3, 2, 128, 128, 16, 8, 3, 2, 1, 0, PS, (1, 1, 2), (1, 1))
E('group', K3, 4, 64, 64, 2, 32, 1, 2, 0, 0, N2V, (2,), (1,))
E('group', KT, 4, 128, 128, 1, 32, 2, 4, 0, 0, T4V, (2, 2), (1, 1))
E('group', KT, 2, 128, 128, 2, 32, 3, 2, 0, 0, T4V, (1, 1, 2), (1, 1))
E('group', KT, 4, 128, 128, 4, 4, 1, 2, 1, 0, D4, (2,), (1, 1))
E('group', K1, 4, 128, 128, 2, 32, 2, 2, 0, 0, P4V, (1, 1), (1, 1))
E('group', K1, 2, 128, 128, 4, 32, 3, 2, 0, 0, P4V, (1, 1, 2), (1, 1))
E('group', K1, 4, 128, 128, 4, 4, 1, 4, 1, 0, P4, (4,), (1, 1))
E('grouptail', K3, 2, 96, 72, 2, 32, 1, 2, 1, 0, PV, (2,), (1, 1))

# ---- batches of per-sample slabs with several chunks of several tiles: block x -> (sample, chunk); each sample is compared with its own launch
E('batch', K3, 3, 128, 64, 4, 64, 3, 1, 0, 0, PV, (1, 1, 2), (1,))
E('batch', K3, 3, 48, 48, 4, 40, 3, 1, 1, 0, N2, (1, 1, 2), (1,))
E('batch', KT, 3, 96, 72, 2, 64, 3, 1, 1, 0, T4V, (1, 1, 2), (1, 1))
E('batch', K1, 3, 64, 32, 6, 64, 2, 1, 1, 0, N2V, (3, 3), (2,))

# ---- g and x 4 bytes off 16-byte alignment, one vec-eligible shape per kind under the default switch: the split kernel would take the
# aligned launch, the misaligned one runs this kernel on its scalar path.  Each has its aligned vec twin above (switch off).
E('off', K3, 1, 128, 64, 2, 32, 1, 1, 1, 4, PS, (1,), (1,))
E('off', K3, 1, 64, 64, 2, 32, 1, 1, 1, 4, N2, (1,), (1,))
E('off', KT, 1, 128, 64, 1, 32, 1, 1, 1, 4, D4, (1,), (1, 1))
E('off', K1, 1, 128, 128, 2, 32, 1, 1, 1, 4, P4, (1,), (1, 1))
# (four tiles in two columns: the halo columns of both sides and the tile walk on the scalar path, bit for bit against the S = 1 vec entries above)
E('off', K3, 1, 128, 64, 4, 64, 1, 1, 1, 4, PS, (4,), (1,))
E('off', KT, 1, 128, 64, 2, 64, 1, 1, 1, 4, D4, (4,), (1, 1))
E('off', K1, 1, 128, 64, 4, 64, 1, 1, 1, 4, P4, (4,), (1,))

# ---- LARGE: one full-size layer per kind at batch 2 under S = 4, what the planner gives these layers at batch 32 (at batch 2 it gives one
# chunk per tile): chunks of 16, 8 and 16 tiles
E('large', K3, 2, 128, 128, 64, 64, 4, 1, 0, 0, PV, (16,) * 4, (1, 1))
E('large', KT, 2, 128, 128, 32, 32, 4, 1, 0, 0, T4V, (8,) * 4, (1, 1))
E('large', K1, 2, 256, 128, 64, 64, 4, 1, 0, 0, P4V, (16,) * 4, (1, 1, 1, 1))

BY_NAME = {e.name: e for e in TABLE}
LARGE = tuple(e.name for e in TABLE if e.name.endswith('_large'))
assert len(LARGE) == 3


# ------------------------------------------------------------------------------------------------ the query
class switch:
    """the split-bf16 switch set to `on` inside the block, restored after it"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = _lib.wgrad_split(self.on)

    def __exit__(self, *exc):
        _lib.wgrad_split(self.old)


def g_shape(e):
    return (e.B, e.Co, 2 * e.H + 1, 2 * e.W + 1) if e.kind == KT else (e.B, e.Co, e.H, e.W)


def answer(e):
    """te_wgrad_form's answer for an entry under the entry's switch: the dict of _lib.WGRAD_FORM, or the negative code of a refusal"""
    with switch(e.sw):
        return _lib.wgrad_form(KIND[e.kind], e.B, e.Co, e.Ci, e.H, e.W, e.S, e.NB, e.off, e.off)


def facts(e, f):
    """(trips, ks, nks) of a launch from the query's answer: tiles of every chunk, the kstride of every channel block by the kernel's
    rule, and the k-steps of a stage"""
    n_tiles = f['tiles_x'] * f['tiles_y'] * e.NB
    trips = tuple(n_tiles * (s + 1) // e.S - n_tiles * s // e.S for s in range(e.S))
    gshift = e.kind == KT
    pch, qch = 32 * f['nwp'], 64
    pC, qC = (e.Ci, e.Co) if gshift else (e.Co, e.Ci)
    ks = []
    for y in range(f['grid_y']):
        for z in range(f['grid_z']):
            co0, ci0 = y * (qch if gshift else pch), z * (pch if gshift else qch)
            pc0, qc0 = (ci0, co0) if gshift else (co0, ci0)
            k = 1
            if f['nwp'] == 2:
                nPB, nQB = (min(pch, pC - pc0) + 31) >> 5, (min(qch, qC - qc0) + 31) >> 5
                k = (1 if nPB >= 2 else 2) * (1 if nQB >= 2 else 2)
            ks.append(k)
    return trips, tuple(ks), f['TW'] * f['TH'] // (4 if f['wino'] else 2)


def check(e):
    """raise AssertionError naming the entry when the library does not plan the declared key and per-block facts for it; returns the answer"""
    f = answer(e)
    assert not isinstance(f, int), f'{e.name}: te_wgrad_form refuses ({f})'
    assert f['form6'] == 0, f'{e.name}: the launch goes to split kernel {f["form6"]}, not to the fp32 kernel'
    got = (e.kind, f['nwp'], f['wino'], f['vec'], f['db'])
    assert got == e.key, f'{e.name}: expected (kind, nwp, wino, vec, db) = {e.key}, the library plans {got}'
    trips, ks, _ = facts(e, f)
    assert trips == e.trips, f'{e.name}: expected tiles per chunk {e.trips}, the launch walks {trips}'
    assert ks == e.ks, f'{e.name}: expected kstride per channel block {e.ks}, the launch has {ks}'
    assert f['grid_x'] == e.B // e.NB * e.S
    return f


# ------------------------------------------------------------------------------------------------ operands and the fp64 reference
def operands(e, device='cpu', seed=None, off=None):
    """(g, x) of an entry from a CPU generator seeded by the entry's place in the table, `off` bytes (the entry's by default) past
    16-byte alignment.  The values depend on the seed and the dims only: an entry and its 4-bytes-off twin hold the same numbers."""
    gen = torch.Generator().manual_seed(3000 + TABLE.index(e) if seed is None else seed)
    off = e.off if off is None else off
    return [off16(torch.randn(shape, generator=gen, dtype=torch.float32), off, device) for shape in (g_shape(e), (e.B, e.Ci, e.H, e.W))]


def chunk_masks(e, f, device):
    """[G, S, NB, H, W] fp64: 1 on the cells that chunk s of a group walks - the tiles [n_tiles s / S, n_tiles (s + 1) / S) of the group's
    NB samples, tile index -> (sample, tile row, tile column), from the query's tile geometry"""
    tiles_1 = f['tiles_x'] * f['tiles_y']
    n_tiles = tiles_1 * e.NB
    m = torch.zeros(e.S, e.NB, e.H, e.W, dtype=torch.float64)
    for s in range(e.S):
        for t in range(n_tiles * s // e.S, n_tiles * (s + 1) // e.S):
            bb, tn = divmod(t, tiles_1)
            ty, tx = divmod(tn, f['tiles_x'])
            m[s, bb, ty * f['TH']:(ty + 1) * f['TH'], tx * f['TW']:(tx + 1) * f['TW']] = 1.0
    assert float(m.sum()) == e.NB * e.H * e.W and float(m.sum(0).max()) == 1.0          # the chunks partition the group's cells
    return m.to(device)[None].expand(e.B // e.NB, -1, -1, -1, -1)


def _taps(e, gm, xg):
    """the nine (or one) tap sums [G, S, Co, Ci, taps] of cell-masked operands: gm [G, S, NB, Co, Hg, Wg], xg [G, S or 1, NB, Ci, H, W]"""
    H, W = e.H, e.W
    out = []
    if e.kind == K1:
        return torch.einsum('gsbohw,gsbihw->gsoi', gm, xg.expand(-1, gm.shape[1], -1, -1, -1, -1))[..., None]
    if e.kind == K3:
        xp = torch.nn.functional.pad(xg, (1, 1, 1, 1)).expand(-1, gm.shape[1], -1, -1, -1, -1)
        for ky in range(3):
            for kx in range(3):
                out.append(torch.einsum('gsbohw,gsbihw->gsoi', gm, xp[..., ky:ky + H, kx:kx + W]))
    else:
        ge = gm.expand(-1, xg.shape[1], -1, -1, -1, -1)
        for ky in range(3):
            for kx in range(3):
                out.append(torch.einsum('gsbohw,gsbihw->gsoi', ge[..., ky:ky + 2 * H:2, kx:kx + 2 * W:2], xg))
    return torch.stack(out, -1)


def reference(e, f, g, x):
    """(ref, bound), both [B / NB, S, Co, Ci, taps] fp64: every slab on its own from slices, restricted to its chunk by zeroing the
    cell-side operand (g for 3x3 and 1x1, x for T2) outside the chunk's tiles, and the elementwise bound (module docstring of
    tests/test_gpu_wgrad_forms.py)"""
    G, NB = e.B // e.NB, e.NB
    m = chunk_masks(e, f, g.device)                                             # [G, S, NB, H, W]
    g6 = g.double().view(G, 1, NB, *g.shape[1:])
    x6 = x.double().view(G, 1, NB, *x.shape[1:])
    if e.kind == KT:
        x6 = x6 * m[:, :, :, None]
    else:
        g6 = g6 * m[:, :, :, None]
    ref = _taps(e, g6, x6)
    trips, ks, _ = facts(e, f)
    gshift = e.kind == KT
    rows, cols = (64, 32 * f['nwp']) if gshift else (32 * f['nwp'], 64)         # channels of a block along co and ci
    kmap = torch.tensor(ks, dtype=torch.float64, device=g.device).view(f['grid_y'], f['grid_z'])
    kmap = kmap.repeat_interleave(rows, 0).repeat_interleave(cols, 1)[:e.Co, :e.Ci]
    if not f['wino']:
        n = m.sum((2, 3, 4)).view(G, e.S, 1, 1, 1)                              # products of the chunk that can be nonzero
        return ref, (n + kmap[None, None, :, :, None]) * U * _taps(e, g6.abs(), x6.abs())
    # pair form: the operands of the four accumulators of a tap row, absolute values expanded through the pre-additions
    H, W, J = e.H, e.W, (e.W + 1) // 2
    ga = torch.nn.functional.pad(g6.abs(), (0, 2 * J - W))
    g0, g1 = ga[..., 0::2], ga[..., 1::2]
    ua = (g0, g0 + g1, g0 + g1, g1)
    xa = torch.nn.functional.pad(x6.abs(), (1, 2 * J + 2 - (W + 1), 1, 1)).expand(-1, e.S, -1, -1, -1, -1)
    pairs = torch.nn.functional.pad(m, (0, 2 * J - W)).view(G, e.S, NB, H, J, 2).amax(-1).sum((2, 3, 4)).view(G, e.S, 1, 1)
    bound = []
    for ky in range(3):
        ek = [xa[..., ky:ky + H, k:k + 2 * J:2] for k in range(4)]
        ta = (ek[0] + ek[2], ek[1] + ek[2], ek[2] + ek[1], ek[1] + ek[3])
        A = [torch.einsum('gsbohw,gsbihw->gsoi', ua[c], ta[c]) for c in range(4)]
        mid = 0.5 * (A[1] + A[2])
        step = (pairs + 2 + 3) * U          # pairs accumulation steps, one rounding each in u_c and t_c, the fold's three roundings
        bound += [step * (A[0] + mid), step * mid, step * (mid + A[3])]
    return ref, torch.stack(bound, -1)


if __name__ == '__main__':
    by_key = {}
    for e in TABLE:
        by_key.setdefault(e.key, []).append(e.name)
    for k in sorted(by_key):
        print(k, ':', ', '.join(by_key[k]))
    print(f'{len(by_key)} keys, {len(TABLE)} entries')

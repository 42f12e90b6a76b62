"""Form table of the FIR kernels (csrc/upfirdn2d.hip): the smallest shapes that land on every instantiation of blur44_kernel<MODE, D, EXT>,
on fir_tile_kernel<2,1,4,4>, <1,2,4,4> and <1,1,4,4,AG>, on fir_direct_kernel and fir_direct_any_kernel<half | double>, and on the
situations inside a form where such a kernel can go wrong.

Which kernel a launch runs is decided by the op, the taps, up / down, minor and the row width (fir_route, actgrad_blur44); the blur44
instantiation by D = (-pad_x0) & 3 and by the +1 rule (a size 64 n + 1 / 32 n + 1 gets no tile of its own for its last column / row: the
last tile's edge lanes filter a fifth column / third row, EXT).  te_fir_form (include/te_hip.h) reports the plan that the launch itself
makes and then dispatches on.  An entry names the op, (planes, H, W), the four pads (px0, px1, py0, py1), the taps, the epilogue (bias with
size_b, act), the operands' offset from 16-byte alignment in bytes, the dtype, and what it is expected to land on: a key of two parts.

  key = (kernel, MODE, D, EXT), the query's own words (MODE, D, EXT are 0 off blur44).
  sit = (ext, tiles, s, pads), worked out by plain arithmetic from the shape and the query's tile size and tile counts (situations()):
    ext    'none', 'x', 'y', 'both': tiles_x tile_w < out_w / tiles_y tile_h < out_h, the last tile column / row has one output more
    tiles  '1x1', 'x' (two or more tiles along x only), 'y', '2x2' (two or more along both); '-' where the direct kernel runs
    s      (-in_w) & 3: the columns by which the 16-byte group that straddles the right edge is loaded further left and shifted (place())
    pads   'plain', or the classes that apply joined by '+': 'crop0' (pad_x0 or pad_y0 < 0: crop left / top), 'crop1' (pad_x1 or
           pad_y1 < 0: crop right / bottom), 'wide' (a pad >= 4: a whole 16-byte group left of the image, or as much above / beside it)
The expected key is data; what a launch does comes from the query.  tests/test_fir_forms_cpu.py holds the table to the query, asserts the
coverage that REQUIRED lists, and sweeps the query for kernels without an entry; tests/test_gpu_fir_forms.py runs every entry after
re-asserting its key.  The list of keys with their entries: `python tests/fir_forms.py`.

Every entry has pads that differ between the axes, H != W and taps that are neither symmetric nor equal to their transpose or to either
flip: K44 = outer((1, 2, 3, 5), (2, 1, 4, 3)), unnormalised and exact in every format (K32, K33 for the direct kernel).  11 planes (one
sample of 11 channels: the blocks of plane groups 11 ... 15 have nothing to do) and, where there is a bias, size_b = 3 (mj % size_b
wraps); one entry per op has a single plane.  out = in + pad0 + pad1 - 3 for the blurs.

Operands (operands()): standard normals from synth.normal keyed by the entry's name, made on the CPU so that the CPU test sees the numbers
of the GPU test; or the EXACT set - integers in [-4, 4], a saved output of random signs, alpha = 0.5, scale = 1 - under which every staged
value, output and per-tile sum is a multiple of 1/2 far below 2^23 in magnitude, so fp32 computes it exactly in any summation order.

reference() is the fp64 restatement (tests/fir_restated.py) with the elementwise bound of tests/test_gpu_loop_trips.py, and
partial[plane][tile] restated from the query's tile size: tile (bx, by) of te_blur_actgrad_f32 owns the INPUT rows
[by th - pad_y0, (by + 1) th - pad_y0) and columns [bx tw - pad_x0, (bx + 1) tw - pad_x0), the last tile of a row also everything up to the
right edge and the last tile of a column everything down to the bottom edge; tile (bx, by) of te_blur_gradact_f32 sums its OUTPUTS, rows
[by th, (by + 1) th) and columns [bx tw, (bx + 1) tw), the last tiles to the edges (the ext column and row included).  A per-tile sum of Lt
terms is held to (Lt + 1) u sum |terms|; where the terms are outputs their own bounds are added.

The four instruments (shared by the CPU test, which proves them on a model with planted defects, and the GPU test):
  elementwise()  |got - fp64| <= bound for every output element, through fp64_check.within (kink cap KINK_CAP)
  exact()        under the EXACT operands the output and every partial[plane][tile] equal the fp64 restatement bit for bit
  per_tile()     partial[plane][tile] within its own bound under the normal operands
  guards()       output and partial live in fp64_check.guarded buffers: every element written, nothing else touched
"""
import os
import sys
from dataclasses import dataclass

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import fp64_check  # noqa: E402
from fir_restated import fir64, fir_bound, slope64  # noqa: E402
from fp64_check import ALPHA, SCALE, U, U32, kink_keep, off16, where64  # noqa: E402
from transeditor_amd import _lib, synth  # noqa: E402

UP, AG, GA = 'upfirdn2d', 'blur_actgrad', 'blur_gradact'
MODE_OF = {UP: 0, AG: 1, GA: 2}
TAPS = {'k44': torch.outer(torch.tensor((1., 2., 3., 5.), dtype=torch.float64), torch.tensor((2., 1., 4., 3.), dtype=torch.float64)),
        'k32': torch.outer(torch.tensor((1., 2., 3.), dtype=torch.float64), torch.tensor((2., 1.), dtype=torch.float64)),
        'k33': torch.outer(torch.tensor((1., 2., 3.), dtype=torch.float64), torch.tensor((2., 1., 4.), dtype=torch.float64))}
for _k in TAPS.values():        # neither symmetric nor equal to the transpose or to either flip
    assert all(_k.shape != v.shape or not torch.equal(_k, v) for v in (_k.t(), _k.flip(0), _k.flip(1), _k.flip(0, 1)))
SIZE_B = 3


@dataclass(frozen=True)
class Entry:
    name: str
    op: str              # UP (te_upfirdn2d_f32 / _f16 / _f64), AG (te_blur_actgrad_f32), GA (te_blur_gradact_f32)
    planes: int
    H: int
    W: int
    pad: tuple           # (px0, px1, py0, py1)
    taps: str            # a name of TAPS
    bias: int            # size_b, 0: no bias
    act: int             # 0 or 3 (leaky ReLU)
    off: int             # bytes by which the operands miss 16-byte alignment
    dtype: str
    up: tuple            # (x, y)
    down: tuple
    minor: int
    key: tuple           # (kernel, MODE, D, EXT)
    sit: tuple           # (ext, tiles, s, pads)
    data: str            # suffix of the synth keys: an entry that lands on the kink gets another one

    def __hash__(self):
        return hash(self.name)


TABLE = []


def E(tag, op, planes, H, W, pad, key, sit, *, taps='k44', bias=0, act=0, off=0, dtype='float32', up=(1, 1), down=(1, 1), minor=1, data=''):
    name = f'{op}_{planes}x{H}x{W}_p' + '.'.join(str(p) for p in pad) + (f'_b{bias}' if bias else '') + ('_act' if act else '') + \
        (f'_off{off}' if off else '') + ('' if dtype == 'float32' else '_' + dtype) + f'_{tag}'
    assert all(t.name != name for t in TABLE), name
    assert H != W and pad[:2] != pad[2:], name
    TABLE.append(Entry(name, op, planes, H, W, tuple(pad), taps, bias, act, off, dtype, tuple(up), tuple(down), minor, tuple(key), tuple(sit), data))


def B(tag, op, planes, out_hw, pad, key, sit, **kw):
    """a blur entry by its OUTPUT size: in = out + 3 - pad0 - pad1"""
    E(tag, op, planes, out_hw[0] + 3 - pad[2] - pad[3], out_hw[1] + 3 - pad[0] - pad[1], pad, key, sit, **kw)


BL = 'blur44'
# pads by D = (-pad_x0) & 3, different on the two axes, all plain
PD = {0: (0, 3, 2, 1), 1: (3, 0, 1, 2), 2: (2, 1, 1, 2), 3: (1, 2, 2, 1)}
EPI = {0: dict(), 1: dict(bias=SIZE_B), 2: dict(act=3), 3: dict(bias=SIZE_B, act=3)}      # MODE 0's epilogues, one per D below

# ---- blur44 MODE 0, one tile of 9 x W outputs: every (D, s), rows of 5, 6, 7 and 8 floats, the four epilogues
for D in range(4):
    for W, s in ((8, 0), (7, 1), (6, 2), (5, 3)):
        B('ds', UP, 11, (9, W), PD[D], (BL, 0, D, 0), ('none', '1x1', s, 'plain'), **EPI[D])
# ---- the same under MODE 1 and MODE 2: every D, every s
for op in (AG, GA):
    for D, (W, s) in enumerate(((8, 0), (7, 1), (6, 2), (5, 3))):
        B('ds', op, 11, (9, W), PD[D], (BL, MODE_OF[op], D, 0), ('none', '1x1', s, 'plain'))
# ---- rows of 4 floats (the first group is the straddling one and needs no shift), of 5 and 7 under another D, and a single plane
for op in (UP, AG, GA):
    m = MODE_OF[op]
    B('w4', op, 11, (6, 4), PD[2], (BL, m, 2, 0), ('none', '1x1', 0, 'plain'), **(EPI[3] if op == UP else {}))
    B('w5', op, 11, (7, 5), PD[1], (BL, m, 1, 0), ('none', '1x1', 3, 'plain'))
    B('w6', op, 11, (7, 6), PD[3], (BL, m, 3, 0), ('none', '1x1', 2, 'plain'))
    B('w7', op, 11, (5, 7), PD[0], (BL, m, 0, 0), ('none', '1x1', 1, 'plain'))
    B('one', op, 1, (6, 7), PD[2], (BL, m, 2, 0), ('none', '1x1', 1, 'plain'), **(EPI[3] if op == UP else {}))
# ---- the +1 rule on one tile: ext x only, y only, both, and 32 x 64 where it just does not apply; every (MODE, D, EXT = 1)
for op in (UP, AG, GA):
    m = MODE_OF[op]
    B('ext', op, 11, (20, 65), PD[(0 + m) % 4], (BL, m, (0 + m) % 4, 1), ('x', '1x1', 3, 'plain'), **(EPI[1] if op == UP else {}))
    B('ext', op, 11, (33, 40), PD[(1 + m) % 4], (BL, m, (1 + m) % 4, 1), ('y', '1x1', 0, 'plain'))
    B('ext', op, 11, (33, 65), PD[(2 + m) % 4], (BL, m, (2 + m) % 4, 1), ('both', '1x1', 3, 'plain'), **(EPI[3] if op == UP else {}))
    B('full', op, 11, (32, 64), PD[(3 + m) % 4], (BL, m, (3 + m) % 4, 0), ('none', '1x1', 0, 'plain'), **(EPI[2] if op == UP else {}))
# ---- more than one tile: just past a tile on both axes (the second tile 2 wide and 2 high), along x only, along y only, 40 x 70, and
# 65 x 129: 2 x 2 tiles with both ext flags, the halo owned by the last tile
for op in (UP, AG, GA):
    m = MODE_OF[op]
    B('past', op, 11, (34, 66), PD[(1 + m) % 4], (BL, m, (1 + m) % 4, 0), ('none', '2x2', 2, 'plain'), **(EPI[3] if op == UP else {}))
    B('tx', op, 11, (20, 66), PD[(0 + m) % 4], (BL, m, (0 + m) % 4, 0), ('none', 'x', 2, 'plain'))
    B('ty', op, 11, (34, 40), PD[(3 + m) % 4], (BL, m, (3 + m) % 4, 0), ('none', 'y', 0, 'plain'))
    B('four', op, 11, (40, 70), PD[(2 + m) % 4], (BL, m, (2 + m) % 4, 0), ('none', '2x2', 2, 'plain'), **(EPI[1] if op == UP else {}))
    # (data='.2': under the first key one of MODE 0's 92 235 elements sits on the kink)
    B('ext4', op, 11, (65, 129), PD[(3 + m) % 4], (BL, m, (3 + m) % 4, 1), ('both', '2x2', 3, 'plain'), **(dict(data='.2', **EPI[3]) if op == UP else {}))
    # ext on one axis with two tiles on the other
    B('extx_ty', op, 5, (34, 65), PD[(2 + m) % 4], (BL, m, (2 + m) % 4, 1), ('x', 'y', 3, 'plain'))
    B('exty_tx', op, 5, (33, 66), PD[(1 + m) % 4], (BL, m, (1 + m) % 4, 1), ('y', 'x', 2, 'plain'))
# ---- pad classes.  wide: a whole 16-byte group left of the image (pad_x0 = 4, 5) or five rows above it, on one tile and on four;
# crops (MODE 0 and 2): left, top, right, bottom on one tile, left + bottom on the 33 x 65 ext tile, top + right on four tiles
for op in (UP, AG, GA):
    m = MODE_OF[op]
    B('wide', op, 11, (7, 9), (4, 1, 2, 0), (BL, m, 0, 0), ('none', '1x1', 1, 'wide'), **(EPI[3] if op == UP else {}))
    B('wide', op, 11, (9, 6), (2, 1, 5, 0), (BL, m, 2, 0), ('none', '1x1', 2, 'wide'))
    B('wide4', op, 11, (40, 70), (5, 2, 1, 1), (BL, m, 3, 0), ('none', '2x2', 2, 'wide'))
for op in (UP, GA):
    m = MODE_OF[op]
    B('crop', op, 11, (10, 11), (-1, 2, 1, 2), (BL, m, 1, 0), ('none', '1x1', 3, 'crop0'), **(EPI[3] if op == UP else {}))
    B('crop', op, 11, (9, 12), (2, 1, -2, 3), (BL, m, 2, 0), ('none', '1x1', 0, 'crop0'))
    B('crop', op, 11, (10, 11), (2, -1, 1, 2), (BL, m, 2, 0), ('none', '1x1', 3, 'crop1'))
    B('crop', op, 11, (9, 12), (1, 2, 3, -1), (BL, m, 3, 0), ('none', '1x1', 0, 'crop1'), **(EPI[2] if op == UP else {}))
    B('cropext', op, 11, (33, 65), (-1, 2, 2, -1), (BL, m, 1, 1), ('both', '1x1', 1, 'crop0+crop1'))
    B('crop4', op, 11, (40, 70), (2, -2, -1, 1), (BL, m, 2, 0), ('none', '2x2', 3, 'crop0+crop1'))
# ---- operands 4, 8 and 12 bytes past a 16-byte boundary
for op in (UP, AG, GA):
    m = MODE_OF[op]
    B('off', op, 11, (33, 65), PD[2], (BL, m, 2, 1), ('both', '1x1', 3, 'plain'), off=4, **(EPI[3] if op == UP else {}))
    B('off', op, 11, (6, 7), PD[3], (BL, m, 3, 0), ('none', '1x1', 1, 'plain'), off=8)
    B('off', op, 11, (34, 66), PD[0], (BL, m, 0, 0), ('none', '2x2', 2, 'plain'), off=12)

# ---- fir_tile_kernel<2,1,4,4> (up 2: out = 2 in + pad0 + pad1 - 3) and <1,2,4,4> (down 2: out = (in + pad0 + pad1 - 4) / 2 + 1):
# out widths 64, 65 and 70, 2 x 2 tiles of 16 x 64, pad_x0 even and odd (the phase of the first tap), a negative pad (floor division of a
# negative mid), with and without the epilogue
U2, D2 = ('tile_up2', 0, 0, 0), ('tile_down2', 0, 0, 0)
E('w64', UP, 11, 4, 32, (2, 1, 1, 2), U2, ('none', '1x1', 0, 'plain'), up=(2, 2))
E('w65', UP, 11, 5, 32, (1, 3, 2, 1), U2, ('none', 'x', 0, 'plain'), up=(2, 2), **EPI[3])
E('w70', UP, 11, 9, 35, (2, 1, 1, 2), U2, ('none', '2x2', 1, 'plain'), up=(2, 2))
E('neg', UP, 11, 6, 34, (-1, 2, 2, -1), U2, ('none', 'x', 2, 'crop0+crop1'), up=(2, 2), **EPI[3])
E('one', UP, 1, 9, 33, (3, 1, -1, 2), U2, ('none', 'x', 3, 'crop0'), up=(2, 2), **EPI[1])
E('w64', UP, 11, 8, 128, (1, 1, 2, 0), D2, ('none', '1x1', 0, 'plain'), down=(2, 2))
E('w65', UP, 11, 10, 130, (2, 1, 1, 1), D2, ('none', 'x', 2, 'plain'), down=(2, 2), **EPI[3])
E('w70', UP, 11, 35, 139, (1, 2, 0, 1), D2, ('none', '2x2', 1, 'plain'), down=(2, 2))
E('neg', UP, 11, 12, 132, (-1, 2, 2, -1), D2, ('none', 'x', 0, 'crop0+crop1'), down=(2, 2), **EPI[3])
E('one', UP, 1, 9, 131, (2, -1, 1, 2), D2, ('none', 'x', 1, 'crop1'), down=(2, 2), **EPI[2])
# ---- fir_tile_kernel<1,1,4,4,AG>: te_blur_actgrad_f32 on rows of 1, 2 and 3 floats; in_h 5 (one tile) and 20 (two tile rows share ownership)
TA = ('tile_ag', 0, 0, 0)
for W, pad in ((1, (2, 1, 1, 2)), (2, (1, 2, 2, 1)), (3, (3, 1, 0, 3))):
    E('ag', AG, 11, 5, W, pad, TA, ('none', '1x1', (-W) & 3, 'plain'))
    E('ag', AG, 11, 20, W, pad, TA, ('none', 'y', (-W) & 3, 'plain'))
E('one', AG, 1, 20, 3, (1, 2, 2, 1), TA, ('none', 'y', 1, 'plain'))
# ---- fir_direct_kernel: minor 2, up_x != up_y, kh != kw; 4 x 4 taps on rows of 3 floats; the epilogue; one f16 and one f64 entry
DI = ('direct', 0, 0, 0)
E('minor2', UP, 11, 5, 7, (1, 1, 2, 0), DI, ('none', '-', 1, 'plain'), taps='k32', up=(2, 1), down=(1, 2), minor=2)
E('k33', UP, 11, 6, 5, (2, 0, 1, 1), DI, ('none', '-', 3, 'plain'), taps='k33', up=(1, 2), **EPI[3])
E('w3', UP, 11, 6, 3, (2, 1, 1, 2), DI, ('none', '-', 1, 'plain'), **EPI[3])
E('w3', UP, 1, 5, 3, (-1, 4, 2, 1), DI, ('none', '-', 1, 'crop0+wide'), **EPI[1])
E('half', UP, 11, 6, 7, (1, 1, 2, 0), DI, ('none', '-', 1, 'plain'), taps='k32', up=(2, 1), dtype='float16')
E('double', UP, 11, 5, 8, (2, 0, 1, 1), DI, ('none', '-', 0, 'plain'), taps='k33', down=(1, 2), dtype='float64')

BY_NAME = {e.name: e for e in TABLE}

# ---- the coverage asked of the table, as (description, predicate) over entries; tests/test_fir_forms_cpu.py asserts each has an entry
_blur = lambda e, m: e.key[0] == BL and e.key[1] == m                                        # noqa: E731
REQUIRED = []
for m in range(3):
    for D in range(4):
        for X in range(2):
            REQUIRED.append((f'blur44<{m},{D},{X}>', lambda e, m=m, D=D, X=X: e.key == (BL, m, D, X)))
    for s in range(4):
        REQUIRED.append((f'MODE {m} s = {s}', lambda e, m=m, s=s: _blur(e, m) and e.sit[2] == s))
        REQUIRED.append((f'MODE {m} in_w = {4 + s}', lambda e, m=m, s=s: _blur(e, m) and e.W == 4 + s))
    for x in ('none', 'x', 'y', 'both'):
        REQUIRED.append((f'MODE {m} ext {x}', lambda e, m=m, x=x: _blur(e, m) and e.sit[0] == x))
    for t in ('1x1', 'x', 'y', '2x2'):
        REQUIRED.append((f'MODE {m} tiles {t}', lambda e, m=m, t=t: _blur(e, m) and e.sit[1] == t))
    for c in ('plain', 'wide') + (() if m == 1 else ('crop0', 'crop1')):
        REQUIRED.append((f'MODE {m} pads {c}', lambda e, m=m, c=c: _blur(e, m) and c in e.sit[3].split('+')))
    REQUIRED.append((f'MODE {m} off 16-byte alignment', lambda e, m=m: _blur(e, m) and e.off in (4, 8, 12)))
for D in range(4):
    for s in range(4):
        REQUIRED.append((f'MODE 0 (D, s) = ({D}, {s})', lambda e, D=D, s=s: _blur(e, 0) and e.key[2] == D and e.sit[2] == s))
for b, a in ((0, 0), (SIZE_B, 0), (0, 3), (SIZE_B, 3)):
    REQUIRED.append((f'MODE 0 epilogue bias {b} act {a}', lambda e, b=b, a=a: _blur(e, 0) and (e.bias, e.act) == (b, a)))
for op in (UP, AG, GA):
    REQUIRED.append((f'{op} single plane', lambda e, op=op: e.op == op and e.planes == 1))
for kern in ('tile_up2', 'tile_down2'):
    for ow in (64, 65, 70):
        REQUIRED.append((f'{kern} out width {ow}', lambda e, kern=kern, ow=ow: e.key[0] == kern and out_hw(e)[1] == ow))
    REQUIRED += [(f'{kern} 2x2 tiles', lambda e, kern=kern: e.key[0] == kern and e.sit[1] == '2x2'),
                 (f'{kern} pad_x0 even', lambda e, kern=kern: e.key[0] == kern and e.pad[0] % 2 == 0),
                 (f'{kern} pad_x0 odd', lambda e, kern=kern: e.key[0] == kern and e.pad[0] % 2 == 1),
                 (f'{kern} negative pad', lambda e, kern=kern: e.key[0] == kern and min(e.pad) < 0),
                 (f'{kern} epilogue', lambda e, kern=kern: e.key[0] == kern and e.bias and e.act),
                 (f'{kern} no epilogue', lambda e, kern=kern: e.key[0] == kern and not e.bias and not e.act)]
for W in (1, 2, 3):
    for H in (5, 20):
        REQUIRED.append((f'tile_ag {H} x {W}', lambda e, W=W, H=H: e.key[0] == 'tile_ag' and (e.H, e.W) == (H, W)))
REQUIRED += [('direct minor 2', lambda e: e.key[0] == 'direct' and e.minor == 2),
             ('direct up_x != up_y', lambda e: e.key[0] == 'direct' and e.up[0] != e.up[1]),
             ('direct kh != kw', lambda e: e.key[0] == 'direct' and TAPS[e.taps].shape[0] != TAPS[e.taps].shape[1]),
             ('direct 3x3 taps', lambda e: e.key[0] == 'direct' and e.taps == 'k33'),
             ('direct 4x4 taps, in_w 3', lambda e: e.key[0] == 'direct' and e.taps == 'k44' and e.W == 3),
             ('direct epilogue', lambda e: e.key[0] == 'direct' and e.bias and e.act),
             ('direct f16', lambda e: e.key[0] == 'direct' and e.dtype == 'float16'),
             ('direct f64', lambda e: e.key[0] == 'direct' and e.dtype == 'float64')]


# ------------------------------------------------------------------------------------------------ the query
def out_hw(e):
    kh, kw = TAPS[e.taps].shape
    px0, px1, py0, py1 = e.pad
    return (e.H * e.up[1] + py0 + py1 - kh) // e.down[1] + 1, (e.W * e.up[0] + px0 + px1 - kw) // e.down[0] + 1


def answer(e):
    """te_fir_form's answer for an entry: the dict of _lib.FIR_FORM, or the negative code of a refusal"""
    kh, kw = TAPS[e.taps].shape
    return _lib.fir_form(e.op, e.planes, e.H, e.W, e.pad, kh, kw, e.up, e.down, e.minor)


def key_of(f):
    return (f['kernel'], f['mode'], f['D'], f['ext'])


def situations(e, f):
    """(ext, tiles, s, pads) of an entry by plain arithmetic from its shape and the query's tile size and tile counts (module docstring)"""
    oh, ow = out_hw(e)
    if f['kernel'] == 'direct':
        ext, tiles = 'none', '-'
    else:
        ext = {(0, 0): 'none', (1, 0): 'x', (0, 1): 'y', (1, 1): 'both'}[(int(f['tiles_x'] * f['tile_w'] < ow), int(f['tiles_y'] * f['tile_h'] < oh))]
        tiles = {(0, 0): '1x1', (1, 0): 'x', (0, 1): 'y', (1, 1): '2x2'}[(int(f['tiles_x'] >= 2), int(f['tiles_y'] >= 2))]
    px0, px1, py0, py1 = e.pad
    pads = [c for c, on in (('crop0', px0 < 0 or py0 < 0), ('crop1', px1 < 0 or py1 < 0), ('wide', max(e.pad) >= 4)) if on]
    return ext, tiles, (-e.W) & 3, '+'.join(pads) or 'plain'


def loop_name(f):
    """the kernel instantiation of a plan as csrc/upfirdn2d.hip spells it"""
    return {'direct': 'fir_direct_kernel', 'blur44': f'blur44_kernel<{f["mode"]},{f["D"]},{"true" if f["ext"] else "false"}>',
            'tile_up2': 'fir_tile_kernel<2,1,4,4>', 'tile_down2': 'fir_tile_kernel<1,2,4,4>', 'tile_ag': 'fir_tile_kernel<1,1,4,4,AG>'}[f['kernel']]


def check(e):
    """raise AssertionError naming the entry when the library does not plan the declared key and situations for it; returns the answer"""
    f = answer(e)
    assert not isinstance(f, int), f'{e.name}: te_fir_form refuses ({f})'
    assert key_of(f) == e.key, f'{e.name}: expected (kernel, MODE, D, EXT) = {e.key}, the library plans {key_of(f)}'
    sit = situations(e, f)
    assert sit == e.sit, f'{e.name}: expected (ext, tiles, s, pads) = {e.sit}, the shape and the query\'s tiles give {sit}'
    assert f['threads'] == 256
    if f['kernel'] == 'direct':
        assert all(f[k] == 0 for k in ('ext_x', 'ext_y', 'tile_h', 'tile_w', 'tiles_x', 'tiles_y', 'zgroups')) and f['grid_x'] > 0, (e.name, f)
        return f
    oh, ow = out_hw(e)
    assert (f['tile_h'], f['tile_w']) == ((32, 64) if f['kernel'] == 'blur44' else (16, 64)), (e.name, f)
    assert (f['ext_x'], f['ext_y']) == (int(sit[0] in ('x', 'both')), int(sit[0] in ('y', 'both'))), (e.name, f)
    assert f['ext'] == int(sit[0] != 'none'), (e.name, f)
    # the tiles (with the ext column / row) cover the output exactly
    assert f['tiles_x'] * f['tile_w'] + f['ext_x'] >= ow > (f['tiles_x'] - 1) * f['tile_w'], (e.name, f)
    assert f['tiles_y'] * f['tile_h'] + f['ext_y'] >= oh > (f['tiles_y'] - 1) * f['tile_h'], (e.name, f)
    assert f['grid_x'] == f['zgroups'] * f['tiles_x'] * f['tiles_y']
    assert f['zgroups'] == (16 if e.planes > 8 else 8) and e.planes in (1, 5, 11), f'{e.name}: {e.planes} planes in {f["zgroups"]} plane groups'
    return f


# ------------------------------------------------------------------------------------------------ operands
@dataclass
class Operands:
    x: torch.Tensor          # the filtered operand: x [planes, H, W(, minor)] of UP, g [planes, H, W] of AG and GA
    k: torch.Tensor
    b: torch.Tensor          # [SIZE_B] or None
    ref: torch.Tensor        # the saved output of AG [planes, H, W] and GA [planes, out_h, out_w], else None
    alpha: float
    scale: float


def _ints(shape, key):
    return (synth.normal(shape, key) * 2.5).round().clamp(-4, 4)


def operands(e, exact=False, device='cpu'):
    """the entry's operands on `device`, e.off bytes past 16-byte alignment: normals keyed by the entry's name, or the EXACT set"""
    dt = getattr(torch, e.dtype)
    key = f'fir_forms.{e.name}{e.data}.'
    oh, ow = out_hw(e)
    shape = (e.planes, e.H, e.W) + ((e.minor,) if e.minor > 1 else ())
    make = _ints if exact else synth.normal
    x = make(shape, key + 'x').to(dt)
    b = make((e.bias,), key + 'b').to(dt) if e.bias else None
    ref = None
    if e.op != UP:
        ref = synth.normal((e.planes, e.H, e.W) if e.op == AG else (e.planes, oh, ow), key + 'ref')
        if exact:
            ref = torch.where(ref > 0, 1.0, -1.0)
    put = lambda t: None if t is None else off16(t.contiguous(), e.off, device)  # noqa: E731
    alpha, scale = (0.5, 1.0) if exact else (ALPHA, SCALE)
    return Operands(put(x), off16(TAPS[e.taps].to(dt), 0, device), put(b), put(ref), alpha, scale)


# ------------------------------------------------------------------------------------------------ the fp64 reference
def owned(e, f):
    """[(tile index, rows, columns)]: the slices of the plane that tile by tiles_x + bx sums into partial[plane][tile] - input rows and
    columns for AG, output rows and columns for GA (module docstring), restated from the query's tile size and tile counts"""
    th, tw, nx, ny = f['tile_h'], f['tile_w'], f['tiles_x'], f['tiles_y']
    px0, _, py0, _ = e.pad
    nrow, ncol = (e.H, e.W) if e.op == AG else out_hw(e)
    oy, ox = (py0, px0) if e.op == AG else (0, 0)
    spans = []
    for by in range(ny):
        for bx in range(nx):
            r0, r1 = max(by * th - oy, 0), nrow if by == ny - 1 else min(max((by + 1) * th - oy, 0), nrow)
            c0, c1 = max(bx * tw - ox, 0), ncol if bx == nx - 1 else min(max((bx + 1) * tw - ox, 0), ncol)
            spans.append((by * nx + bx, slice(r0, r1), slice(c0, c1)))
    assert sum((r.stop - r.start) * (c.stop - c.start) for _, r, c in spans) == nrow * ncol, f'{e.name}: the tiles do not partition the plane'
    return spans


def _tile_sums(e, f, terms, extra=None):
    """(partial, bound) [planes, tiles] of the per-tile sums of `terms` [planes, rows, columns]: (Lt + 1) u sum |terms| (+ the sum of
    `extra`, the terms' own bounds)"""
    spans = owned(e, f)
    part = terms.new_zeros(e.planes, len(spans))
    bound = terms.new_zeros(e.planes, len(spans))
    for t, r, c in spans:
        Lt = (r.stop - r.start) * (c.stop - c.start)
        part[:, t] = terms[:, r, c].sum(dim=(1, 2))
        bound[:, t] = (Lt + 1) * U32 * terms[:, r, c].abs().sum(dim=(1, 2))
        if extra is not None:
            bound[:, t] += extra[:, r, c].sum(dim=(1, 2))
    return part, bound


def slopes(ops):
    """(scale, alpha * scale) as the two fused blur backward passes form them in fp32"""
    return float(np.float32(ops.scale)), float(np.float32(ops.alpha) * np.float32(ops.scale))


def reference(e, f, ops):
    """dict(y, bound, keep, part, pbound) in fp64 on the operands' device: the output with its elementwise bound and, under an activation,
    the elements off the kink; partial[plane][tile] with its bound (None for te_upfirdn2d)"""
    dt = getattr(torch, e.dtype)
    k = ops.k.double()
    a32 = float(np.float32(ops.alpha))
    s32, as32 = slopes(ops)
    x = ops.x.double()
    if e.op == UP:
        if e.minor > 1:
            x = x.permute(0, 3, 1, 2)
        fir = fir64(x, k, e.up, e.down, e.pad)
        mag = fir64(x.abs(), k, e.up, e.down, e.pad)
        T = -(-k.shape[0] // e.up[1]) * -(-k.shape[1] // e.up[0])             # taps that meet a sample (zero insertion skips the others)
        keep = None
        if e.bias or e.act:
            pre = fir
            if e.bias:
                bm = ops.b.double()[torch.arange(e.planes, device=x.device) % e.bias][:, None, None]
                pre, mag = fir + bm, mag + bm.abs()
            gain = where64(pre > 0, s32, a32 * s32) if e.act else torch.full_like(pre, s32)
            y = pre * gain
            if e.act:
                keep = kink_keep(pre, (T + 2) * U32 * mag)
            bound = fir_bound(mag, y, T, gain)
        else:
            y = fir
            acc = U32 if dt == torch.float16 else U[dt]                       # half accumulates in fp32 and rounds once at the store
            bound = (T + 2) * acc * mag + U[dt] * y.abs() + (2.0 ** -25 if dt == torch.float16 else 0.0)
            if dt == torch.float64:
                bound = 2 * bound                                             # the fp64 reference has the same round-off as the kernel
        if e.minor > 1:
            y, bound = y.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()
        return dict(y=y, bound=bound, keep=keep, part=None, pbound=None)
    if e.op == AG:
        s = x * slope64(ops.ref, s32, as32)
        y = fir64(s, k, pad=e.pad)
        bound = fir_bound(fir64(s.abs(), k, pad=e.pad), y, 16)
        part, pbound = _tile_sums(e, f, s)
    else:
        c = slope64(ops.ref, s32, as32)
        y = fir64(x, k, pad=e.pad) * c
        bound = fir_bound(fir64(x.abs(), k, pad=e.pad), y, 16, c)
        part, pbound = _tile_sums(e, f, y, bound)
    return dict(y=y, bound=bound, keep=None, part=part, pbound=pbound)


def kink_share(e, f):
    """the share of an act entry's elements that the elementwise check leaves out, from the fp64 reference of its normal operands"""
    keep = reference(e, f, operands(e))['keep']
    return 0.0 if keep is None else 1.0 - float(keep.double().mean())


# ------------------------------------------------------------------------------------------------ launches and instruments
@dataclass
class Run:
    ybuf: torch.Tensor       # fp32 words of the guarded output buffer
    y: torch.Tensor          # the output inside it, in the entry's dtype and shape
    pbuf: torch.Tensor       # the same for partial [planes, tiles]; None for te_upfirdn2d
    part: torch.Tensor


def y_shape(e):
    oh, ow = out_hw(e)
    return (e.planes, oh, ow) + ((e.minor,) if e.minor > 1 else ())


def buffers(e, f, device):
    """a Run of guarded, pattern-filled buffers for the entry's launch.  The guard pattern is fp32: an f16 / f64 output is a view of fp32
    words (an even number of halves), so for these two dtypes `guards` sees an unwritten element only where a whole word stayed"""
    dt = getattr(torch, e.dtype)
    n = int(np.prod(y_shape(e)))
    words = n * torch.empty((), dtype=dt).element_size()
    assert words % 4 == 0
    ybuf, inner = fp64_check.guarded(words // 4, device)
    y = inner.view(dt).view(y_shape(e))
    if e.op == UP:
        return Run(ybuf, y, None, None)
    tiles = f['tiles_x'] * f['tiles_y']
    pbuf, pin = fp64_check.guarded(e.planes * tiles, device)
    return Run(ybuf, y, pbuf, pin.view(e.planes, tiles))


def elementwise(e, R, run, results=None):
    """instrument 1"""
    return fp64_check.within(e.name, 'y', run.y, R['y'], R['bound'], R['keep'], results=results)


def exact(e, Rx, run):
    """instrument 2: under the EXACT operands the bits of the fp64 restatement, output and partial[plane][tile]"""
    assert float(Rx['y'].abs().max()) < 2.0 ** 23 and bool((Rx['y'] * 2 == (Rx['y'] * 2).round()).all())
    bad = run.y.double().to(Rx['y'].device) != Rx['y']
    assert not bool(bad.any()), f'{e.name}: {int(bad.sum())} output elements differ from the exact result, first at {bad.nonzero()[0].tolist()}'
    if Rx['part'] is not None:
        assert float(Rx['part'].abs().max()) < 2.0 ** 23
        bad = run.part.double().to(Rx['part'].device) != Rx['part']
        assert not bool(bad.any()), (f'{e.name}: partial[plane][tile] differs from the exact sum of the tile at (plane, tile) = '
                                     f'{bad.nonzero()[0].tolist()}: {float(run.part[tuple(bad.nonzero()[0])])} for {float(Rx["part"][tuple(bad.nonzero()[0])])}')


def per_tile(e, R, run, results=None):
    """instrument 3"""
    if R['part'] is not None:
        return fp64_check.within(e.name, 'partial', run.part, R['part'], R['pbound'], results=results)


def guards(e, run):
    """instrument 4: every element of the output and of partial written, nothing around them touched"""
    for what, buf, t in (('the output', run.ybuf, run.y), ('partial', run.pbuf, run.part)):
        if buf is not None:
            n = buf.numel() - 2 * fp64_check.GUARD
            fp64_check.untouched(e.name, what, buf, n, torch.ones(n, dtype=torch.bool, device=buf.device))


if __name__ == '__main__':
    by_key = {}
    for e in TABLE:
        by_key.setdefault((e.key, e.sit), []).append(e.name)
    for k in sorted(by_key):
        print(k, ':', ', '.join(by_key[k]))
    print(f'{len(set(e.key for e in TABLE))} kernels (kernel, MODE, D, EXT), {len(by_key)} keys, {len(TABLE)} entries')

"""Form table of the split-bf16 family: the smallest shapes that land on every kernel, grid rule and epilogue of TE_CONV_3X3W6
(csrc/wino6.hip), TE_CONV_S2S6 (s2s6.hip), TE_CONV_T2S6 (t2s6.hip: body and edge kernel), TE_CONV_1X1S6 (p1s6.hip) and of the split
weight-gradient kernels (wgrad6.hip).

Which kernel a launch runs is decided by the shape, by launch constants and by the test and tool hooks te_conv_wino6_form,
te_conv_wino6_tiles_per_block, te_conv_s2s6_form, te_conv_t2s6_form, te_wgrad_t2_wide and te_wgrad_split_bf16.  te_conv_split_form
(include/te_hip.h) reports the plan that a forward launch itself makes and then dispatches on, te_wgrad6_form the kernel of a
weight-gradient launch.  An entry names a kind, a shape, the operands that matter to the form, the hook values it runs under, and what
it is expected to land on.  The expected key is data; what a launch does comes from the query.  tests/test_split6_forms_cpu.py checks
the table against the queries and sweeps them for keys the table lacks; tests/test_gpu_split6_forms.py runs every entry against fp64
after re-asserting its key.  `python tests/split6_forms.py` lists the keys with their entries.

Forward key: (kind, 'q' two-image | 'pp' ping-pong, pair16, isc, edge CT, scratch); `expect` holds the further answers an entry is
about (ntiles, idle blocks, tiles per run, runs per XCD, M blocks).  Weight-gradient key: (kind, te_wgrad6_form name).

Shapes are (B, K, M, H, W), H x W the low-resolution size.  Constraints that set the smallest shapes: `pair16` needs
(B / 2) (H / 8) (M / 64) >= 128 blocks (te_conv_wino6_supported), 1X1S6 needs B (H W / 256) (M / 128) >= 128; the automatic tile walk
takes runs of two tiles only from 256 two-image blocks of two tiles up, 16.8 M outputs: the one LARGE entry.
"""
import contextlib
import os
import sys
from dataclasses import dataclass, field

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import conv_routes as cr  # noqa: E402
import split6_restated as sr  # noqa: E402
from transeditor_amd import _lib  # noqa: E402

W6, S2, T2, P1 = 'w6', 's2', 't2', 'p1'
KIND = {W6: _lib.CONV_3X3W6, S2: _lib.CONV_S2S6, T2: _lib.CONV_T2S6, P1: _lib.CONV_1X1S6}
YARD = {W6: _lib.CONV_3X3, S2: _lib.CONV_S2, T2: _lib.CONV_T2, P1: _lib.CONV_1X1}       # the fp32 kernel of the same operation
OP = {W6: '3x3', S2: 'down', T2: 'up', P1: '1x1'}                                         # conv_routes.ref_conv
PACKS = {W6: (_lib.PACK_W6FWD, _lib.PACK_W6DGRAD), S2: (_lib.PACK_S6FWD, _lib.PACK_S6SWAP), T2: (_lib.PACK_T6FWD, _lib.PACK_T6SWAP),
         P1: (_lib.PACK_P6FWD, _lib.PACK_P6DGRAD)}
YARD_PACKS = {W6: (_lib.PACK_FWD, _lib.PACK_DGRAD), S2: (_lib.PACK_FWD, _lib.PACK_SWAP), T2: (_lib.PACK_FWD, _lib.PACK_SWAP),
              P1: (_lib.PACK_FWD, _lib.PACK_DGRAD)}
HOOKS = {'wino6_form': _lib.wino6_form, 'wino6_tiles_per_block': _lib.wino6_tiles_per_block, 's2s6_form': _lib.s2s6_form,
         't2s6_form': _lib.t2s6_form, 'wgrad_t2_wide': _lib.wgrad_t2_wide, 'wgrad_split': _lib.wgrad_split}
FORM_HOOK = {W6: 'wino6_form', S2: 's2s6_form', T2: 't2s6_form'}
PP, Q = {W6: 1, S2: 0, T2: 0}, {W6: 3, S2: 2, T2: 2}       # hook values: the ping-pong form, the two-image form wherever M % 128 == 0


@contextlib.contextmanager
def hooks(values):
    """the hooks named in `values` ({name: value} or a tuple of pairs) set for the duration, every hook of the family restored after it"""
    saved = {k: fn(-1) for k, fn in HOOKS.items()}
    try:
        for k, v in dict(values).items():
            HOOKS[k](v)
            assert HOOKS[k](-1) == v, (k, v)
        yield
    finally:
        for k, v in saved.items():
            HOOKS[k](v)
        assert {k: fn(-1) for k, fn in HOOKS.items()} == saved


@dataclass(frozen=True)
class Fwd:
    name: str
    kind: str
    shape: tuple         # (B, K, M, H, W)
    isc: int             # style scales (and demodulation scales) given
    epi: str             # 'none', 'res', 'both' (residual + mask)
    act: int
    adj: int             # 1: fed from the adjoint pack (W6DGRAD, S6SWAP, T6SWAP, P6DGRAD) of the adjoint weight
    hooks: tuple         # ((hook name, value), ...)
    scratch: int         # T2S6: the column scratch is handed over
    key: tuple
    expect: dict = field(default_factory=dict)

    def __hash__(self):
        return hash(self.name)


@dataclass(frozen=True)
class Wg:
    name: str
    kind: str            # '3x3', 't2', '1x1'
    B: int
    Co: int
    Ci: int
    H: int
    W: int
    S: int
    NB: int
    hooks: tuple
    key: tuple           # (kind, te_wgrad6_form name)

    def __hash__(self):
        return hash(self.name)


FWD, WG = [], []
LARGE = []


def F(kind, tag, shape, form, isc, act=0, epi='none', adj=0, tpb=None, scratch=1, pair16=0, large=False, **expect):
    """form: 'pp' / 'q' (the hook value that forces it) or 'auto' (the default hook values); lands=: the kernel it is expected to run where that differs"""
    hk = []
    landed = expect.pop('lands', form)
    if kind in FORM_HOOK and form != 'auto':
        hk.append((FORM_HOOK[kind], PP[kind] if form == 'pp' else Q[kind]))
    if tpb is not None:
        hk.append(('wino6_tiles_per_block', tpb))
    B, K, M, H, W = shape
    key = (kind, landed, pair16, isc if kind != P1 else 0, (4 if H >= 64 and W >= 64 else 2) if kind == T2 else 0, scratch if kind == T2 else 0)
    name = (f'{kind}_{landed}' + ('_pair16' if pair16 else '') + ('_isc' if isc else '') + (f'_{epi}' if epi != 'none' else '') + (f'_act{act}' if act else '') +
            ('_adj' if adj else '') + ('_noscr' if kind == T2 and not scratch else '') + f'_{B}x{K}x{M}x{H}x{W}_{tag}')
    assert all(e.name != name for e in FWD), name
    e = Fwd(name, kind, shape, isc, epi, act, adj, tuple(hk), scratch if kind == T2 else 0, key, expect)
    FWD.append(e)
    if large:
        LARGE.append(name)
    return e


# ---- TE_CONV_3X3W6.  Tiles are 8 rows x 32 columns; a one-tile image is all edge, 56 x 96 and 80 x 96 have interior tiles.
for isc in (0, 1):
    F(W6, 'tile1', (1, 32, 64, 8, 32), 'pp', isc, act=3, ntiles=1, idle=7, mblocks=1)
    F(W6, 'tiles4', (1, 32, 64, 16, 64), 'pp', isc, act=4, ntiles=4, idle=4)
    F(W6, 'm192', (1, 32, 192, 8, 32), 'pp', isc, epi='res', ntiles=1, mblocks=3, idle=21)
    F(W6, 'k160', (2, 160, 64, 8, 32), 'pp', isc, epi='both', act=3, ntiles=2)
    F(W6, 'interior', (1, 32, 64, 56, 96), 'pp', isc, ntiles=21, idle=3)
    F(W6, 'adj', (1, 32, 64, 16, 64), 'pp', isc, adj=1, act=3, ntiles=4)
    F(W6, 'm128', (1, 32, 128, 8, 32), 'pp', isc, act=3, mblocks=2)
    # W == 16 at an even batch, from 128 blocks up: two samples side by side; the ping-pong kernel only, whatever the hook says
    F(W6, 'pair16', (16, 32, 512, 16, 16), 'auto', isc, act=3, pair16=1, lands='pp', ntiles=16, mblocks=8, idle=0)
    F(W6, 'pair16', (16, 32, 512, 16, 16), 'q', isc, epi='res', pair16=1, lands='pp', ntiles=16, mblocks=8)
    # the two-image kernel: a tile per block, then runs of at most 2, 3 and 4 tiles.  30 tiles: XCDs of 3 and 4 tiles - runs of (1, 2) and
    # (2, 2) under 2, of 3 and 4 under 4; 21 tiles: XCDs of 2 and 3 - one run each under 3; 5 tiles: three XCDs have no tile, their runs are empty
    F(W6, 'tile1', (1, 32, 128, 8, 32), 'q', isc, act=3, tpb=1, ntiles=1, idle=7, mblocks=1, lists=0, tpb_=1)
    F(W6, 'run2', (1, 32, 128, 80, 96), 'q', isc, act=4, tpb=2, ntiles=30, lists=2, idle=0)
    F(W6, 'run3', (1, 32, 128, 56, 96), 'q', isc, epi='res', tpb=3, ntiles=21, lists=1, idle=0)
    F(W6, 'run4', (1, 32, 128, 80, 96), 'q', isc, epi='both', act=3, tpb=4, ntiles=30, lists=1, idle=0)
    F(W6, 'run2short', (1, 32, 128, 40, 32), 'q', isc, tpb=2, ntiles=5, lists=1, idle=3)
    F(W6, 'auto1', (1, 32, 128, 56, 96), 'q', isc, act=3, tpb=0, ntiles=21, lists=0, tpb_=1)
    F(W6, 'k160', (1, 160, 256, 8, 32), 'q', isc, act=3, tpb=1, mblocks=2)
    F(W6, 'adj', (1, 32, 128, 16, 64), 'q', isc, adj=1, act=4, tpb=2, ntiles=4, lists=1, idle=4)
# the automatic walk choosing runs of two under the default hooks: 64 tiles x 8 blocks of 128 output channels = 256 runs of two
F(W6, 'auto2', (2, 32, 1024, 64, 128), 'auto', 1, act=3, lands='q', large=True, ntiles=64, mblocks=8, tpb_=2, lists=4, blocks=256, idle=0)

# ---- TE_CONV_S2S6.  Output tiles of 8 rows x 16 columns.
for isc in (0, 1):
    F(S2, 'tile1', (1, 32, 64, 8, 16), 'pp', isc, act=3, ntiles=1, idle=7)
    F(S2, 'tiles3', (3, 48, 128, 8, 16), 'pp', isc, act=4, ntiles=3, mblocks=2, idle=10)
    F(S2, 'm192', (1, 32, 192, 16, 32), 'pp', isc, epi='res', ntiles=4, mblocks=3)
    F(S2, 'k160', (1, 160, 64, 8, 16), 'pp', isc, epi='both', act=3)
    F(S2, 'adj', (1, 32, 64, 8, 32), 'pp', isc, adj=1, ntiles=2)
    F(S2, 'tile1', (1, 32, 128, 8, 16), 'q', isc, act=3, ntiles=1, mblocks=1, idle=7)
    F(S2, 'tiles3', (3, 48, 128, 8, 16), 'q', isc, act=4, ntiles=3, mblocks=1, idle=5)
    F(S2, 'm256', (1, 32, 256, 16, 32), 'q', isc, epi='res', ntiles=4, mblocks=2)
    F(S2, 'k160', (1, 160, 128, 8, 16), 'q', isc, epi='both', act=3)
    F(S2, 'adj', (1, 32, 128, 8, 32), 'q', isc, adj=1, ntiles=2)
    F(S2, 'm192', (1, 32, 192, 8, 16), 'q', isc, lands='pp', mblocks=3)          # M % 128 != 0: the ping-pong kernel under the two-image hook

# ---- TE_CONV_T2S6.  Body tiles of 8 x 16 cells; the edge kernel's CT is 4 from 64 x 64 cells up.  K = 48 and 96 end the edge kernel's
# 32-channel chunks on a 16-channel tail.
for isc in (0, 1):
    for scr in (1, 0):
        F(T2, 'tile1', (1, 32, 64, 8, 16), 'pp', isc, act=3, scratch=scr, ntiles=1, idle=7, edge_line_tiles=2)
        F(T2, 'tile1', (1, 32, 128, 8, 16), 'q', isc, act=4, scratch=scr, ntiles=1, mblocks=1)
        F(T2, 'ct4', (1, 32, 64, 64, 64), 'pp', isc, act=3, scratch=scr, ntiles=32, idle=0, edge_line_tiles=3)
        F(T2, 'ct4', (1, 32, 128, 64, 64), 'q', isc, scratch=scr, ntiles=32)
    F(T2, 'k48', (3, 48, 64, 8, 16), 'pp', isc, act=4, ntiles=3)
    F(T2, 'k96', (1, 96, 128, 16, 32), 'q', isc, act=3, ntiles=4)
    F(T2, 'adj', (2, 48, 64, 8, 32), 'pp', isc, adj=1, act=3)
    F(T2, 'adj', (2, 32, 128, 8, 16), 'q', isc, adj=1)
    F(T2, 'k96', (1, 96, 64, 64, 80), 'pp', isc, scratch=0, ntiles=40)

# ---- TE_CONV_1X1S6: one kernel (two-image), no scales, bias or activation.  Tiles of 256 pixels; 128 blocks at the least.
F(P1, 'tps1', (32, 64, 512, 16, 16), 'q', 0, ntiles=32, mblocks=4, blocks=128, idle=0)
F(P1, 'tps4', (8, 64, 512, 32, 32), 'q', 0, epi='res', ntiles=32, mblocks=4)
F(P1, 'm128', (8, 64, 128, 64, 64), 'q', 0, ntiles=128, mblocks=1)
F(P1, 'm256', (8, 192, 256, 32, 64), 'q', 0, epi='res', ntiles=64, mblocks=2)
F(P1, 'k192', (8, 192, 512, 32, 32), 'q', 0, ntiles=32)
F(P1, 'idle', (11, 64, 512, 32, 32), 'q', 0, ntiles=44, idle=16)
F(P1, 'adj', (8, 64, 512, 32, 32), 'q', 0, adj=1, ntiles=32)
F(P1, 'adj', (8, 128, 256, 32, 64), 'q', 0, adj=1, epi='res')
F(P1, 'k128', (8, 128, 512, 32, 32), 'q', 0, ntiles=32)


# ---- the weight gradients (csrc/wgrad6.hip), launched with an explicit S and NB.  A chunk walks cell columns of 32 (3x3) or 16 (T2, 1x1)
# cells: U = NB W / 32 (16) columns of H rows.  S = 1: everything; U % S == 0: whole columns; S % U == 0: a column's rows in S / U parts -
# the chunk boundary falls inside a tile column; otherwise the flattened (column, row) steps in S parts.
K3, KT, K1 = '3x3', 't2', '1x1'
WG_KIND = {K3: _lib.CONV_3X3, KT: _lib.CONV_T2, K1: _lib.CONV_1X1}
WG_COLS = {K3: 32, KT: 16, K1: 16}


def G(kind, tag, B, Co, Ci, H, W, S, NB, form, wide=None):
    hk = (('wgrad_split', 1),) + ((('wgrad_t2_wide', wide),) if wide is not None else ())
    name = f'wg{kind}_{form}_{B}x{Co}x{Ci}x{H}x{W}_s{S}' + (f'g{NB}' if NB > 1 else '') + f'_{tag}'
    assert all(e.name != name for e in WG), name
    e = Wg(name, kind, B, Co, Ci, H, W, S, NB, hk, (kind, form))
    WG.append(e)
    return e


G(K3, 'key', 1, 64, 64, 2, 32, 1, 1, 'w6')
G(K3, 'row1', 1, 64, 64, 1, 32, 1, 1, 'w6')
G(K3, 'rows3', 1, 64, 64, 3, 64, 4, 1, 'w6')               # U = 2, S = 4: each column's rows [0, 1) and [1, 3)
G(K3, 'steps', 1, 64, 64, 3, 64, 3, 1, 'w6')               # U = 2, S = 3: steps [0, 2), [2, 4), [4, 6) of (column, row)
G(K3, 'cols', 2, 64, 64, 2, 64, 2, 1, 'w6')                # U = 2, S = 2: whole columns
G(K3, 'blocks', 1, 192, 128, 2, 32, 1, 1, 'w6')            # three and two channel blocks
G(K3, 'group', 4, 64, 128, 2, 32, 1, 2, 'w6')
G(K3, 'group', 4, 64, 64, 3, 32, 2, 2, 'w6')
G(K3, 'pair', 2, 32, 32, 2, 32, 1, 1, 'w6pair')
G(K3, 'pair', 6, 32, 32, 3, 32, 2, 1, 'w6pair')            # U = 1, S = 2: rows [0, 1) and [1, 3)
G(KT, 'key', 1, 64, 128, 2, 16, 1, 1, 't2wide')
G(KT, 'row1', 1, 64, 128, 1, 16, 1, 1, 't2wide')
G(KT, 'blocks', 2, 128, 256, 3, 32, 4, 1, 't2wide')        # U = 2, S = 4
G(KT, 'group', 4, 64, 128, 1, 16, 1, 2, 't2wide')
G(KT, 'key', 1, 64, 64, 2, 16, 1, 1, 't2narrow')
G(KT, 'blocks', 1, 192, 192, 3, 32, 3, 1, 't2narrow')      # U = 2, S = 3; three channel blocks per side
G(KT, 'narrow', 1, 64, 128, 2, 16, 1, 1, 't2narrow', wide=0)
G(KT, 'narrow', 2, 128, 256, 3, 32, 4, 1, 't2narrow', wide=0)
G(KT, 'group', 4, 64, 64, 1, 16, 1, 2, 't2narrow')
G(KT, 'co96', 1, 96, 64, 2, 16, 1, 1, 't2masked')          # 32 valid channels in the last block of g ...
G(KT, 'ci96', 1, 64, 96, 3, 16, 2, 1, 't2masked')          # ... and of x
G(KT, 'co32', 2, 32, 64, 1, 32, 1, 1, 't2masked')
G(K1, 'key', 1, 128, 128, 2, 16, 1, 1, 'p1')
G(K1, 'row1', 1, 128, 128, 1, 16, 1, 1, 'p1')
G(K1, 'blocks', 2, 256, 128, 3, 32, 4, 1, 'p1')
G(K1, 'steps', 1, 128, 256, 3, 32, 3, 1, 'p1')
G(K1, 'group', 4, 128, 128, 2, 16, 1, 2, 'p1')

TABLE = FWD + WG
BY_NAME = {e.name: e for e in TABLE}
assert len(BY_NAME) == len(TABLE)


# ------------------------------------------------------------------------------------------------ the queries
def answer(e, hook_values=None, scratch=None):
    """the query's answer for an entry under its hooks (or under `hook_values` / `scratch` instead): the dict of _lib.CONV_SPLIT_FORM or
    the negative code of a refusal (forward kinds), the te_wgrad6_form name (weight gradients)"""
    with hooks(e.hooks if hook_values is None else hook_values):
        if isinstance(e, Wg):
            return _lib.wgrad6_form(WG_KIND[e.kind], e.B, e.Co, e.Ci, e.H, e.W, e.NB)
        return _lib.conv_split_form(KIND[e.kind], *e.shape, e.isc, e.scratch if scratch is None else scratch)


def fwd_key(kind, f):
    return (kind, 'q' if f['two_image'] else 'pp', f['pair16'], f['isc'], f['edge_ct'], f['scratch'])


def check(e, hook_values=None, scratch=None, key=None):
    """raise AssertionError naming the entry when the library does not plan the declared key (or `key`) for it; returns the answer"""
    f = answer(e, hook_values, scratch)
    want = e.key if key is None else key
    if isinstance(e, Wg):
        assert (e.kind, f) == want, f'{e.name}: expected {want}, te_wgrad6_form names {f}'
        return f
    assert not isinstance(f, int), f'{e.name}: te_conv_split_form refuses ({f})'
    assert fwd_key(e.kind, f) == want, f'{e.name}: expected {want}, the library plans {fwd_key(e.kind, f)}'
    if key is None:
        for k, v in e.expect.items():
            k = k.rstrip('_')
            assert f[k] == v, f'{e.name}: expected {k} = {v}, the library plans {f[k]}'
    return f


def twins(e):
    """[(what, hook values, scratch, key)]: the other launches of the same operands that the header promises give the same bits"""
    out = []
    if isinstance(e, Wg):
        if e.key[1] == 't2wide':
            out.append(('64 x 64 slabs', dict(e.hooks, wgrad_t2_wide=0), None, (e.kind, 't2narrow')))
        return out
    kind, landed, pair16, isc, ct, scr = e.key
    M = e.shape[2]
    if kind in FORM_HOOK and M % 128 == 0 and not pair16:
        other = 'pp' if landed == 'q' else 'q'
        hv = {FORM_HOOK[kind]: PP[kind] if other == 'pp' else Q[kind]}
        if kind == W6 and other == 'q':
            hv['wino6_tiles_per_block'] = 1
        out.append((other, hv, None, (kind, other, pair16, isc, ct, scr)))
    if kind == W6 and landed == 'q' and e.name not in LARGE:
        have = dict(e.hooks).get('wino6_tiles_per_block')
        for n in (1, 2, 3, 4):
            if n != have:
                out.append((f'tpb{n}', dict(e.hooks, wino6_tiles_per_block=n), None, e.key))
    if kind == T2:
        out.append(('scratch' if not scr else 'no scratch', dict(e.hooks), 1 - scr, (kind, landed, pair16, isc, ct, 1 - scr)))
    return out


# ------------------------------------------------------------------------------------------------ chunks of a weight-gradient launch
def chunk_masks(e):
    """[S, NB', H, W] fp64 on the CPU: 1 on the cells that chunk s of a sample group walks, by the rule of wg6_chunk / wg6_segment
    (csrc/wgrad6.hip).  NB' = NB, or 1 for the sample-pair form, whose chunks are per sample."""
    nb = 1 if e.key[1] == 'w6pair' else e.NB
    cols = WG_COLS[e.kind]
    tiles_x = e.W // cols
    U, H, S = nb * tiles_x, e.H, e.S
    m = torch.zeros(S, nb, H, e.W, dtype=torch.float64)

    def mark(s, t0, t1):
        for t in range(t0, t1):
            col, row = divmod(t, H)
            b, tx = divmod(col, tiles_x)
            m[s, b, row, tx * cols:(tx + 1) * cols] = 1.0

    for s in range(S):
        if U % S == 0:
            for k in range(U // S):
                mark(s, (s + k * S) * H, (s + k * S) * H + H)
        elif S % U == 0:
            u, r, R = s % U, s // U, S // U
            mark(s, u * H + H * r // R, u * H + H * (r + 1) // R)
        else:
            mark(s, U * H * s // S, U * H * (s + 1) // S)
    assert float(m.sum()) == nb * H * e.W and float(m.sum(0).max()) == 1.0          # the chunks partition the group's cells
    return m


# ------------------------------------------------------------------------------------------------ operands, fp64 reference, bound
WSCALE, MGAIN = 0.7, 0.6
BIAS_OFF = 3.0          # |bias| >= 3: the kink window is as wide as the worst-case bound, 6 L u S for the single-accumulator kinds


def operands(e, device='cpu'):
    """the entry's tensors from a CPU generator seeded by the entry's place in the table (the same values on every machine).
    Forward kinds: x, w [M, K, k, k] (the weight of the convolution as computed; an `adj` entry packs its adjoint), bias, isc, osc, res,
    mref (None where the entry has none); weight gradients: g, x."""
    gen = torch.Generator().manual_seed(7000 + TABLE.index(e))
    rn = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float32)
    if isinstance(e, Wg):
        gs = (e.B, e.Co, 2 * e.H + 1, 2 * e.W + 1) if e.kind == KT else (e.B, e.Co, e.H, e.W)
        return {k: v.to(device) for k, v in (('g', rn(*gs)), ('x', rn(e.B, e.Ci, e.H, e.W)))}
    B, K, M, H, W = e.shape
    ks = 1 if e.kind == P1 else 3
    op = OP[e.kind]
    o = {'x': rn(B, K, *cr.in_hw(op, H, W)), 'w': rn(M, K, ks, ks) / (K * ks * ks) ** 0.5, 'bias': None, 'isc': None, 'osc': None,
         'res': None, 'mref': None}
    if e.kind != P1:
        b = rn(M)
        o['bias'] = torch.sign(b) * (BIAS_OFF + 0.5 * b.abs())
    if e.isc:
        o['isc'] = 1 + 0.5 * rn(B, K)
        o['osc'] = (1 + 0.3 * rn(B, M)).abs() + 0.1
    out_shape = (B, M) + cr.out_hw(op, H, W)
    if e.epi in ('res', 'both'):
        o['res'] = rn(*out_shape)
    if e.epi == 'both':
        o['mref'] = rn(*out_shape)
    return {k: (v.to(device) if v is not None else None) for k, v in o.items()}


def packed(e, o, yard=False):
    """the packed weights of the entry's launch (yard: of the fp32 kernel of the same operation) - from the forward pack of o['w'], or,
    for an `adj` entry, from the adjoint pack of the weight whose data gradient this convolution is"""
    fwd, adj = (YARD_PACKS if yard else PACKS)[e.kind]
    if not e.adj:
        return _lib.conv_pack(o['w'], fwd, WSCALE)
    w = o['w'].flip(2, 3) if e.kind in (W6, P1) else o['w']            # (stride-1 kinds: taps flipped back; a 1x1 flip is the identity)
    return _lib.conv_pack(w.transpose(0, 1).contiguous(), adj, WSCALE)


def coefficient(e, like):
    """the multiple of u S in the elementwise bound (module docstring of tests/test_gpu_split6_forms.py), a tensor shaped `like`"""
    B, K, M, H, W = e.shape
    L = (1 if e.kind == P1 else 9) * K
    if e.kind == S2:
        c = L * (1 + 5 / 128) + 1 + 5.5
    elif e.kind == W6:
        c = 6 * 3 * K + 9.5
    else:
        c = 6 * L + 5.5
    coef = torch.full_like(like, c)
    if e.kind == T2:                                                  # the last row and column: the fp32 edge kernel
        coef[..., -1, :] = L + 8
        coef[..., :, -1] = L + 8
    return coef


def reference(e, o):
    """(y, bound, keep) in fp64 on the operands' device; keep is None without an activation"""
    from fp64_check import A32, S32, U32 as U, kink_keep, where64
    op = OP[e.kind]
    d = lambda t: t.double()
    x, w = d(o['x']), d(o['w']) * WSCALE
    if o['isc'] is not None:
        x = x * d(o['isc'])[:, :, None, None]
    osc = d(o['osc'])[:, :, None, None] if o['osc'] is not None else 1.0
    bias = d(o['bias'])[None, :, None, None] if o['bias'] is not None else 0.0
    pre = cr.ref_conv(op, x, w) * osc + bias
    S = (sr.abs_sum('wino_row', w, x) if e.kind == W6 else cr.ref_conv(op, x.abs(), w.abs())) * osc + (bias.abs() if o['bias'] is not None else 0.0)
    coef = coefficient(e, pre)
    g = torch.ones_like(pre)
    keep = None
    if e.act >= 3:
        gain = S32 if e.act == 3 else 1.0
        g = where64(pre > 0, gain, A32 * gain)
        keep = kink_keep(pre, coef * U * S)
    y = pre * g
    bound = coef * U * S * g + 2 * U * y.abs()
    if o['res'] is not None:
        y = y + d(o['res'])
        bound = bound + U * y.abs()
    if o['mref'] is not None:
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
        m = where64(d(o['mref']) > 0, f32(MGAIN), float(torch.tensor(0.2, dtype=torch.float32) * torch.tensor(MGAIN, dtype=torch.float32)))
        y = y * m
        bound = bound * m + U * y.abs()
    return y, bound, keep


def wg_reference(e, o):
    """(ref, bound), [B / NB', S, Co, Ci, taps] fp64 on the operands' device: torch.nn.grad.conv2d_weight of every sample group with the
    cell-side operand (g; x for T2) zeroed outside the chunk's cells, and the elementwise bound"""
    from fp64_check import U32 as U
    g, x = o['g'].double(), o['x'].double()
    m = chunk_masks(e).to(g.device)
    S, nb = m.shape[:2]
    taps = 1 if e.kind == K1 else 9
    refs, bounds = [], []
    for b0 in range(0, e.B, nb):
        for s in range(S):
            gb, xb = g[b0:b0 + nb], x[b0:b0 + nb]
            cells = m[s][:, None]
            n = float(m[s].sum())
            if e.kind == KT:
                xm = xb * cells
                wg = lambda gg, xx: torch.nn.grad.conv2d_weight(gg, (e.Ci, e.Co, 3, 3), xx, stride=2).transpose(0, 1).reshape(e.Co, e.Ci, 9)
                refs.append(wg(gb, xm))
                bounds.append((6 * n + 1.5) * U * wg(gb.abs(), xm.abs()))
            elif e.kind == K1:
                gm = gb * cells
                refs.append(torch.einsum('bohw,bihw->oi', gm, xb)[..., None])
                bounds.append((6 * n + 1.5) * U * torch.einsum('bohw,bihw->oi', gm.abs(), xb.abs())[..., None])
            else:
                gm = gb * cells
                refs.append(torch.nn.grad.conv2d_weight(xb, (e.Co, e.Ci, 3, 3), gm, padding=1).reshape(e.Co, e.Ci, 9))
                pairs = float(m[s].view(nb, e.H, e.W // 2, 2).amax(-1).sum())
                bounds.append((6 * pairs + 5.5) * U * sr.abs_sum('wg_pair', gm, xb))
    shape = (e.B // nb, S, e.Co, e.Ci, taps)
    return torch.stack(refs).view(shape), torch.stack(bounds).view(shape)


# ------------------------------------------------------------------------------------------------ the groups of the grouped instruments
def _ar(n):
    return torch.arange(n, dtype=torch.int64)


def run_place(f):
    """place of every tile in its block's run (two-image TE_CONV_3X3W6 in banded order): [ntiles] int64, zeros for a tile per block"""
    n, lists = f['ntiles'], f['lists']
    place = torch.zeros(n, dtype=torch.int64)
    if lists:
        for xcd in range(8):
            first, nb = xcd * n // 8, (xcd + 1) * n // 8 - xcd * n // 8
            for lq in range(lists):
                lo, hi = lq * nb // lists, (lq + 1) * nb // lists
                place[first + lo:first + hi] = _ar(hi - lo)
    return place


def groups(e, f):
    """{name: int64 labels broadcastable to the output}: the marginals of the kernel's own coordinates over which the grouped
    instruments are taken (f: the query's answer).  Negative labels belong to no group."""
    if isinstance(e, Wg):
        cb = 128 if e.key[1] in ('t2wide', 'p1') else 64
        cob = 128 if e.key[1] == 'p1' else 64
        taps = 1 if e.kind == K1 else 9
        G, S = e.B // (1 if e.key[1] == 'w6pair' else e.NB), e.S
        g = {'tap': _ar(taps).view(1, 1, 1, 1, taps), 'co': ((_ar(e.Co) % cob) // 32).view(1, 1, e.Co, 1, 1),
             'ci': ((_ar(e.Ci) % cb) // 32).view(1, 1, 1, e.Ci, 1), 'chunk': _ar(S).view(1, S, 1, 1, 1)}
        if e.key[1] == 'w6pair':
            g['sample parity'] = (_ar(G) % 2).view(G, 1, 1, 1, 1)
        return g
    B, K, M, H, W = e.shape
    Ho, Wo = cr.out_hw(OP[e.kind], H, W)
    row, col = _ar(Ho).view(1, 1, Ho, 1), _ar(Wo).view(1, 1, 1, Wo)
    g = {'m quarter': ((_ar(M) % 128) // 32).view(1, M, 1, 1), 'sample': _ar(B).view(B, 1, 1, 1)}
    if e.kind == W6:
        g['row % 8'] = row % 8
        g['col % 32'] = (col + 16 * (_ar(B).view(B, 1, 1, 1) % 2)) if f['pair16'] else col % 32
        border = torch.full((1, 1, H, W), -1, dtype=torch.int64)
        border[..., :, 0], border[..., :, -1], border[..., 0, :], border[..., -1, :] = 2, 3, 0, 1
        g['border'] = border
        if f['lists']:
            tx, ty = W // 32, H // 8
            tile = (_ar(B).view(B, 1, 1, 1) * ty + row // 8) * tx + col // 32
            g['run place'] = run_place(f)[tile]
    elif e.kind == S2:
        g['row % 8'], g['col % 16'] = row % 8, col % 16
    elif e.kind == T2:
        body = (row < 2 * H) & (col < 2 * W)
        neg = torch.full((1, 1, Ho, Wo), -1, dtype=torch.int64)
        g['parity'] = torch.where(body, 2 * (row % 2) + col % 2, neg)
        g['cell row % 8'] = torch.where(body, (row // 2) % 8 + 0 * col, neg)
        g['cell col % 16'] = torch.where(body, (col // 2) % 16 + 0 * row, neg)
        g['lines'] = torch.where(body, neg, torch.where(row == 2 * H, 0, 1) + 0 * col)
    else:
        pixel = row * W + col
        g['pixel 16s'], g['pixel % 16'], g['image'] = (pixel % 256) // 16, pixel % 16, ((_ar(M) % 128) // 64).view(1, M, 1, 1)
    return g


if __name__ == '__main__':
    by_key = {}
    for e in TABLE:
        by_key.setdefault(e.key, []).append(e.name)
    for k in sorted(by_key, key=str):
        print(k, ':', ', '.join(by_key[k]))
    print(f'{len(by_key)} keys, {len(TABLE)} entries')

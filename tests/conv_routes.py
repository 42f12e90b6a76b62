"""Route table of the convolution ops: which kernel every selector picks, for the smallest shapes that land on each route.

An entry names an op kind, a shape (B, K = input channels, M = output channels, H, W = LOW-resolution size), the module switches
it runs under and the routes it is expected to take:

* fwd / dgrad: the (pack kind, convolution kind) pairs of op/modconv.fwd_kinds / bwd_kinds ('3x3', 'up', 'down', modulated '1x1')
  or plain_1x1_kinds (op 'skip': the plain 1x1 product of the discriminator's ResBlock, whose shape is the skip branch's);
* wgrad: (te_wgrad_split_supported 0 / 1 / 2, kernel form, plan of the plain gradient).  Forms: 'w6' (3x3 dense), 'w6pair'
  (Co == Ci == 32, sample pairs), 't2wide' / 't2narrow' / 't2masked' (the transposed kind: 64 x 128 / 64 x 64 channel blocks /
  wgrad6t_kernel<true>'s channel tail), 'p1' (split 1x1), 'fp32' (the fp32 kernel).  Plan: 'group' (te_wgrad_group_plan
  NB > 1) or 'slabs' (per-sample slabs).

Plain data and host code: tests/test_conv_routes_cpu.py checks the table against the predicates without a GPU,
tests/test_gpu_conv_routes.py runs every entry against fp64.  in_hw, out_hw and ref_conv are the geometry and the fp64 reference of
an op kind, for that module and for tests/test_gpu_conv_forms.py.
"""
import contextlib
import ctypes as C
import itertools
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from transeditor_amd import _lib

PACK_NAMES = ('FWD', 'DGRAD', 'SWAP', 'WFWD', 'WDGRAD', 'W6FWD', 'W6DGRAD', 'S6FWD', 'S6SWAP', 'T6FWD', 'T6SWAP', 'P6FWD', 'P6DGRAD')
CONV_NAMES = ('3X3', 'T2', 'S2', '1X1', '3X3W', '3X3W6', 'S2S6', 'T2S6', '1X1S6')
assert [getattr(_lib, 'PACK_' + n) for n in PACK_NAMES] == list(range(len(PACK_NAMES)))
assert [getattr(_lib, 'CONV_' + n) for n in CONV_NAMES] == list(range(len(CONV_NAMES)))

WGRAD_FORMS = _lib.WGRAD6_FORMS       # te_wgrad6_form: 'fp32', 'w6', 'w6pair', 't2wide', 't2narrow', 't2masked', 'p1'
WGRAD_PLANS = ('group', 'slabs')

# every (pack, kind) pair the three selectors can return (the CPU test checks a sweep of the selectors against this set)
ALL_FWD = {('W6FWD', '3X3W6'), ('WFWD', '3X3W'), ('FWD', '3X3'), ('S6FWD', 'S2S6'), ('FWD', 'S2'), ('T6FWD', 'T2S6'), ('FWD', 'T2'),
           ('FWD', '1X1')}
ALL_DGRAD = {('W6DGRAD', '3X3W6'), ('WDGRAD', '3X3W'), ('DGRAD', '3X3'), ('T6SWAP', 'T2S6'), ('SWAP', 'T2'), ('S6SWAP', 'S2S6'),
             ('SWAP', 'S2'), ('DGRAD', '1X1')}
ALL_PLAIN_1X1 = {('P6FWD', '1X1S6'), ('FWD', '1X1'), ('P6DGRAD', '1X1S6'), ('DGRAD', '1X1')}

DEFAULT_SWITCHES = {'USE_WINOGRAD': True, 'split_bf16': True, 'USE_SPLIT_S2': True, 'USE_SPLIT_T2': True, 'USE_SPLIT_1X1': True,
                    'USE_CLOSED_MODCONV': True}


@dataclass(frozen=True)
class Route:
    name: str
    op: str                  # '3x3', 'up', 'down', '1x1' (modulated), 'skip' (plain 1x1)
    shape: tuple             # (B, K, M, H, W), H x W = low-resolution size
    fwd: tuple
    dgrad: tuple
    wgrad: tuple             # (split_supported, form, plan)
    switches: dict = field(default_factory=dict)

    def __hash__(self):
        return hash(self.name)


def R(name, op, shape, fwd, dgrad, wgrad, **switches):
    return Route(name, op, shape, tuple(fwd.split('/')), tuple(dgrad.split('/')), wgrad, switches)


ROUTES = [
    # ---- '3x3' forward: Winograd on the bf16 pipe (W % 32 == 0, 16-column pair form), fp32 Winograd, direct
    R('3x3_w6_dgrad_direct', '3x3', (2, 32, 64, 8, 32), 'W6FWD/3X3W6', 'DGRAD/3X3', (0, 'fp32', 'slabs')),        # mixed (dgrad M = 32)
    R('3x3_w6_both', '3x3', (1, 64, 64, 8, 32), 'W6FWD/3X3W6', 'W6DGRAD/3X3W6', (1, 'w6', 'slabs')),
    R('3x3_w6_pair16', '3x3', (8, 32, 512, 32, 16), 'W6FWD/3X3W6', 'DGRAD/3X3', (0, 'fp32', 'slabs')),           # just 128 blocks
    R('3x3_pair16_few_blocks', '3x3', (8, 32, 256, 32, 16), 'FWD/3X3', 'DGRAD/3X3', (0, 'fp32', 'slabs')),        # 64 blocks
    R('3x3_pair16_odd_batch', '3x3', (9, 32, 512, 32, 16), 'FWD/3X3', 'DGRAD/3X3', (0, 'fp32', 'slabs')),
    R('3x3_wino_k16', '3x3', (2, 16, 64, 8, 32), 'WFWD/3X3W', 'DGRAD/3X3', (0, 'fp32', 'slabs')),                  # K = 16: no W6
    R('3x3_wino_fwd', '3x3', (1, 8, 32, 16, 32), 'WFWD/3X3W', 'DGRAD/3X3', (0, 'fp32', 'slabs')),
    R('3x3_wino_dgrad', '3x3', (1, 32, 8, 16, 32), 'FWD/3X3', 'WDGRAD/3X3W', (0, 'fp32', 'slabs')),
    R('3x3_w6_dgrad_only', '3x3', (1, 64, 32, 8, 32), 'FWD/3X3', 'W6DGRAD/3X3W6', (0, 'fp32', 'slabs')),
    R('3x3_wino_both', '3x3', (1, 32, 32, 16, 32), 'WFWD/3X3W', 'WDGRAD/3X3W', (2, 'fp32', 'slabs')),           # odd B: pair falls back
    R('3x3_direct_ragged', '3x3', (2, 12, 10, 9, 9), 'FWD/3X3', 'DGRAD/3X3', (0, 'fp32', 'slabs')),
    R('3x3_m32', '3x3', (2, 32, 32, 8, 32), 'FWD/3X3', 'DGRAD/3X3', (2, 'w6pair', 'slabs')),                      # M = 32: no W6
    R('3x3_m32_odd_batch', '3x3', (3, 32, 32, 8, 32), 'FWD/3X3', 'DGRAD/3X3', (2, 'fp32', 'slabs')),
    R('3x3_h4', '3x3', (2, 32, 64, 4, 32), 'FWD/3X3', 'DGRAD/3X3', (0, 'fp32', 'slabs')),                        # H = 4: no W6
    R('3x3_w48', '3x3', (2, 32, 64, 8, 48), 'FWD/3X3', 'DGRAD/3X3', (0, 'fp32', 'slabs')),                       # W = 48: no W6
    R('3x3_w6_no_winograd', '3x3', (1, 64, 64, 8, 32), 'FWD/3X3', 'DGRAD/3X3', (1, 'w6', 'slabs'), USE_WINOGRAD=False),
    R('3x3_w6_split_off', '3x3', (1, 64, 64, 8, 32), 'WFWD/3X3W', 'WDGRAD/3X3W', (1, 'fp32', 'slabs'), split_bf16=False),
    R('3x3_group', '3x3', (16, 512, 512, 4, 4), 'FWD/3X3', 'DGRAD/3X3', (0, 'fp32', 'group')),
    # ---- 'down' (stride 2): S2S6 forward, T2S6 data gradient (USE_SPLIT_T2), fp32 S2 / T2
    R('down_s2s6_t2s6', 'down', (1, 64, 64, 8, 16), 'S6FWD/S2S6', 'T6SWAP/T2S6', (1, 't2narrow', 'slabs')),
    R('down_s2s6_dgrad_fp32', 'down', (1, 32, 64, 8, 16), 'S6FWD/S2S6', 'SWAP/T2', (1, 't2masked', 'slabs')),   # mixed (dgrad M = 32)
    R('down_fp32_dgrad_t2s6', 'down', (1, 64, 32, 8, 16), 'FWD/S2', 'T6SWAP/T2S6', (1, 't2masked', 'slabs')),   # mixed (fwd M = 32)
    R('down_fp32', 'down', (1, 8, 8, 4, 8), 'FWD/S2', 'SWAP/T2', (0, 'fp32', 'slabs')),
    R('down_k16', 'down', (1, 16, 64, 8, 16), 'FWD/S2', 'SWAP/T2', (0, 'fp32', 'slabs')),                        # K = 16
    R('down_h4', 'down', (1, 32, 64, 4, 16), 'FWD/S2', 'SWAP/T2', (1, 't2masked', 'slabs')),                     # H = 4
    R('down_w8', 'down', (1, 32, 64, 8, 8), 'FWD/S2', 'SWAP/T2', (0, 'fp32', 'slabs')),                          # W = 8
    R('down_t2_wide', 'down', (1, 64, 128, 8, 16), 'S6FWD/S2S6', 'T6SWAP/T2S6', (1, 't2wide', 'slabs')),
    R('down_split_s2_off', 'down', (1, 64, 64, 8, 16), 'FWD/S2', 'T6SWAP/T2S6', (1, 't2narrow', 'slabs'), USE_SPLIT_S2=False),
    R('down_split_t2_off', 'down', (1, 64, 64, 8, 16), 'S6FWD/S2S6', 'SWAP/T2', (1, 't2narrow', 'slabs'), USE_SPLIT_T2=False),
    R('down_split_off', 'down', (1, 64, 64, 8, 16), 'FWD/S2', 'SWAP/T2', (1, 'fp32', 'slabs'), split_bf16=False),
    R('down_group', 'down', (16, 512, 512, 2, 2), 'FWD/S2', 'SWAP/T2', (0, 'fp32', 'group')),
    # ---- 'up' (transposed stride 2): T2S6 (body + edge kernel) forward, S2S6 data gradient (USE_SPLIT_S2)
    R('up_t2s6_s2s6', 'up', (1, 64, 64, 8, 16), 'T6FWD/T2S6', 'S6SWAP/S2S6', (1, 't2narrow', 'slabs')),
    R('up_t2s6_dgrad_fp32', 'up', (1, 32, 64, 8, 16), 'T6FWD/T2S6', 'SWAP/S2', (1, 't2masked', 'slabs')),       # mixed
    R('up_t2_wide', 'up', (1, 128, 64, 8, 16), 'T6FWD/T2S6', 'S6SWAP/S2S6', (1, 't2wide', 'slabs')),
    R('up_fp32_dgrad_s2s6', 'up', (1, 64, 32, 8, 16), 'FWD/T2', 'S6SWAP/S2S6', (1, 't2masked', 'slabs')),       # mixed (fwd M = 32)
    R('up_fp32', 'up', (1, 8, 8, 4, 8), 'FWD/T2', 'SWAP/S2', (0, 'fp32', 'slabs')),
    R('up_w8', 'up', (1, 64, 64, 8, 8), 'FWD/T2', 'SWAP/S2', (0, 'fp32', 'slabs')),                              # W = 8
    R('up_split_off', 'up', (1, 64, 64, 8, 16), 'FWD/T2', 'SWAP/S2', (1, 'fp32', 'slabs'), split_bf16=False),
    # ---- USE_CLOSED_MODCONV off: the same kernels, reached through the chan_scale -> conv_core -> chan_scale composite under second_order()
    R('3x3_closed_off', '3x3', (1, 64, 64, 8, 32), 'W6FWD/3X3W6', 'W6DGRAD/3X3W6', (1, 'w6', 'slabs'), USE_CLOSED_MODCONV=False),
    R('up_closed_off', 'up', (1, 64, 64, 8, 16), 'T6FWD/T2S6', 'S6SWAP/S2S6', (1, 't2narrow', 'slabs'), USE_CLOSED_MODCONV=False),
    R('1x1_closed_off', '1x1', (2, 128, 128, 8, 16), 'FWD/1X1', 'DGRAD/1X1', (1, 'p1', 'slabs'), USE_CLOSED_MODCONV=False),
    # ---- modulated 1x1 (always the fp32 kind; the weight gradient has a split form)
    R('1x1_split_wgrad', '1x1', (2, 128, 128, 8, 16), 'FWD/1X1', 'DGRAD/1X1', (1, 'p1', 'slabs')),
    R('1x1_fp32', '1x1', (2, 64, 96, 8, 8), 'FWD/1X1', 'DGRAD/1X1', (0, 'fp32', 'slabs')),
    # ---- plain 1x1 (ResBlock skip branch; the shape is the skip's: x is (2H) x (2W))
    R('skip_p1s6', 'skip', (2, 128, 128, 128, 128), 'P6FWD/1X1S6', 'P6DGRAD/1X1S6', (1, 'p1', 'slabs')),
    R('skip_p1s6_fwd_only', 'skip', (2, 64, 128, 128, 128), 'P6FWD/1X1S6', 'DGRAD/1X1', (0, 'fp32', 'slabs')),  # dgrad M = 64
    R('skip_p1s6_dgrad_only', 'skip', (2, 128, 64, 128, 128), 'FWD/1X1', 'P6DGRAD/1X1S6', (0, 'fp32', 'slabs')),  # fwd M = 64
    R('skip_fp32_split_convs', 'skip', (1, 64, 64, 8, 16), 'FWD/1X1', 'DGRAD/1X1', (0, 'fp32', 'slabs')),     # conv1 3X3W6, conv2 S2S6 / T2S6
    R('skip_fp32', 'skip', (2, 64, 64, 8, 8), 'FWD/1X1', 'DGRAD/1X1', (0, 'fp32', 'slabs')),
    R('skip_p1s6_few_blocks', 'skip', (1, 128, 128, 128, 128), 'FWD/1X1', 'DGRAD/1X1', (1, 'p1', 'slabs')),    # 64 blocks
    R('skip_split_1x1_off', 'skip', (2, 128, 128, 128, 128), 'FWD/1X1', 'DGRAD/1X1', (1, 'p1', 'slabs'), USE_SPLIT_1X1=False),
]
BY_NAME = {r.name: r for r in ROUTES}
assert len(BY_NAME) == len(ROUTES), 'route names must be unique'

# predicate edges: (just inside, just outside) - each pair differs in the one quantity its predicate tests
EDGES = {
    'wino6 K % 32': ('3x3_w6_dgrad_direct', '3x3_wino_k16'),
    'wino6 M % 64': ('3x3_w6_dgrad_direct', '3x3_m32'),
    'wino6 H % 8': ('3x3_w6_dgrad_direct', '3x3_h4'),
    'wino6 W % 32': ('3x3_w6_dgrad_direct', '3x3_w48'),
    'wino6 pair16 blocks': ('3x3_w6_pair16', '3x3_pair16_few_blocks'),
    'wino6 pair16 even B': ('3x3_w6_pair16', '3x3_pair16_odd_batch'),
    's2s6 K >= 32': ('down_s2s6_dgrad_fp32', 'down_k16'),
    's2s6 H % 8': ('down_s2s6_dgrad_fp32', 'down_h4'),
    's2s6 W % 16': ('down_s2s6_dgrad_fp32', 'down_w8'),
    't2s6 M % 64': ('up_t2s6_s2s6', 'up_t2s6_dgrad_fp32'),
    't2s6 W % 16': ('up_t2s6_s2s6', 'up_w8'),
    'p1s6 blocks': ('skip_p1s6', 'skip_p1s6_few_blocks'),
    'p1s6 M % 128': ('skip_p1s6', 'skip_p1s6_fwd_only'),
    'wgrad6 pair even B': ('3x3_m32', '3x3_m32_odd_batch'),
}


# ------------------------------------------------------------------------------------------------ geometry and reference of an op kind
def in_hw(op, H, W):
    """the input's size for the low-resolution size H x W"""
    return (2 * H + 1, 2 * W + 1) if op == 'down' else (H, W)


def out_hw(op, H, W):
    return (2 * H + 1, 2 * W + 1) if op == 'up' else (H, W)


def ref_conv(op, x, w):
    """the op kind's convolution from stock torch ops, in the operands' precision"""
    if op == '3x3':
        return F.conv2d(x, w, padding=1)
    if op in ('1x1', 'skip'):
        return F.conv2d(x, w)
    if op == 'up':
        return F.conv_transpose2d(x, w.transpose(0, 1), stride=2)
    return F.conv2d(x, w, stride=2)


# ------------------------------------------------------------------------------------------------ switches
@contextlib.contextmanager
def switches(**sw):
    """set the module switches of op/modconv for the duration (defaults for the rest), restored in `finally`"""
    from transeditor_amd.op import modconv as mc
    names = ('USE_WINOGRAD', 'USE_SPLIT_S2', 'USE_SPLIT_T2', 'USE_SPLIT_1X1', 'USE_CLOSED_MODCONV')
    old = {n: getattr(mc, n) for n in names}
    old_split = mc.USE_SPLIT_BF16
    want = dict(DEFAULT_SWITCHES, **sw)
    try:
        for n in names:
            setattr(mc, n, want[n])
        mc.set_split_bf16(want['split_bf16'])
        yield mc
    finally:
        for n, v in old.items():
            setattr(mc, n, v)
        mc.set_split_bf16(old_split)


# ------------------------------------------------------------------------------------------------ what the selectors pick
def _names(pair):
    return PACK_NAMES[pair[0]], CONV_NAMES[pair[1]]


def _w(route):
    B, K, M, H, W = route.shape
    ks = 1 if route.op in ('1x1', 'skip') else 3
    return torch.empty(M, K, ks, ks)          # (the selectors read the shape only)


def conv_routes(route):
    """(fwd, dgrad) as name pairs, from the selectors under the switches currently set"""
    from transeditor_amd.op import modconv as mc
    B, K, M, H, W = route.shape
    w = _w(route)
    if route.op == 'skip':
        return _names(mc.plain_1x1_kinds(B, w, H, W)), _names(mc.plain_1x1_kinds(B, w, H, W, dgrad=True))
    return _names(mc.fwd_kinds(route.op, B, w, H, W)), _names(mc.bwd_kinds(route.op, B, w, H, W))


def wgrad_problem(route):
    """(kind code, B, Co, Ci, H, W) of the correlation te_wgrad_f32 runs for the weight gradient (as op/modconv._wgrad_raw calls it)"""
    B, K, M, H, W = route.shape
    if route.op == 'down':        # the transposed kind with the roles of the two tensors swapped
        return _lib.CONV_T2, B, K, M, H, W
    kind = {'3x3': _lib.CONV_3X3, 'up': _lib.CONV_T2, '1x1': _lib.CONV_1X1, 'skip': _lib.CONV_1X1}[route.op]
    return kind, B, M, K, H, W


def group_plan(kind, B, Co, Ci, H, W):
    nb, sc = C.c_int(0), C.c_int(0)
    rc = _lib.lib().te_wgrad_group_plan(kind, B, Co, Ci, H, W, C.byref(nb), C.byref(sc))
    assert rc == 0
    return nb.value, sc.value


def wgrad_form(kind, B, Co, Ci, H, W, NB=1):
    """(te_wgrad_split_supported, the kernel te_wgrad6_form reports - the decision the launch dispatches on - for aligned operands)"""
    return int(_lib.lib().te_wgrad_split_supported(kind, Co, Ci, H, W)), _lib.wgrad6_form(kind, B, Co, Ci, H, W, NB)


def wgrad_route(route):
    """(split_supported, form of the per-sample launch, plan of the plain gradient)"""
    kind, B, Co, Ci, H, W = wgrad_problem(route)
    sup, form = wgrad_form(kind, B, Co, Ci, H, W)
    nb, _ = group_plan(kind, B, Co, Ci, H, W)
    if nb > 1:        # the grouped launch takes the same kernel as the per-sample one
        assert wgrad_form(kind, B, Co, Ci, H, W, nb)[1] == form
    return sup, form, ('group' if nb > 1 else 'slabs')


def actual(route):
    """(fwd, dgrad, wgrad) the selectors and planners pick for the entry under its switches"""
    with switches(**route.switches):
        f, d = conv_routes(route)
        return f, d, wgrad_route(route)


def check(route):
    """raise AssertionError naming the entry when it does not land on its declared routes"""
    got = actual(route)
    want = (route.fwd, route.dgrad, route.wgrad)
    assert got == want, f'route {route.name} {route.op} {route.shape} {route.switches}: expected {want}, selectors give {got}'


# ------------------------------------------------------------------------------------------------ sweep of the selectors
SWEEP_B = (1, 2, 3, 8, 9, 16)
SWEEP_C = (8, 12, 16, 32, 64, 96, 128, 512)
SWEEP_HW = ((4, 8), (8, 16), (8, 32), (9, 9), (16, 16), (32, 16), (8, 48), (32, 32), (64, 64))
SWEEP_SWITCHES = ({}, {'USE_WINOGRAD': False}, {'split_bf16': False}, {'USE_SPLIT_S2': False}, {'USE_SPLIT_T2': False},
                  {'USE_SPLIT_1X1': False})


def sweep():
    """every (fwd pack/kind, dgrad pack/kind, plain 1x1 pack/kind, wgrad form) the selectors return over a grid of shapes and switches"""
    from transeditor_amd.op import modconv as mc
    fwd, dgrad, plain, forms = set(), set(), set(), set()
    for sw in SWEEP_SWITCHES:
        with switches(**sw):
            for B, K, M, (H, W) in itertools.product(SWEEP_B, SWEEP_C, SWEEP_C, SWEEP_HW):
                w3, w1 = torch.empty(M, K, 3, 3), torch.empty(M, K, 1, 1)
                for op in ('3x3', 'up', 'down', '1x1'):
                    w = w1 if op == '1x1' else w3
                    fwd.add(_names(mc.fwd_kinds(op, B, w, H, W)))
                    dgrad.add(_names(mc.bwd_kinds(op, B, w, H, W)))
                plain.add(_names(mc.plain_1x1_kinds(B, w1, H, W)))
                plain.add(_names(mc.plain_1x1_kinds(B, w1, H, W, dgrad=True)))
                for kind in (_lib.CONV_3X3, _lib.CONV_T2, _lib.CONV_1X1):
                    forms.add(wgrad_form(kind, B, M, K, H, W)[1])
            # (p1s6 needs H W % 256 == 0 and a block per two CUs: a few large images)
            for B, K, M in itertools.product((1, 2, 8), (64, 128, 512), (64, 128, 512)):
                w1 = torch.empty(M, K, 1, 1)
                plain.add(_names(mc.plain_1x1_kinds(B, w1, 64, 64)))
                plain.add(_names(mc.plain_1x1_kinds(B, w1, 64, 64, dgrad=True)))
    return fwd, dgrad, plain, forms

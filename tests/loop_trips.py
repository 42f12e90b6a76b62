"""Loop-trip table: the smallest shapes at which the kernels that launch fewer blocks than they have work go round their loop more
than once.

Two kinds of loop.  The FIR kernels (csrc/upfirdn2d.hip: blur44_kernel, fir_tile_kernel) walk the planes pg, pg + zgroups, ... of a
tile with the next plane prefetched into registers across a barrier; the elementwise and second-pass kernels cap their grid and
stride over the rest.  In the other unit tests every one of these loops runs once.

An entry names the op, its shape and arguments, the loop it targets and the trips it expects as (fewest, most) over the blocks
(threads) of the launch.  The expected trips are data; what a launch really does comes from the library's host-side queries
(te_*_plan / te_*_cover / te_fir_form in include/te_hip.h, each of which calls the grid function of the launch), never from constants
restated here; a plane-walk entry's `loop` is asserted against the instantiation that te_fir_form plans.  tests/test_loop_trips_cpu.py checks the table against the queries without a GPU, tests/test_gpu_loop_trips.py runs every
entry against fp64 after re-asserting its trips.
"""
import ctypes as C
from dataclasses import dataclass, field

from transeditor_amd import _lib


@dataclass(frozen=True)
class Trip:
    name: str
    op: str          # see actual()
    shape: tuple
    loop: str        # the kernel whose loop the entry is about
    trips: tuple     # (fewest, most) trips of a block (plane walks) or of a thread (capped grids)
    args: dict = field(default_factory=dict)

    def __hash__(self):
        return hash(self.name)


def T(name, op, shape, loop, trips, **args):
    return Trip(name, op, shape, loop, trips, args)


BLUR = (1, 3, 3, 1)      # the model's blur taps (outer product, normalised by the ops)

# ---- FIR plane walks: trips 2 and 3 in one launch, plane count no multiple of 8.
# pad = (pad0, pad1) of the forward op; gpad = the four pads (x0, x1, y0, y1) of the adjoint pass, whose input is the forward output.
PLANE_WALKS = [
    # blur44 MODE 0, one tile per plane: 7145 planes
    T('blur_bias_act_1tile', 'blur_bias_act', (5, 1429, 6, 7), 'blur44_kernel<0,2,false>', (2, 3), pad=(2, 1)),
    T('blur_plain_1tile_d3', 'upfirdn2d', (5, 1429, 6, 7), 'blur44_kernel<0,3,false>', (2, 3), pad=(1, 1), up=1, down=1),
    # the +1 rule: a 33 x 65 output is one tile whose edge lanes filter a third row / fifth column
    T('blur_bias_act_ext', 'blur_bias_act', (5, 1429, 33, 65), 'blur44_kernel<0,2,true>', (2, 3), pad=(2, 1)),
    # four tiles per plane: 1636 planes, with the xcd_tile decode
    T('blur_bias_act_4tiles', 'blur_bias_act', (4, 409, 40, 70), 'blur44_kernel<0,2,false>', (2, 3), pad=(2, 1)),
    # blur44 MODE 1 (activation-gradient prologue): the backward of the three cases above
    T('blur_actgrad_1tile', 'blur_actgrad', (5, 1429, 6, 7), 'blur44_kernel<1,3,false>', (2, 3), gpad=(1, 2, 1, 2)),
    T('blur_actgrad_ext', 'blur_actgrad', (5, 1429, 33, 65), 'blur44_kernel<1,3,true>', (2, 3), gpad=(1, 2, 1, 2)),
    T('blur_actgrad_4tiles', 'blur_actgrad', (4, 409, 40, 70), 'blur44_kernel<1,3,false>', (2, 3), gpad=(1, 2, 1, 2)),
    # blur44 MODE 2 (activation-gradient epilogue)
    T('blur_gradact_1tile', 'blur_gradact', (5, 1429, 6, 7), 'blur44_kernel<2,3,false>', (2, 3), gpad=(1, 2, 1, 2)),
    T('blur_gradact_4tiles', 'blur_gradact', (4, 409, 40, 70), 'blur44_kernel<2,3,false>', (2, 3), gpad=(1, 2, 1, 2)),
    # fir_tile_kernel: upsampling by 2 (13 065 planes of 4 x 8 -> 8 x 16) and its adjoint (down by 2, 8 x 16 -> 4 x 8)
    T('fir_up2', 'upfirdn2d', (5, 2613, 4, 8), 'fir_tile_kernel<2,1,4,4>', (2, 3), pad=(2, 1), up=2, down=1),
    T('fir_down2', 'upfirdn2d', (5, 2613, 8, 16), 'fir_tile_kernel<1,2,4,4>', (2, 3), pad=(1, 1), up=1, down=2),
    # rows narrower than one 16-byte group: the activation-gradient prologue on the generic tile kernel
    T('blur_actgrad_w3', 'blur_actgrad', (5, 2613, 4, 3), 'fir_tile_kernel<1,1,4,4,AG>', (2, 3), gpad=(1, 2, 1, 2)),
]

# ---- capped grids: a thread strides to a second element
CAPPED = [
    T('fir_direct_f32', 'fir_direct', (2, 9, 242, 242), 'fir_direct_kernel', (1, 2), taps=(1, 2, 1), pad=(1, 1), dtype='float32'),
    T('fir_direct_f16', 'fir_direct', (2, 9, 242, 242), 'fir_direct_any_kernel<half>', (1, 2), taps=(1, 2, 1), pad=(1, 1), dtype='float16'),
    T('fir_direct_f64', 'fir_direct', (2, 9, 242, 242), 'fir_direct_any_kernel<double>', (1, 2), taps=(1, 2, 1), pad=(1, 1), dtype='float64'),
    T('chan_scale_vec4', 'chan_scale', (2, 33, 256, 256), 'chan_scale_vec4_kernel', (1, 2)),
    T('chan_scale_flat4', 'chan_scale', (2, 33, 257, 257), 'chan_scale_flat4_kernel', (1, 2)),       # planes straddle a 16-byte vector
    T('chan_scale_scalar', 'chan_scale', (5, 70001, 1, 3), 'chan_scale_kernel', (1, 2)),              # planes narrower than a vector
    T('bias_act_scalar', 'bias_act', (3, 7, 159, 159), 'bias_act_scalar_kernel', (1, 2), dtype='float32'),
    T('bias_act_f16', 'bias_act', (2, 5, 231, 231), 'bias_act_any_kernel<half>', (1, 2), dtype='float16'),
    T('bias_act_f64', 'bias_act', (2, 5, 231, 231), 'bias_act_any_kernel<double>', (1, 2), dtype='float64'),
    # (B, K, M, H, W) of the 3x3 op: 13 channel splits, 655 360 outputs through the fixed-order epilogue
    T('conv_finalize', 'conv_finalize', (20, 512, 512, 8, 8), 'conv_finalize_kernel', (1, 2)),
    # (rows, K, N) of a linear layer: the weight gradient [N, K] of 2055 rows = a split-K launch over 2048 rows + a 7-row tail
    T('splitk_finish', 'splitk_finish', (2055, 520, 512), 'splitk_finish_kernel', (1, 2)),
    # (B, S, Co, Ci, taps) of a te_wgrad_reduce_f32 problem that tests/test_gpu_determinism.py already runs against fp64: recorded
    # here so that the trip it relies on stays asserted
    T('sum_parts', 'sum_parts', (16, 1, 256, 256, 9), 'sum_parts_kernel', (2, 3)),
    # (B, K, M, H, W) of the 3x3 op whose weight (576, 512, 3, 3) packs as 18 x 16 = 288 tiles, in both directions and under both
    # Winograd forms
    T('pack_tiles_split', 'pack', (1, 512, 576, 8, 32), 'pack_tiles<9>', (1, 2), fwd='W6FWD/3X3W6', dgrad='W6DGRAD/3X3W6'),
    T('pack_tiles_fp32', 'pack', (1, 512, 576, 8, 32), 'pack_tiles<9>', (1, 2), fwd='WFWD/3X3W', dgrad='WDGRAD/3X3W', split_bf16=False),
]

TABLE = PLANE_WALKS + CAPPED
BY_NAME = {t.name: t for t in TABLE}
assert len(BY_NAME) == len(TABLE), 'entry names must be unique'


# ------------------------------------------------------------------------------------------------ what the library plans
def _cdiv(a, b):
    return -(-a // b)


def _plan(fn, *args):
    z, t = C.c_int(-1), C.c_int(-1)
    rc = fn(*args, C.byref(z), C.byref(t))
    assert rc == 0, f'{fn.__name__} refused {args} ({rc})'
    return z.value, t.value


def fir_plan(entry):
    """(planes, zgroups, tiles per plane) of the launch the entry makes; zgroups = 0 where the direct kernel runs"""
    L = _lib.lib()
    B, Cn, H, W = entry.shape
    a = entry.args
    if entry.op in ('blur_actgrad', 'blur_gradact'):
        fn = L.te_blur_actgrad_plan if entry.op == 'blur_actgrad' else L.te_blur_gradact_plan
        return (B * Cn,) + _plan(fn, B * Cn, H, W, 4, 4, *a['gpad'])
    taps = a.get('taps', BLUR)
    up, down = a.get('up', 1), a.get('down', 1)
    p0, p1 = a['pad']
    return (B * Cn,) + _plan(L.te_upfirdn2d_plan, B * Cn, H, W, 1, len(taps), len(taps), up, up, down, down, p0, p1, p0, p1)


def fir_loop(entry):
    """the kernel instantiation that te_fir_form plans for a plane-walk entry, as csrc/upfirdn2d.hip spells it"""
    from fir_forms import loop_name
    B, Cn, H, W = entry.shape
    a = entry.args
    if entry.op in ('blur_actgrad', 'blur_gradact'):
        f = _lib.fir_form(entry.op, B * Cn, H, W, a['gpad'])
    else:
        up, down, k = a.get('up', 1), a.get('down', 1), len(a.get('taps', BLUR))
        f = _lib.fir_form('upfirdn2d', B * Cn, H, W, a['pad'] * 2, k, k, (up, up), (down, down))
    assert not isinstance(f, int), f'{entry.name}: te_fir_form refuses ({f})'
    return loop_name(f)


def walk_trips(planes, zgroups):
    """(fewest, most) planes a block walks: the block of plane group pg < planes filters pg, pg + zgroups, ..."""
    assert zgroups > 0
    first, last = 0, min(zgroups, planes) - 1
    return _cdiv(planes - last, zgroups), _cdiv(planes - first, zgroups)


def stride_trips(n, cover):
    """(fewest, most) elements a thread of a grid-stride loop handles when one trip of the grid covers `cover` of n elements"""
    assert cover > 0
    return n // cover, _cdiv(n, cover)


def fir_out_hw(entry):
    B, Cn, H, W = entry.shape
    a = entry.args
    if 'gpad' in a:
        x0, x1, y0, y1 = a['gpad']
        return H + y0 + y1 - 3, W + x0 + x1 - 3
    k = len(a.get('taps', BLUR))
    up, down = a.get('up', 1), a.get('down', 1)
    p0, p1 = a['pad']
    return (H * up + p0 + p1 - k) // down + 1, (W * up + p0 + p1 - k) // down + 1


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def pack_kinds(entry):
    """pack kinds (forward, data gradient) of a 'pack' entry, by name"""
    return entry.args['fwd'].split('/')[0], entry.args['dgrad'].split('/')[0]


def conv_kinds(entry):
    """((pack, kind) of the forward, of the data gradient), by name, that op/modconv's selectors pick for a (B, K, M, H, W) entry of
    the 3x3 op under the entry's switches"""
    import torch

    import conv_routes as cr
    B, K, M, H, W = entry.shape
    sw = {k: v for k, v in entry.args.items() if k in cr.DEFAULT_SWITCHES}
    with cr.switches(**sw) as mc:
        w = torch.empty(M, K, 3, 3)
        return cr._names(mc.fwd_kinds('3x3', B, w, H, W)), cr._names(mc.bwd_kinds('3x3', B, w, H, W))


def actual(entry):
    """(fewest, most) trips of the entry's loop, from the library's queries"""
    L = _lib.lib()
    if entry in PLANE_WALKS:
        planes, zgroups, tiles = fir_plan(entry)
        assert zgroups > 0 and tiles > 0, f'{entry.name}: the direct kernel runs, not a plane walk'
        return walk_trips(planes, zgroups)
    if entry.op == 'fir_direct':
        if entry.args['dtype'] == 'float32':      # (the f16 / f64 entry points have the direct kernel only)
            assert fir_plan(entry)[1:] == (0, 0), f'{entry.name}: a plane-walking kernel runs, not the direct one'
        B, Cn = entry.shape[:2]
        n = B * Cn * _numel(fir_out_hw(entry))
        return stride_trips(n, L.te_upfirdn2d_direct_cover(n))
    if entry.op == 'chan_scale':
        B, Cn, H, W = entry.shape
        return stride_trips(_numel(entry.shape), L.te_chan_scale_cover(B * Cn, H * W, 1))
    if entry.op == 'bias_act':
        n = _numel(entry.shape)
        if entry.args['dtype'] != 'float32':
            return stride_trips(n, L.te_bias_act_any_cover(n))
        vec = C.c_int(-1)
        cover = L.te_bias_act_f32_cover(n, _numel(entry.shape[2:]), 1, C.byref(vec))
        assert vec.value == 0, f'{entry.name}: the 16-byte path runs, not the scalar one'
        return stride_trips(n, cover)
    if entry.op == 'conv_finalize':
        B, K, M, H, W = entry.shape
        assert conv_kinds(entry) == (('FWD', '3X3'), ('DGRAD', '3X3')), f'{entry.name}: not the direct kernel: {conv_kinds(entry)}'
        assert L.te_conv_splitk_count(_lib.CONV_3X3, B, K, M, H, W) > 1, f'{entry.name}: the launch is not split'
        assert L.te_conv_splitk_count(_lib.CONV_3X3, B, M, K, H, W) > 1, f'{entry.name}: the data gradient is not split'
        return stride_trips(B * M * H * W, L.te_conv_finalize_cover(B * M * H * W))
    if entry.op == 'splitk_finish':
        R, K, N = entry.shape
        return stride_trips(N * K, L.te_small_gemm_splitk_finish_cover(N, K))
    if entry.op == 'sum_parts':
        B, S, Co, Ci, taps = entry.shape
        parts, cover = C.c_int(-1), C.c_int64(-1)
        assert L.te_wgrad_reduce_plan(B, S, Co, Ci, taps, C.byref(parts), C.byref(cover)) == 0
        assert parts.value > 1, f'{entry.name}: the first pass writes dW itself, no second pass'
        return stride_trips(Co * Ci * taps, cover.value)
    if entry.op == 'pack':
        B, K, M, H, W = entry.shape
        want = tuple(tuple(entry.args[d].split('/')) for d in ('fwd', 'dgrad'))
        assert conv_kinds(entry) == want, f'{entry.name}: expected {want}, the selectors give {conv_kinds(entry)}'
        got = set()
        for kind in pack_kinds(entry):       # both layouts are packed from the weight (M, K, 3, 3)
            blocks, tiles = C.c_int(-1), C.c_int(-1)
            assert L.te_conv_pack_plan(getattr(_lib, 'PACK_' + kind), M, K, 3, C.byref(blocks), C.byref(tiles)) == 0
            got.add(stride_trips(tiles.value, blocks.value))
        assert len(got) == 1, f'{entry.name}: the two layouts walk differently: {got}'
        return got.pop()
    raise AssertionError(f'unknown op {entry.op}')


def check(entry):
    """raise AssertionError naming the entry when its loop does not make the declared trips"""
    got = actual(entry)
    assert got == entry.trips, f'{entry.name} {entry.op} {entry.shape} {entry.args}: expected trips {entry.trips} of {entry.loop}, the library plans {got}'
    if entry in PLANE_WALKS:      # the instantiation the entry names; a last trip that some blocks have and others do not
        assert fir_loop(entry) == entry.loop, f'{entry.name}: expected {entry.loop}, the library plans {fir_loop(entry)}'
        assert got[1] == got[0] + 1 and got[0] >= 2, f'{entry.name}: trips {got}'
        assert fir_plan(entry)[0] % 8 != 0, f'{entry.name}: plane count is a multiple of 8'
    else:
        assert got[1] >= 2, f'{entry.name}: trips {got}'

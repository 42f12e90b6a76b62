"""The loop-trip table (tests/loop_trips.py) against the library's host-side queries: every entry makes the trips it declares, every
plane-walk entry has blocks with t and with t + 1 trips.  Host code only, no GPU."""
import ctypes as C

import pytest

import loop_trips as lt
from transeditor_amd import _lib

IDS = lambda e: e.name


@pytest.mark.parametrize('entry', lt.TABLE, ids=IDS)
def test_entry_makes_its_trips(entry):
    lt.check(entry)


@pytest.mark.parametrize('entry', lt.PLANE_WALKS, ids=IDS)
def test_plane_walk_has_a_ragged_last_trip(entry):
    planes, zgroups, tiles = lt.fir_plan(entry)
    assert zgroups % 8 == 0 and planes % 8 != 0
    per_block = [lt._cdiv(planes - pg, zgroups) for pg in range(zgroups)]
    t = min(per_block)
    assert t >= 2 and set(per_block) == {t, t + 1}
    assert sum(per_block) == planes                     # every plane is filtered by exactly one plane group


def test_tile_counts_of_the_plane_walks():
    tiles = {e.name: lt.fir_plan(e)[2] for e in lt.PLANE_WALKS}
    assert tiles['blur_bias_act_1tile'] == tiles['blur_bias_act_ext'] == tiles['blur_actgrad_ext'] == 1       # 33 x 65: the +1 rule
    assert tiles['blur_bias_act_4tiles'] == tiles['blur_actgrad_4tiles'] == tiles['blur_gradact_4tiles'] == 4
    assert tiles['fir_up2'] == tiles['fir_down2'] == tiles['blur_actgrad_w3'] == 1
    # the bias-gradient partials are laid out with the tile count te_blur_actgrad_tiles gives
    for e in lt.PLANE_WALKS:
        if 'gpad' in e.args:
            assert _lib.lib().te_blur_actgrad_tiles(e.shape[2], e.shape[3], 4, 4, *e.args['gpad']) == tiles[e.name]


def test_small_problems_make_one_trip():
    """the shapes of the other unit tests are on the near side of every threshold (that is the gap the table closes)"""
    L = _lib.lib()
    z, t = C.c_int(-1), C.c_int(-1)
    assert L.te_upfirdn2d_plan(27, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1, C.byref(z), C.byref(t)) == 0
    assert z.value >= 27 and z.value % 8 == 0 and t.value == 1          # one plane per block
    assert L.te_upfirdn2d_plan(27, 16, 16, 1, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, C.byref(z), C.byref(t)) == 0
    assert (z.value, t.value) == (0, 0)                                 # 3 x 3 taps: the direct kernel
    assert L.te_upfirdn2d_direct_cover(1000) == 1024 and L.te_bias_act_any_cover(1000) == 1024
    assert L.te_chan_scale_cover(8, 64 * 64, 1) == 8 * 64 * 64
    assert L.te_conv_finalize_cover(16 * 512 * 16) == 16 * 512 * 16
    assert L.te_small_gemm_splitk_finish_cover(32, 512) == 32 * 512


def test_queries_refuse_bad_arguments():
    L = _lib.lib()
    z, t = C.c_int(0), C.c_int(0)
    assert L.te_upfirdn2d_plan(0, 4, 4, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0, C.byref(z), C.byref(t)) < 0
    assert L.te_upfirdn2d_plan(4, 4, 4, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0, None, C.byref(t)) < 0
    assert L.te_blur_actgrad_plan(4, 4, 4, 3, 3, 1, 1, 1, 1, C.byref(z), C.byref(t)) < 0
    assert L.te_blur_gradact_plan(4, 4, 3, 4, 4, 1, 2, 1, 2, C.byref(z), C.byref(t)) < 0          # in_w < 4
    assert L.te_upfirdn2d_direct_cover(0) < 0 and L.te_chan_scale_cover(0, 4, 1) < 0 and L.te_bias_act_any_cover(-1) < 0
    assert L.te_bias_act_f32_cover(0, 4, 1, None) < 0 and L.te_conv_finalize_cover(0) < 0
    assert L.te_small_gemm_splitk_finish_cover(0, 4) < 0
    assert L.te_conv_pack_plan(99, 8, 8, 3, C.byref(z), C.byref(t)) < 0
    assert L.te_wgrad_reduce_plan(1, 1, 8, 8, 5, C.byref(z), C.byref(t)) < 0

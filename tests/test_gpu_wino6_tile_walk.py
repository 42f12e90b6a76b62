"""The tile walk of wino6q_kernel (csrc/wino6.hip): a block of the two-image form of TE_CONV_3X3W6 walks a run of consecutive tiles and
carries its pipeline across them.  Every output element sees the same products in the same order as in the ping-pong kernel
(form 1), so the comparison is torch.equal, for runs of at most 2 and 3 tiles and the automatic choice, with every epilogue
configuration of test_split_bf16_kernel_forms_are_bit_identical, with and without style scales.  The output buffer is filled with NaN
before every call: a tile no block wrote shows.  (The barrier schedule itself is checked on the CPU: tests/test_wino6_schedule.py.)"""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from transeditor_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, K, M, H, W)                    tiles  what it exercises
WALK_SHAPES = [(3, 32, 128, 16, 64),   # 12   two stages, the shortest pipeline; runs cross sample boundaries; every tile an edge tile, flags change
               (2, 64, 256, 24, 96),   # 18   per M block, two M blocks; interior and edge tiles alternate; uneven runs for n = 3
               (1, 128, 128, 8, 32),   # 1    a block with a single tile under a forced n = 2
               (5, 32, 384, 8, 32),    # 5    fewer tiles than XCDs: blocks without a tile
               (2, 160, 128, 40, 96)]  # 30   ten stages; H not a power of two


def conv_w6(x, u6, M, isc=None, osc=None, bias=None, act=0, res=None, mask_ref=None, mask_gain=1.0):
    """TE_CONV_3X3W6 into an output buffer that holds NaN before the call"""
    B, K, H, W = x.shape
    out = torch.full((B, M, H, W), float('nan'), device=x.device, dtype=x.dtype)
    assert _lib.lib().te_conv_splitk_count(_lib.CONV_3X3W6, B, K, M, H, W) == 1
    _lib._check(_lib.lib().te_conv_res_f32(_lib._ptr(out), _lib._ptr(None), _lib._ptr(x), _lib._ptr(u6), _lib._ptr(isc), _lib._ptr(osc),
                                           _lib._ptr(bias), _lib._ptr(res), _lib._ptr(mask_ref), mask_gain, act, _lib.CONV_3X3W6,
                                           B, K, M, H, W, _lib._stream()), 'te_conv_res_f32')
    return out


def operands(B, K, M, H, W):
    x = synth.normal((B, K, H, W), f'w6tw.x.{K}.{H}').to(DEV)
    w = (synth.normal((M, K, 3, 3), f'w6tw.w.{M}.{K}') / (3 * math.sqrt(K))).to(DEV)
    isc, osc = (1 + 0.3 * synth.normal((B, K), 'w6tw.i')).to(DEV), (1 + 0.3 * synth.normal((B, M), 'w6tw.o')).to(DEV)
    bias = synth.normal((M,), 'w6tw.b').to(DEV)
    res, mref = synth.normal((B, M, H, W), 'w6tw.r').to(DEV), synth.normal((B, M, H, W), 'w6tw.m').to(DEV)
    return x, w, isc, osc, bias, res, mref


def three_epilogues(x, u6, M, isc, osc, bias, res, mref):
    return (conv_w6(x, u6, M, isc, osc, bias, 3),
            conv_w6(x, u6, M, isc, None, bias, 4, res=res, mask_ref=mref, mask_gain=1.3),
            conv_w6(x, u6, M, isc))


@pytest.mark.parametrize('styled', [True, False])
@pytest.mark.parametrize('B,K,M,H,W', WALK_SHAPES)
def test_tile_walk_is_bit_identical_to_the_ping_pong_kernel(B, K, M, H, W, styled):
    x, w, isc, osc, bias, res, mref = operands(B, K, M, H, W)
    if not styled:
        isc = None
    u6 = _lib.conv_pack(w, _lib.PACK_W6FWD, 0.9)
    old_form, old_tpb = _lib.wino6_form(-1), _lib.wino6_tiles_per_block(-1)
    try:
        _lib.wino6_form(1)
        assert _lib.conv_split_form(_lib.CONV_3X3W6, B, K, M, H, W, styled)['two_image'] == 0          # the ping-pong kernel
        want = three_epilogues(x, u6, M, isc, osc, bias, res, mref)
        _lib.wino6_form(3)
        for n in (2, 3, 0):
            _lib.wino6_tiles_per_block(n)
            f = _lib.conv_split_form(_lib.CONV_3X3W6, B, K, M, H, W, styled)
            assert f['two_image'] == 1 and (f['tpb'] == n or n == 0) and (f['lists'] > 0) == (f['tpb'] >= 2), f      # the two-image kernel on runs of n
            got = three_epilogues(x, u6, M, isc, osc, bias, res, mref)
            for k, (a, b) in enumerate(zip(want, got)):
                assert torch.isfinite(b).all(), f'tiles_per_block {n}, epilogue {k}: outputs nobody wrote'
                assert torch.equal(a, b), f'tiles_per_block {n}, epilogue {k}: {int((a != b).sum())} elements differ'
    finally:
        _lib.wino6_form(old_form)
        _lib.wino6_tiles_per_block(old_tpb)
    assert _lib.wino6_form(-1) == old_form and _lib.wino6_tiles_per_block(-1) == old_tpb


def test_tile_walk_vs_fp64():
    """the family's bar, 5e-6 against fp64 F.conv2d, with the walk forced"""
    B, K, M, H, W = 3, 96, 128, 24, 64
    x, w, isc, _, _, _, _ = operands(B, K, M, H, W)
    want = F.conv2d(x.double() * isc.double()[:, :, None, None], w.double(), padding=1)
    old_form, old_tpb = _lib.wino6_form(3), _lib.wino6_tiles_per_block(3)
    try:
        f = _lib.conv_split_form(_lib.CONV_3X3W6, B, K, M, H, W, True)
        assert (f['two_image'], f['tpb']) == (1, 3) and f['lists'] > 0
        got = conv_w6(x, _lib.conv_pack(w, _lib.PACK_W6FWD), M, isc)
    finally:
        _lib.wino6_form(old_form)
        _lib.wino6_tiles_per_block(old_tpb)
    e = rel_err(got, want)
    print(f'tile walk (n = 3) vs fp64: {e:.2e}')
    assert e < 5e-6


def test_tiles_per_block_hook_round_trips():
    old = _lib.wino6_tiles_per_block(-1)
    try:
        assert _lib.wino6_tiles_per_block(3) == old
        assert _lib.wino6_tiles_per_block(-1) == 3                   # a query returns what was set
        assert _lib.wino6_tiles_per_block(3) == 3 and _lib.wino6_tiles_per_block(-1) == 3      # its own value changes nothing
        assert _lib.wino6_tiles_per_block(1 << 20) == 3 and _lib.wino6_tiles_per_block(-7) == 3   # out of range: query only
        assert _lib.wino6_tiles_per_block(0) == 3 and _lib.wino6_tiles_per_block(-1) == 0
    finally:
        _lib.wino6_tiles_per_block(old)
    assert _lib.wino6_tiles_per_block(-1) == old


CHILD = '''
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
import test_gpu_wino6_tile_walk as T
from transeditor_amd import _lib
B, K, M, H, W = T.WALK_SHAPES[0]
x, w, isc, osc, bias, res, mref = T.operands(B, K, M, H, W)
u6 = _lib.conv_pack(w, _lib.PACK_W6FWD, 0.9)
_lib.wino6_form(1)
want = T.three_epilogues(x, u6, M, isc, osc, bias, res, mref)
_lib.wino6_form(3)
for n in (2, 3, 0):
    _lib.wino6_tiles_per_block(n)
    got = T.three_epilogues(x, u6, M, isc, osc, bias, res, mref)
    assert all(torch.equal(a, b) for a, b in zip(want, got)), n
print('interleaved ok')
'''


def test_tile_walk_in_interleaved_xcd_order():
    """TE_XCD_INTERLEAVED is read once per process: a fresh child, which compares against form 1 inside itself"""
    env = dict(os.environ, TE_XCD_INTERLEAVED='1')
    r = subprocess.run([sys.executable, '-c', CHILD.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))], env=env, capture_output=True,
                       text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and 'interleaved ok' in r.stdout

"""Every form of the FIR kernels (tests/fir_forms.py) against fp64, tile by tile, launched at the C ABI (_lib._launch) so that
partial[plane][tile] is seen before anything sums it.  Each test re-asserts its entry's key (kernel, MODE, D, EXT) and situations
(ext, tiles, s, pads) through te_fir_form before it compares numbers, then runs the four instruments of tests/fir_forms.py:

  1. elementwise: |y - y64| <= (T + 2) u (|k| * |x| + |b|) g + u |y64| for every output element (tests/test_gpu_loop_trips.py derives it;
     T = taps that meet a sample, g the leaky-ReLU gain), elements on the kink left out up to KINK_CAP (the CPU test finds none);
  2. exact: under the EXACT operands (integers, alpha 1/2, scale 1) the output and every partial[plane][tile] carry the bits of the fp64
     restatement, ownership restated from the query's tile size;
  3. per tile: partial[plane][tile] within (Lt + 1) u sum |terms| of its own tile under the normal operands (+ the outputs' bounds where
     the terms are outputs);
  4. guards: output and partial inside pattern-filled buffers - every element written, nothing around them touched - and a second run
     gives the same bits.
tests/test_fir_forms_cpu.py proves each instrument on a model with planted defects.  `max err / bound` per entry and the worst per key
are printed at the end of the module; MEASURED is a copy of that report from the MI355X, which nothing asserts.
"""
import pytest
import torch

import fir_forms as ff
import fp64_check
from transeditor_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RESULTS = []
IDS = lambda e: e.name
SUFFIX = {'float32': 'f32', 'float16': 'f16', 'float64': 'f64'}

# worst max err / bound per kernel (kernel, MODE, D, EXT) over both instruments with a bound; MI355X (a record, nothing asserts it)
MEASURED = {('blur44', 0, 0, 0): 0.2302, ('blur44', 0, 0, 1): 0.2356, ('blur44', 0, 1, 0): 0.2192, ('blur44', 0, 1, 1): 0.2282,
            ('blur44', 0, 2, 0): 0.2391, ('blur44', 0, 2, 1): 0.3193, ('blur44', 0, 3, 0): 0.2313, ('blur44', 0, 3, 1): 0.2651,
            ('blur44', 1, 0, 0): 0.2337, ('blur44', 1, 0, 1): 0.2808, ('blur44', 1, 1, 0): 0.2715, ('blur44', 1, 1, 1): 0.2965,
            ('blur44', 1, 2, 0): 0.2575, ('blur44', 1, 2, 1): 0.2851, ('blur44', 1, 3, 0): 0.2575, ('blur44', 1, 3, 1): 0.2763,
            ('blur44', 2, 0, 0): 0.2147, ('blur44', 2, 0, 1): 0.2574, ('blur44', 2, 1, 0): 0.2261, ('blur44', 2, 1, 1): 0.2569,
            ('blur44', 2, 2, 0): 0.2313, ('blur44', 2, 2, 1): 0.2113, ('blur44', 2, 3, 0): 0.2310, ('blur44', 2, 3, 1): 0.1992,
            ('direct', 0, 0, 0): 0.9958, ('tile_ag', 0, 0, 0): 0.1872, ('tile_down2', 0, 0, 0): 0.2251, ('tile_up2', 0, 0, 0): 0.4832}

_report = fp64_check.report_fixture('max err / bound per entry (tests/test_gpu_fir_forms.py):', RESULTS, lambda name: ff.BY_NAME[name].key,
                                    'worst per key (kernel, MODE, D, EXT):', widths=(58, 8))


def launch(e, f, ops):
    """the entry's launch at the C ABI into guarded buffers -> fir_forms.Run"""
    run = ff.buffers(e, f, DEV)
    dt = getattr(torch, e.dtype)
    kh, kw = ops.k.shape
    assert ops.x.data_ptr() % 16 == e.off and (ops.ref is None or ops.ref.data_ptr() % 16 == e.off), 'the operands have the alignment the table says'
    if e.op == ff.UP:
        args = [_lib._ptr(run.y, dt), _lib._ptr(ops.x, dt), _lib._ptr(ops.k, dt), e.planes, e.H, e.W, e.minor, kh, kw, e.up[0], e.up[1],
                e.down[0], e.down[1], *e.pad]
        if e.dtype == 'float32':
            args += [_lib._ptr(ops.b), e.bias or 1, e.act, ops.alpha, ops.scale]
        _lib._launch('te_upfirdn2d_' + SUFFIX[e.dtype], *args)
    else:
        _lib._launch('te_blur_actgrad_f32' if e.op == ff.AG else 'te_blur_gradact_f32', _lib._ptr(run.y), _lib._ptr(run.part), _lib._ptr(ops.x),
                     _lib._ptr(ops.ref), _lib._ptr(ops.k), e.planes, e.H, e.W, kh, kw, *e.pad, ops.alpha, ops.scale)
    ff.guards(e, run)
    return run


@pytest.mark.parametrize('entry', ff.TABLE, ids=IDS)
def test_form_against_fp64(entry):
    e = entry
    f = ff.check(e)
    with torch.no_grad():
        ops = ff.operands(e, device=DEV)
        run = launch(e, f, ops)
        R = ff.reference(e, f, ops)
        ff.elementwise(e, R, run, RESULTS)
        ff.per_tile(e, R, run, RESULTS)
        again = launch(e, f, ops)
        assert torch.equal(run.ybuf, again.ybuf), f'{e.name}: a second run gives other output bits'
        assert run.pbuf is None or torch.equal(run.pbuf, again.pbuf), f'{e.name}: a second run gives other partial sums'
        opx = ff.operands(e, exact=True, device=DEV)
        ff.exact(e, ff.reference(e, f, opx), launch(e, f, opx))

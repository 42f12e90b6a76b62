"""Generate tests/golden/reference_kernels.npz: the outputs of the REFERENCE's own two native kernels on the GPU.

    python -m oracle.gen_ref_kernels [OUT_DIR]      # from the repo root, on a GPU, with oracle/_ref built (oracle/build_ref_ops.py)

The inputs are the deterministic draws of transeditor_amd/synth.py for the cases listed in tests/test_gpu_reference_kernels.py,
which compares our kernels against what is written here:

* fused_bias_act in fp32 (forward, gradient, gradient of the gradient) and in double: compared bit for bit, so only the SHA-256
  of each output's bytes is stored (the outputs of the largest cases are megabytes each);
* fused_bias_act in half: the output values themselves;
* upfirdn2d: the output as its distance in units in the last place from the CPU oracle's fp64 result rounded to fp32
  (T.fir_encode / T.fir_reference: mostly small integers, a fraction of the bytes of the values), or the values themselves
  where the oracle cannot express the padding.

Data only; the reference kernels are not needed once the fixture exists.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import build_ref_ops, te_oracle as O          # noqa: E402
from transeditor_amd import synth                          # noqa: E402
import test_gpu_reference_kernels as T                     # noqa: E402  (the case lists and fixture keys)

DEV = 'cuda'
SQRT2 = math.sqrt(2)


def main(out_dir):
    fused, fir = build_ref_ops.load_module('te_ref_fused'), build_ref_ops.load_module('te_ref_upfirdn2d')
    assert fused is not None and fir is not None, 'oracle/_ref is not built (python -m oracle.build_ref_ops)'
    out = {}
    for shape in T.FUSED_SHAPES:
        x, b, g, ggi, ggb = (t.to(DEV) for t in T.fused_inputs(shape))
        empty = x.new_empty(0)
        want = fused.fused_bias_act(x, b, empty, 3, 0, 0.2, SQRT2)
        want_g = fused.fused_bias_act(g, empty, want, 3, 1, 0.2, SQRT2)
        want_gg = fused.fused_bias_act(ggi, ggb, want, 3, 1, 0.2, SQRT2)
        for mode, t in (('fwd', want), ('grad', want_g), ('gradgrad', want_gg)):
            out[T.fused_key(shape, mode)] = np.array(T.digest(t))
    for dtype in T.OTHER_DTYPES:
        x, b, g = (t.to(DEV) for t in T.other_dtype_inputs(dtype))
        empty = x.new_empty(0)
        want = fused.fused_bias_act(x, b, empty, 3, 0, 0.2, SQRT2)
        want_g = fused.fused_bias_act(g, empty, want, 3, 1, 0.2, SQRT2)
        for mode, t in (('fwd', want), ('grad', want_g)):
            out[T.other_dtype_key(dtype, mode)] = np.array(T.digest(t)) if dtype == torch.float64 else t.cpu().numpy()
    for shape, taps, up, down, pad in T.FIR_CASES:
        B, C, H, W = shape
        x = T.fir_input(shape).to(DEV)
        k = O.fir_kernel(taps, float(up * up)).to(DEV)
        # the reference op works on [major, in_h, in_w, minor] with minor = 1 (utils/op/upfirdn2d.py:97, 116-118)
        want = fir.upfirdn2d(x.reshape(-1, H, W, 1), k, up, up, down, down, pad[0], pad[1], pad[2], pad[3])
        want = want.reshape(B, C, want.shape[1], want.shape[2]).cpu()
        base = T.fir_base(shape, taps, up, down, pad)
        key = T.fir_key(shape, taps, up, down, pad)
        if base is None:
            out[key] = want.numpy()
        else:
            out[key + '.ulps'] = T.fir_encode(want, base).numpy()
    torch.cuda.synchronize()
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'reference_kernels.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays)')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden'))

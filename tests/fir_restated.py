"""upfirdn2d restated in fp64 from slices, with the round-off bound of one FIR output: what the GPU tests of the FIR kernels
(tests/test_gpu_loop_trips.py, tests/test_gpu_fir_forms.py through tests/fir_forms.py) compare with.  Plain torch, no library, any device.

    mid = o down + up - 1 - pad0,  i0 = floor(mid / up),  out[o] = sum_t in[i0 + t] kflip[j0 + t up]        (csrc/upfirdn2d.hip)
is the same thing as: insert up - 1 zeros after every sample, pad by pad0 / pad1 zeros (a negative pad crops instead), convolve with the
flipped taps, keep every down-th output.
"""
import torch
import torch.nn.functional as F

from fp64_check import AS32, S32, U32, where64


def _xy(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def fir64(x, k, up=1, down=1, pad=(0, 0, 0, 0)):
    """upfirdn2d of x [..., H, W] (fp64) with taps k [kh, kw]; up / down: one int or (x, y); pad = (px0, px1, py0, py1), a negative pad
    crops that many rows / columns of the zero-inserted image"""
    px0, px1, py0, py1 = pad
    (ux, uy), (dx, dy) = _xy(up), _xy(down)
    H, W = x.shape[-2:]
    if ux > 1 or uy > 1:
        z = x.new_zeros(x.shape[:-2] + (H * uy, W * ux))
        z[..., ::uy, ::ux] = x
        x = z
    x = F.pad(x, (max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)))
    x = x[..., max(-py0, 0):x.shape[-2] - max(-py1, 0), max(-px0, 0):x.shape[-1] - max(-px1, 0)]
    kh, kw = k.shape
    oh, ow = x.shape[-2] - kh + 1, x.shape[-1] - kw + 1
    kf = torch.flip(k, [0, 1])
    out = None
    for a in range(kh):
        for c in range(kw):
            t = x[..., a:a + oh, c:c + ow] * kf[a, c]
            out = t if out is None else out + t
    return out[..., ::dy, ::dx]


def slope64(ref, pos=S32, neg=AS32):
    """the leaky-ReLU gradient factor of a saved output as the two fused blur backward passes apply it: scale, or alpha * scale formed in fp32"""
    return where64(ref > 0, pos, neg)


def fir_bound(absfir, y64, T, gain=1.0, absb=0.0, u=U32):
    """elementwise round-off bound of a FIR output of T taps with bias b and leaky-ReLU gain g: (T + 2) u (|k| * |x| + |b|) g + u |y|
    (derivation: module docstring of tests/test_gpu_loop_trips.py)"""
    return (T + 2) * u * (absfir + absb) * gain + u * y64.abs()

"""Our kernels against the outputs of the REFERENCE's own native kernels (utils/op/fused_bias_act_kernel.cu and
upfirdn2d_kernel.cu, compiled for gfx950 by oracle/build_ref_ops.py and run on the MI355X by oracle/gen_ref_kernels.py, which
stored what they computed in tests/golden/reference_kernels.npz):

* K1 `fused_bias_act` in the three modes the reference's autograd wrapper uses (utils/op/fused_act.py:27-31, 43-45, 54):
  forward with bias, gradient with the saved output as reference, gradient-of-gradient with a bias term - fp32 BIT FOR BIT
  (the fixture holds the SHA-256 of each reference output), half and double through te_bias_act_f16 / _f64 (double bit for
  bit as well, half within one half ulp);
* K2 `upfirdn2d` on the configurations the model uses (blur after the transposed convolution, the discriminator's blurs,
  x2 up / down resampling of the skip paths) and their adjoints, plus odd shapes, crops (negative pads) and non-square taps (the
  fixture keeps each output as its distance in units in the last place from the oracle's fp64 result, see fir_encode);
* the CPU oracle's restatements of both kernels against the real kernels' outputs - which pins the one piece of arithmetic in
  the golden fixtures that was "the oracle's restatement" (fused_bias_act_kernel.cu:26-47 has no CPU twin in the reference).

The case lists, inputs and fixture keys below are shared with oracle/gen_ref_kernels.py."""
import hashlib
import math

import pytest
import torch

from conftest import rel_err
from oracle import te_oracle as O
from transeditor_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SQRT2 = math.sqrt(2)

FUSED_SHAPES = [(4, 64, 32, 32), (2, 7, 5, 3), (16, 512), (3, 33), (2, 128, 64, 64)]
OTHER_DTYPES = [torch.float16, torch.float64]
OTHER_DTYPE_SHAPE = (3, 16, 9, 11)


def digest(t):
    """SHA-256 of a tensor's bytes (dtype and shape spelled in), for bit-for-bit comparisons against a stored output"""
    t = t.detach().contiguous().cpu()
    h = hashlib.sha256(f'{t.dtype}:{tuple(t.shape)}:'.encode())
    h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b'')
    return h.hexdigest()


def fused_key(shape, mode):
    return f'fused.{"x".join(map(str, shape))}.{mode}'


def fused_inputs(shape):
    x = synth.normal(shape, 'refk.x')
    b = 0.5 * synth.normal((shape[1],), 'refk.b')
    g = synth.normal(shape, 'refk.g')
    ggi, ggb = synth.normal(shape, 'refk.ggi'), synth.normal((shape[1],), 'refk.ggb')
    return x, b, g, ggi, ggb


def other_dtype_key(dtype, mode):
    return f'fused.{str(dtype).replace("torch.", "")}.{mode}'


def other_dtype_inputs(dtype):
    shape = OTHER_DTYPE_SHAPE
    return (synth.normal(shape, 'refk.xd').to(dtype), synth.normal((shape[1],), 'refk.bd').to(dtype),
            synth.normal(shape, 'refk.gd').to(dtype))


@pytest.fixture(scope='module')
def ref_out(golden):
    return golden('reference_kernels')


@pytest.mark.parametrize('shape', FUSED_SHAPES)
def test_fused_bias_act_bit_for_bit_vs_reference_kernel(ref_out, shape):
    x, b, g, ggi, ggb = (t.to(DEV) for t in fused_inputs(shape))
    # forward (fused_act.py:54)
    got = _lib.bias_act(x, b, None, 3, 0, 0.2, SQRT2)
    assert digest(got) == str(ref_out[fused_key(shape, 'fwd')])
    want = got                                                          # (= the reference's output, bit for bit)
    # the oracle's restatement, on the CPU, against the real kernel
    orc = O.fused_leaky_relu(x.cpu(), b.cpu(), 0.2, SQRT2)
    assert digest(orc) == str(ref_out[fused_key(shape, 'fwd')]), float((orc - want.cpu()).abs().max())
    # gradient pass (fused_act.py:27-31): grad_output, no bias, the saved OUTPUT as the slope reference
    assert digest(_lib.bias_act(g, None, want, 3, 1, 0.2, SQRT2)) == str(ref_out[fused_key(shape, 'grad')])
    gi, gb = _lib.bias_act_bwd(g, want, 0.2, SQRT2)                   # our single pass: the same values + the bias gradient
    assert digest(gi) == str(ref_out[fused_key(shape, 'grad')])
    want_g = gi
    dims = [0] + list(range(2, len(shape)))
    assert rel_err(gb, want_g.double().sum(dim=dims)) < 1e-5           # (fused_act.py:33-38: grad_input.sum(dim))
    # gradient of the gradient (fused_act.py:43-45): bias term present, slope from the saved output
    assert digest(_lib.bias_act(ggi, ggb, want, 3, 1, 0.2, SQRT2)) == str(ref_out[fused_key(shape, 'gradgrad')])


@pytest.mark.parametrize('dtype', OTHER_DTYPES)
def test_fused_bias_act_other_dtypes_vs_reference_kernel(ref_out, dtype):
    x, b, g = (t.to(DEV) for t in other_dtype_inputs(dtype))
    got = _lib.bias_act(x, b, None, 3, 0, 0.2, SQRT2)
    assert got.dtype == dtype
    if dtype == torch.float64:                                          # bit for bit: the fixture holds the SHA-256
        assert digest(got) == str(ref_out[other_dtype_key(dtype, 'fwd')])
        want = got                                                      # (= the reference's output, bit for bit)
    else:       # half: the reference computes in half, we accumulate in fp32 and round once (te_hip.h): within one half ulp
        want = torch.as_tensor(ref_out[other_dtype_key(dtype, 'fwd')]).to(DEV)
        assert want.dtype == dtype and rel_err(got, want) < 2e-3
    got_g = _lib.bias_act(g, None, want, 3, 1, 0.2, SQRT2)
    if dtype == torch.float64:
        assert digest(got_g) == str(ref_out[other_dtype_key(dtype, 'grad')])
    else:
        assert rel_err(got_g, torch.as_tensor(ref_out[other_dtype_key(dtype, 'grad')]).to(DEV)) < 2e-3


FIR_CASES = [   # (B, C, H, W), taps, up, down, (px0, px1, py0, py1)
    ((2, 8, 33, 33), (1, 3, 3, 1), 1, 1, (1, 1, 1, 1)),       # blur after the transposed convolution (2H+1 -> 2H), :264-266
    ((2, 8, 32, 32), (1, 3, 3, 1), 1, 1, (2, 2, 2, 2)),       # its adjoint / the discriminator's blur before the strided conv
    ((1, 4, 257, 257), (1, 3, 3, 1), 1, 1, (1, 1, 1, 1)),     # the FFHQ-256 top shape
    ((1, 4, 256, 256), (1, 3, 3, 1), 1, 1, (2, 2, 2, 2)),
    ((2, 3, 16, 16), (1, 3, 3, 1), 2, 1, (2, 1, 2, 1)),       # ToRGB skip: Upsample, :103-108
    ((2, 3, 32, 32), (1, 3, 3, 1), 1, 2, (1, 1, 1, 1)),       # its adjoint: Downsample, :124-129
    ((2, 8, 64, 64), (1, 3, 3, 1), 1, 2, (2, 2, 2, 2)),       # blur + every second pixel (discriminator skip branch)
    ((1, 5, 13, 9), (1, 2, 1), 1, 1, (0, 3, 2, 0)),           # odd sizes, 3 taps, asymmetric pads
    ((2, 2, 11, 17), (1, 3, 3, 1), 1, 1, (-1, 2, 1, -2)),     # negative pads = crop
    ((2, 3, 9, 7), (1, 1), 2, 1, (1, 0, 1, 0)),               # x2 up with 2 taps (the reference's mode 4)
    ((2, 3, 18, 14), (1, 1), 1, 2, (0, 0, 0, 0)),             # x2 down with 2 taps (mode 6)
    ((1, 2, 40, 70), (1, 2, 1), 1, 1, (1, 1, 1, 1)),          # 3 taps (mode 2), more than one 16 x 64 tile
]
# (upfirdn2d_kernel.cu:176-215 launches a kernel for exactly six (up, down, taps) classes - the ones above; for any other
# configuration the reference op returns its uninitialised output buffer.  Our generic form, fir_direct_kernel, is checked
# against the oracle in tests/test_gpu_fir_fuzz.py.)


def fir_key(shape, taps, up, down, pad):
    return f'fir.{"x".join(map(str, shape))}.k{"".join(map(str, taps))}.u{up}d{down}.p{"_".join(map(str, pad))}'


def fir_input(shape):
    B, C, H, W = shape
    return synth.normal(shape, f'refk.fir.{H}.{W}')


def fir_base(shape, taps, up, down, pad):
    """the oracle's upfirdn2d in fp64, rounded to fp32 - the base the stored reference outputs are kept relative to; None where the
    oracle cannot express the padding (it takes one (pad0, pad1) pair for both axes)"""
    if not (pad[0] == pad[2] and pad[1] == pad[3]):
        return None
    k = O.fir_kernel(taps, float(up * up)).double()
    return O.upfirdn2d(fir_input(shape).double(), k, up, down, (pad[0], pad[1])).float().contiguous()


def fir_encode(want, base):
    """a reference output as its distance from `base` in units in the last place (int32 difference of the fp32 bit patterns): the
    same information as the values, but mostly small integers, which the compressed fixture stores in a fraction of the bytes"""
    return (want.contiguous().view(torch.int32).long() - base.view(torch.int32).long()).int()


def fir_reference(ref_out, shape, taps, up, down, pad):
    """the reference kernel's output for one FIR case, decoded from the fixture (values, or `.ulps` relative to fir_base).  The
    decoding is exact wherever the fp64 oracle rounds to the same fp32 value as where the fixture was written, and otherwise one
    unit in the last place away - far inside the 1e-6 bar."""
    key = fir_key(shape, taps, up, down, pad)
    if key in ref_out:
        return torch.as_tensor(ref_out[key])
    base = fir_base(shape, taps, up, down, pad)
    return (base.view(torch.int32) + torch.as_tensor(ref_out[key + '.ulps'])).view(torch.float32)


@pytest.mark.parametrize('shape,taps,up,down,pad', FIR_CASES)
def test_upfirdn2d_vs_reference_kernel(ref_out, shape, taps, up, down, pad):
    x = fir_input(shape).to(DEV)
    k = O.fir_kernel(taps, float(up * up)).to(DEV)
    want = fir_reference(ref_out, shape, taps, up, down, pad).to(DEV)
    got = _lib.upfirdn2d_raw(x, k, (up, up), (down, down), pad)
    assert tuple(got.shape) == tuple(want.shape)                      # integer index path: exact
    e = rel_err(got, want)
    assert e < 1e-6, e                                                # same taps, same sums; only the order of the 16 additions may differ
    if pad[0] == pad[2] and pad[1] == pad[3]:                         # the oracle's restatement takes one (pad0, pad1) pair for both axes
        orc = O.upfirdn2d(x.cpu(), k.cpu(), up, down, (pad[0], pad[1]))
        assert tuple(orc.shape) == tuple(want.shape) and rel_err(orc, want) < 1e-6

"""Every form of the fp32 direct convolution kernel (tests/conv_forms.py) against fp64, called directly: conv_pack, then
_lib.conv(x, wp, kind, ...) with the kind given, so that no selector stands between the table and the kernel.  Each test re-asserts
its entry's form through te_conv_form before it compares numbers, so a changed launch constant cannot silently move a case onto
another instantiation.

Reference: stock torch ops in fp64 on the same device - the convolution of tests/conv_routes.py (ref_conv) of x * isc with
w * wscale, then osc, bias, leaky ReLU and gain, then + res, then the mask slope; the constants 0.2, sqrt(2), mask_gain and
0.2 * mask_gain as the fp32 kernel has them.

Bound, elementwise, from the arithmetic.  u = 2^-24, L = taps * Kp products per output (Kp: K padded to the packed layout),
S = |osc| * sum |wscale w| |isc x| + |bias| (the same fp64 ops on absolute values), g = the slope and gain at the element:
    |got - ref| <= (L + 4) u S g + 2 u |y|
L + 1 for the fp32 chain in any order, one rounding each for the style-scale product at staging, osc and bias; slope and gain round y
twice.  A residual add is one more u |y + res|; the mask multiplies all of that by its slope and rounds once more, u |out|.  A
split launch sums its ksplit partial sums in a second kernel: ksplit u S g more.  Not in this list, and not needed by any entry:
the packing rounds wscale * w once (one more u S g would cover it); padded channels contribute exact zeros.  The bound is not tuned;
max err / bound per entry is printed at the end of the module.  Measured on the MI355X, worst entry per kind: 3x3 0.033, S2 0.027,
T2 0.032, 1x1 0.162 (its sums are 9 times shorter, so the worst-case bound is closer to the typical error); left out at most 4.9e-4.

Leaky-ReLU kink: elements whose fp64 pre-activation lies within its own bound, (L + 4 + ksplit) u S, of 0 are left out (the slope may
differ there); at most KINK_CAP = 0.1 % of an entry (tests/fp64_check.py).  The operands come from a CPU generator, so the left-out share is a property
of the table that a CPU run of reference() shows; the large T2 entries have no activation.

Bitwise: a second run gives the same bits; for single-sample forms sample b of the batch launch equals a launch that holds only
sample b, whenever te_conv_form gives both launches the same form key and split count; the entries of conv_forms.DGRAD run again
from the data-gradient pack of the adjoint weight and give the bits of the forward pack.  The last row and last column of the T2
three-region entries are compared on their own first, so a wrong tap mask is named in the failure.
"""
import math

import pytest
import torch

import conv_forms as cf
import conv_routes as cr
import fp64_check
from fp64_check import A32, S32, U32 as U, where64, within
from transeditor_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WSCALE = 0.7
MGAIN = 0.6
OPS = {'3X3': '3x3', 'T2': 'up', 'S2': 'down', '1X1': '1x1'}
KPAD = 16                  # channel padding of the packed layouts; checked against te_conv_packed_numel in _products()
# entries whose first seed leaves more than half the cap on the kink (fp64 reference alone, on the CPU; a 2 x 8 x 3 x 5 output has 240
# elements, so one element there is 0.4 %): the seed is advanced by 100 000 times this
RESEED = {'s2_tc2_gen_multi_split': 1, 's2_tc2_fast_split': 1, 's2_tc2_fast_split_nsv_th': 1}
RESULTS = []
IDS = lambda e: e.name
_report = fp64_check.report_fixture('max err / bound per entry (tests/test_gpu_conv_forms.py):', RESULTS, widths=(44, 10))


def _products(entry):
    """L = taps * Kp, with Kp read off the library's packed size"""
    B, K, M, H, W = entry.shape
    taps = 1 if entry.kind == '1X1' else 9
    Kp = -(-K // KPAD) * KPAD
    numel = _lib.lib().te_conv_packed_numel(_lib.PACK_FWD, M, K, 1 if taps == 1 else 3)
    assert numel % (taps * Kp) == 0 and numel // (taps * Kp) >= M
    return taps * Kp


def operands(entry, device=DEV):
    """the entry's tensors, from a CPU generator seeded by the entry's place in the table (the same values on every machine)"""
    B, K, M, H, W = entry.shape
    op = OPS[entry.kind]
    ks = 1 if entry.kind == '1X1' else 3
    g = torch.Generator().manual_seed(1000 + cf.TABLE.index(entry) + 100000 * RESEED.get(entry.name, 0))
    rn = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float32)
    o = {'x': rn(B, K, *cr.in_hw(op, H, W)), 'w': rn(M, K, ks, ks) / math.sqrt(K * ks * ks), 'bias': rn(M),
         'isc': None, 'osc': None, 'res': None, 'mref': None}
    # biases off zero, of both signs: the window around the kink is as wide as the worst-case bound (1e-3 of S at K = 128), and
    # with pre-activations centred on 0 the smallest entries would leave out more than the cap
    o['bias'] = torch.sign(o['bias']) * (1.0 + 0.5 * o['bias'].abs())
    if entry.has_isc:
        o['isc'] = 1 + 0.5 * rn(B, K)
        o['osc'] = (1 + 0.3 * rn(B, M)).abs() + 0.1
    out_shape = (B, M) + cr.out_hw(op, H, W)
    if entry.epi in ('res', 'both'):
        o['res'] = rn(*out_shape)
    if entry.epi in ('mask', 'both'):
        o['mref'] = rn(*out_shape)
    return {k: (v.to(device) if v is not None else None) for k, v in o.items()}


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def reference(entry, o, ksplit):
    """(y, bound, keep) in fp64 on the operands' device; keep is None without an activation"""
    op = OPS[entry.kind]
    d = lambda t: t.double()
    x, w = d(o['x']), d(o['w']) * WSCALE
    if o['isc'] is not None:
        x = x * d(o['isc'])[:, :, None, None]
    osc = d(o['osc'])[:, :, None, None] if o['osc'] is not None else 1.0
    bias = d(o['bias'])[None, :, None, None]
    pre = cr.ref_conv(op, x, w) * osc + bias
    S = cr.ref_conv(op, x.abs(), w.abs()) * osc + bias.abs()              # (osc > 0 by construction)
    L = _products(entry)
    g = torch.ones_like(pre)
    keep = None
    if entry.act >= 3:
        gain = S32 if entry.act == 3 else 1.0
        g = where64(pre > 0, gain, A32 * gain)
        keep = fp64_check.kink_keep(pre, (L + 4 + (ksplit if ksplit > 1 else 0)) * U * S)
    y = pre * g
    bound = (L + 4) * U * S * g + 2 * U * y.abs()
    if ksplit > 1:
        bound = bound + ksplit * U * S * g
    if o['res'] is not None:
        y = y + d(o['res'])
        bound = bound + U * y.abs()
    if o['mref'] is not None:
        m = where64(d(o['mref']) > 0, _f32(MGAIN), float(torch.tensor(0.2, dtype=torch.float32) * torch.tensor(MGAIN, dtype=torch.float32)))
        y = y * m
        bound = bound * m + U * y.abs()
    return y, bound, keep


def _launch(entry, o, wp, b=None):
    """the entry's launch; b: only sample b"""
    B, K, M, H, W = entry.shape
    s = (lambda t: t) if b is None else (lambda t: None if t is None else t[b:b + 1].contiguous())
    return _lib.conv(s(o['x']), wp, cf.KINDS[entry.kind], M, H, W, isc=s(o['isc']), osc=s(o['osc']), bias=o['bias'], act=entry.act,
                     res=s(o['res']), mask_ref=s(o['mref']), mask_gain=MGAIN, split=bool(entry.with_ws))


def _pack(entry, o, dgrad=False):
    if not dgrad:
        return _lib.conv_pack(o['w'], _lib.PACK_FWD, WSCALE)
    # the weight whose data gradient this convolution is: [Co = K][Ci = M], taps flipped back for the stride-1 kinds
    if entry.kind in ('3X3', '1X1'):
        return _lib.conv_pack(o['w'].flip(2, 3).transpose(0, 1).contiguous(), _lib.PACK_DGRAD, WSCALE)
    return _lib.conv_pack(o['w'].transpose(0, 1).contiguous(), _lib.PACK_SWAP, WSCALE)


def _compare(entry, y, ref, bound, keep, ans, what='y'):
    if ans['nreg'] == 3:
        for name, sl in (('last row', (Ellipsis, slice(-1, None), slice(None))), ('last col', (Ellipsis, slice(None), slice(-1, None)))):
            within(entry.name, f'{what} {name}', y[sl], ref[sl], bound[sl], None if keep is None else keep[sl], results=RESULTS)
    within(entry.name, what, y, ref, bound, keep, results=RESULTS)


@pytest.mark.parametrize('entry', cf.TABLE, ids=IDS)
def test_form_against_fp64(entry):
    ans = cf.check(entry)
    B = entry.shape[0]
    with torch.no_grad():
        o = operands(entry)
        wp = _pack(entry, o)
        y = _launch(entry, o, wp)
        ref, bound, keep = reference(entry, o, ans['ksplit'])
        _compare(entry, y, ref, bound, keep, ans)
        assert torch.equal(y, _launch(entry, o, wp)), f'{entry.name}: a second run gives other bits'
        one = cf.answer(entry.kind, (1,) + entry.shape[1:], entry.has_isc, entry.epi, entry.with_ws)
        if B > 1 and not ans['multi_sample'] and cf.form_of(one) == cf.form_of(ans) and one['ksplit'] == ans['ksplit']:
            for b in sorted({0, B - 1}):
                assert torch.equal(y[b:b + 1], _launch(entry, o, wp, b)), f'{entry.name}: sample {b} of the batch differs from its own launch'


@pytest.mark.parametrize('entry', [cf.BY_NAME[n] for n in cf.DGRAD], ids=IDS)
def test_form_from_the_data_gradient_pack(entry):
    """the same launch fed from PACK_DGRAD / PACK_SWAP of the adjoint weight, against the adjoint reference (which is the forward
    reference of the transposed, flipped weight): the forms do not depend on the pack"""
    ans = cf.check(entry)
    with torch.no_grad():
        o = operands(entry)
        y = _launch(entry, o, _pack(entry, o, dgrad=True))
        ref, bound, keep = reference(entry, o, ans['ksplit'])
        _compare(entry, y, ref, bound, keep, ans, 'dgrad y')
        assert torch.equal(y, _launch(entry, o, _pack(entry, o))), f'{entry.name}: the data-gradient pack gives other bits than the forward pack'


@pytest.mark.parametrize('kind,shape,has_isc,epi', cf.REFUSED, ids=lambda v: str(v).replace(' ', ''))
def test_refused_combinations_raise(kind, shape, has_isc, epi):
    """an epilogue with style scales, or on the strided / transposed kinds: the launch refuses as the query does, nothing runs"""
    e = cf.Form('refused', kind, shape, has_isc, epi, 0, 1, ())
    assert cf.answer(e) == -3
    B, K, M, H, W = shape
    op = OPS[kind]
    x = torch.zeros((B, K) + cr.in_hw(op, H, W), device=DEV)
    w = torch.zeros(M, K, 1 if kind == '1X1' else 3, 1 if kind == '1X1' else 3, device=DEV)
    out = torch.zeros((B, M) + cr.out_hw(op, H, W), device=DEV)
    with pytest.raises(RuntimeError, match='te_conv_res_f32'):
        _lib.conv(x, _lib.conv_pack(w, _lib.PACK_FWD), cf.KINDS[kind], M, H, W, isc=torch.ones(B, K, device=DEV) if has_isc else None,
                  res=out if epi in ('res', 'both') else None, mask_ref=out if epi in ('mask', 'both') else None)

"""The AlexNet LPIPS as a loss on the GPU (transeditor_amd.lpips_alex.AlexLPIPSLoss; pSp/criteria/lpips/lpips.py:29-35 as
pSp/training/coach_new.py:285-320 uses it): te_pool3s2_max_bwd_f32 bit for bit against torch's own max_pool2d backward,
te_alex_stem_dgrad_f32 elementwise against fp64, and the value and the gradient of the whole loss against the fp64 restatement of
tests/lpips_alex_loss_restated.py, at reduced widths on the smallest planes, at the true widths against what the reference's own class
returned (tests/golden/lpips_alex_loss_ref.npz), on the training crop and at 256 px; the bitwise properties.

Accuracy bar of a value (relative error) and of a gradient (rel_l2), against fp64: max(4 x yardstick, 2^-20), the yardstick being the
same formula in plain fp32 torch autograd on the CPU for the same inputs (for the golden case: the reference's own recorded result).
The 4 x margin and the floor are this suite's convention (test_gpu_lpips_alex.py).  No ReLU sign and no pool argmax is pinned.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_alex_loss_restated as LR
import lpips_alex_restated as R
from conftest import ROOT
from fp64_check import SENTINEL, U32 as EPS

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FLOOR = 2.0 ** -20
WIDTHS = (8, 16, 24, 16, 16)


def _bar(yard):
    return max(4 * yard, FLOOR)


# --------------------------------------------------------------------------------------------------------- the pool backwards
POOL_CASES = [(3, 3, 3),                # one window
              (5, 7, 8),                # (8 - 3) % 2 == 1: no window reaches the last column
              (4, 10, 9),               # the last row unreached
              (2, 63, 63),              # the first pool at 256 px; several blocks
              (2, 31, 31)]              # the second one


def _pool_case(case):
    """x = relu(randn) in multiples of 1/4: many ties, many windows that are zero throughout; g integer multiples of 2^-8: every sum of
    up to four of them is exact, so the order of the additions cannot show"""
    planes, H, W = case
    gen = torch.Generator().manual_seed(100 * planes + 10 * H + W)
    x = (torch.relu(torch.randn(1, planes, H, W, generator=gen)) * 4).round() / 4
    g = torch.randint(-512, 513, (1, planes, (H - 3) // 2 + 1, (W - 3) // 2 + 1), generator=gen).float() / 256
    return x, g


@pytest.mark.parametrize('case', POOL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_pool_backward_is_torchs_bit_for_bit(case):
    from transeditor_amd import _lib
    planes, H, W = case
    x, g = _pool_case(case)
    want = LR.pool3s2_max_bwd(g, x)
    u = F.unfold(x.view(planes, 1, H, W), 3, stride=2)                          # [planes, 9, windows]
    ties = float(((u == u.max(1, keepdim=True).values).sum(1) > 1).float().mean())
    gx, gd, xd = torch.full_like(x, SENTINEL).to(DEV), g.to(DEV), x.to(DEV)
    got = _lib.pool3s2_max_bwd(gd, xd)
    assert got.shape == x.shape and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    if H >= 7:
        assert ties > 0.15                                                      # windows whose maximum is held by two or more elements
    if (H - 3) % 2:
        assert bool((got[:, :, H - 1] == 0).all())
    if (W - 3) % 2:
        assert bool((got[:, :, :, W - 1] == 0).all())
    # through the C ABI onto a buffer full of sentinels: every element is written
    _lib._launch('te_pool3s2_max_bwd_f32', gx.data_ptr(), gd.data_ptr(), xd.data_ptr(), planes, H, W)
    assert torch.equal(gx, got)
    assert torch.equal(_lib.pool3s2_max_bwd(gd.expand(2, -1, -1, -1).contiguous(), xd.expand(2, -1, -1, -1).contiguous())[1], got[0])


def test_pool_backward_nan_and_refusals():
    from transeditor_amd import _lib
    x, g = _pool_case((2, 9, 9))
    x[0, 0, 4, 4] = float('nan')                                               # in four windows; torch gives each one's gradient to the NaN
    x[0, 1, 2, 3] = float('nan')
    got = _lib.pool3s2_max_bwd(g.to(DEV), x.to(DEV)).cpu()
    assert torch.equal(got, LR.pool3s2_max_bwd(g, x))
    assert float(got[0, 0, 4, 4]) == float(g[0, 0, 1:3, 1:3].sum())
    gx, gd, xd = torch.full((1, 2, 9, 9), SENTINEL, device=DEV), g.to(DEV), x.to(DEV)
    with pytest.raises(RuntimeError, match='te_pool3s2_max_bwd_f32 failed'):
        _lib._launch('te_pool3s2_max_bwd_f32', gx.data_ptr(), gd.data_ptr(), xd.data_ptr(), 2, 2, 9)
    with pytest.raises(RuntimeError, match='inconsistent shapes'):
        _lib.pool3s2_max_bwd(gd[:, :, :3], xd)
    torch.cuda.synchronize()
    assert bool((gx == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------ the stem's data gradient
STEM_CASES = [(2, 11, 13, 64),          # Ho = 2: every tap row and column at the border
              (3, 33, 30, 72),          # Co past two LDS stages of 32 (72 = 64 + 8); no window reaches column 29
              (1, 256, 256, 64)]        # the true geometry: 63 x 63 -> 256 x 256, the 16-byte stores


def _stem_case(case):
    """g ~ N(0, 1) with half of it masked to 0 (it arrives through a ReLU mask), w ~ N(0, 1)"""
    N, H, W, Co = case
    gen = torch.Generator().manual_seed(sum(p * v for p, v in zip((3, 5, 7, 11), case)) + 1)
    Ho, Wo = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    g = torch.randn(N, Co, Ho, Wo, generator=gen) * (torch.rand(N, Co, Ho, Wo, generator=gen) > 0.5)
    return g, torch.randn(Co, 3, 11, 11, generator=gen)


def _unreached(H, W):
    """[H,W] bool: the pixels no window reaches: every tap k of a row y with y + 2 - k = 4 oy asks for oy >= Ho (and columns likewise)"""
    def axis(n):
        no = (n - 7) // 4 + 1
        return torch.tensor([not any((y + 2 - k) % 4 == 0 and 0 <= (y + 2 - k) // 4 < no for k in range(11)) for y in range(n)])
    return axis(H).view(-1, 1) | axis(W).view(1, -1)


@pytest.fixture(scope='module')
def stem_refs():
    """per case: the inputs, the fp64 gradient, the elementwise bound and torch's own fp32 result on the CPU; computed once"""
    out = {}
    for case in STEM_CASES:
        N, H, W, Co = case
        g, w = _stem_case(case)
        sigma = torch.tensor(R.SIGMA, dtype=torch.float32).view(1, 3, 1, 1)
        want = LR.stem_dgrad(g, w, (H, W))
        bound = (9 * Co + 4) * EPS * LR.stem_dgrad(g.abs(), w.abs(), (H, W))
        op = (H - (4 * g.shape[2] + 3), W - (4 * g.shape[3] + 3))
        cpu32 = F.conv_transpose2d(g, w, None, 4, 2, op) / sigma
        out[case] = dict(g=g, w=w, want=want, bound=bound, cpu32=cpu32)
    return out


@pytest.mark.parametrize('case', STEM_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_stem_gradient_against_fp64(stem_refs, case):
    """|gimg - gimg64| <= (9 Co + 4) 2^-24 (|w|^T |g|) / sigma elementwise: a chain of at most 9 Co products (3 x 3 taps of a phase per
    channel), the division and the fp32 constant; torch's fp32 CPU result meets the same bound.  A pixel no window reaches is exactly 0"""
    from transeditor_amd import _lib
    N, H, W, Co = case
    d = stem_refs[case]
    wt = _lib.alex_stem_dgrad_weight(d['w']).to(DEV)
    got = _lib.alex_stem_dgrad(d['g'].to(DEV), wt, (N, 3, H, W))
    assert got.shape == (N, 3, H, W) and got.dtype == torch.float32 and got.is_contiguous()
    err = (got.cpu().double() - d['want']).abs()
    err_cpu = (d['cpu32'].double() - d['want']).abs()
    live = d['bound'] > 0
    print(f'alex stem dgrad {case}: max err / bound {float((err[live] / d["bound"][live]).max()):.3f} (torch fp32 on the CPU: '
          f'{float((err_cpu[live] / d["bound"][live]).max()):.3f})')
    assert bool((err_cpu <= d['bound']).all())                                  # the yardstick itself
    assert bool((err <= d['bound']).all())
    dead = _unreached(H, W)
    assert bool((got.cpu()[:, :, dead] == 0).all()) and bool((d['want'][:, :, dead] == 0).all())
    assert bool((d['want'][:, :, ~dead] != 0).all())
    if W == 30:
        assert bool(dead[:, 29].all()) and int(dead.sum()) == H
    else:
        assert int(dead.sum()) == 0
    assert torch.equal(got, _lib.alex_stem_dgrad(d['g'].to(DEV), wt, (N, 3, H, W)))                # two runs
    if N > 1:                                                                   # an image's gradient does not depend on its batch
        assert torch.equal(got[1:2], _lib.alex_stem_dgrad(d['g'][1:2].contiguous().to(DEV), wt, (1, 3, H, W)))


def test_stem_gradient_nan_reaches_its_taps_and_refusals():
    from transeditor_amd import _lib
    case = (1, 43, 40, 64)
    g, w = _stem_case(case)
    wt = _lib.alex_stem_dgrad_weight(w).to(DEV)
    clean = _lib.alex_stem_dgrad(g.to(DEV), wt, (1, 3, 43, 40)).cpu()
    assert g.shape == (1, 64, 10, 9)
    oy, ox = 4, 3
    g[0, 5, oy, ox] = float('nan')
    got = _lib.alex_stem_dgrad(g.to(DEV), wt, (1, 3, 43, 40)).cpu()
    y, x = torch.arange(43).view(-1, 1), torch.arange(40).view(1, -1)
    hit = ((4 * oy - 2 <= y) & (y <= 4 * oy + 8) & (4 * ox - 2 <= x) & (x <= 4 * ox + 8)).expand(1, 3, 43, 40)
    assert int(hit[0, 0].sum()) == 11 * 11                                      # the window of output (4, 3): no weight is exactly 0
    assert torch.equal(got.isnan(), hit) and torch.equal(got[~hit], clean[~hit])
    out = torch.full((1, 3, 43, 40), SENTINEL, device=DEV)
    gd = g.to(DEV)
    for N, H, W, Co in [(0, 43, 40, 64), (1, 6, 40, 64), (1, 43, 40, 0)]:
        with pytest.raises(RuntimeError, match='te_alex_stem_dgrad_f32 failed'):
            _lib._launch('te_alex_stem_dgrad_f32', out.data_ptr(), gd.data_ptr(), wt.data_ptr(), N, H, W, Co)
    with pytest.raises(RuntimeError, match='inconsistent shapes'):
        _lib.alex_stem_dgrad(gd, wt, (1, 3, 47, 40))                             # (47 - 7) / 4 + 1 = 11 rows, not g's 10
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_both_kernels_index_past_2_31_elements():
    """the flat indices are 64-bit: the last planes / the last image of a tensor of more than 2^31 elements equal a call on them alone
    bit for bit (a 32-bit index would wrap onto other planes).  8.6 GB per tensor, a few milliseconds of kernel time"""
    from transeditor_amd import _lib
    planes = (1 << 31) // (64 * 64) + 3
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.rand(1, planes, 64, 64, device=DEV, generator=gen)
    g = torch.rand(1, planes, 31, 31, device=DEV, generator=gen)
    assert x.numel() > 1 << 31
    big = _lib.pool3s2_max_bwd(g, x)
    for sl in (slice(0, 2), slice(planes - 2, planes)):
        assert torch.equal(big[:, sl], _lib.pool3s2_max_bwd(g[:, sl].contiguous(), x[:, sl].contiguous()))
    assert float(big[0, -1].abs().sum()) > 0
    del x, g, big
    N = (1 << 31) // (3 * 512 * 512) + 10
    w = torch.randn(8, 3, 11, 11, generator=torch.Generator().manual_seed(6))
    wt = _lib.alex_stem_dgrad_weight(w).to(DEV)
    g = torch.randn(N, 8, 127, 127, device=DEV, generator=gen)
    big = _lib.alex_stem_dgrad(g, wt, (N, 3, 512, 512))
    assert big.numel() > 1 << 31
    for n in (0, N - 1):
        assert torch.equal(big[n:n + 1], _lib.alex_stem_dgrad(g[n:n + 1].contiguous(), wt, (1, 3, 512, 512)))
    assert float(big[-1].abs().sum()) > 0
    del g, big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- the whole loss
@pytest.fixture(scope='module')
def golden_ref():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'lpips_alex_loss_ref.npz'))


@pytest.fixture(scope='module')
def full(golden_ref):
    """true widths, the seeded convolution weights of the golden file and the reference's own heads"""
    from transeditor_amd.lpips_alex import AlexLPIPSLoss
    sd = R.state_dict(LR.GOLDEN['seed'])
    lin = {f'lin{l}.model.1.weight': torch.from_numpy(golden_ref[f'lin{l}']).view(1, -1, 1, 1) for l in range(5)}
    return dict(sd=sd, lin=lin, mod=AlexLPIPSLoss(state_dict=sd, lin_state_dict=lin))


@pytest.fixture(scope='module')
def reduced():
    from transeditor_amd.lpips_alex import AlexLPIPSLoss
    sd, lin = R.state_dict(3, WIDTHS), LR.lin_state_dict(4, WIDTHS)
    return dict(sd=sd, lin=lin, mod=AlexLPIPSLoss(state_dict=sd, lin_state_dict=lin))


def _run(mod, x, y):
    """(value, gradient w.r.t. x) of the library, on the CPU"""
    xin = x.to(DEV).requires_grad_(True)
    v = mod(xin, y.to(DEV))
    assert v.ndim == 0 and v.is_cuda and v.dtype == torch.float32
    v.backward()
    return v.detach().cpu(), xin.grad.cpu()


def _check(name, got, want64, yard):
    """the value's relative error and the gradient's rel_l2 under max(4 x yardstick, 2^-20) each"""
    (v, g), (v64, g64), (yv, yg) = got, want64, yard
    ev, eg = abs(float(v) - float(v64)) / abs(float(v64)), R.rel_l2(g, g64)
    print(f'AlexLPIPSLoss {name}: value {float(v64):.6f}, error {ev:.3e} (yardstick {yv:.3e}, bar {_bar(yv):.3e}); gradient rel_l2 {eg:.3e} '
          f'(yardstick {yg:.3e}, ratio to the bar {eg / _bar(yg):.3f})')
    assert ev <= _bar(yv) and eg <= _bar(yg)
    assert float(g64.abs().max()) > 0 and bool(g.isfinite().all())


def _against_fp64(name, net, x, y):
    v64, g64 = LR.value_and_grad(x, y, net['sd'], net['lin'], torch.float64)
    v32, g32 = LR.value_and_grad(x, y, net['sd'], net['lin'], torch.float32)
    got = _run(net['mod'], x, y)
    _check(name, got, (v64, g64), (abs(float(v32) - float(v64)) / float(v64), R.rel_l2(g32, g64)))
    return got


@pytest.mark.parametrize('H,W', [(31, 31), (45, 39)])
def test_loss_at_reduced_widths_on_the_smallest_planes(reduced, H, W):
    """31 x 31: planes of 7, 3 and 1, the smallest both pools take.  45 x 39: 10 x 9 -> 4 x 4 -> 1 x 1, an unreached edge at each pool
    ((10 - 3) % 2 == 1 and (4 - 3) % 2 == 1)"""
    _against_fp64(f'{H}x{W} widths {WIDTHS}', reduced, R.images(H, 2, H, W), R.images(W + 1, 2, H, W))


def test_loss_against_the_reference_class(full, golden_ref):
    """64 px, B = 3, true widths: the reference's own LPIPS('alex') under torch autograd in fp32 on the CPU is the yardstick"""
    x, y = torch.from_numpy(golden_ref['x']), torch.from_numpy(golden_ref['y'])        # (stored: the recorded run's own bits)
    v64, g64 = torch.from_numpy(golden_ref['v64']), torch.from_numpy(golden_ref['g64'])
    v_ref, g_ref = torch.from_numpy(golden_ref['v_ref']), torch.from_numpy(golden_ref['g_ref'])
    yard = (abs(float(v_ref) - float(v64)) / float(v64), R.rel_l2(g_ref, g64))
    v, g = _run(full['mod'], x, y)
    _check('64 px B=3 (golden)', (v, g), (v64, g64), yard)
    assert R.rel_l2(g, g_ref) <= _bar(yard[1]) + yard[1]                        # against the reference's values: the triangle inequality
    assert full['mod'].widths == R.WIDTHS


def test_loss_on_the_training_crop(full):
    """coach_new.py:303: lpips_loss(inversed[:, :, 35:223, 32:220], real[:, :, 35:223, 32:220]) on a 256 px batch.  The window is not
    contiguous; torch's slicing carries the gradient back, and outside the window it is exactly 0"""
    img, real = R.images(188, 2, 256), R.images(189, 2, 256)
    win = (slice(None), slice(None), slice(35, 223), slice(32, 220))
    v64, g64 = LR.value_and_grad(img[win], real[win], full['sd'], full['lin'], torch.float64)
    v32, g32 = LR.value_and_grad(img[win], real[win], full['sd'], full['lin'], torch.float32)
    xin = img.to(DEV).requires_grad_(True)
    assert not xin[win].is_contiguous()
    v = full['mod'](xin[win], real.to(DEV)[win])
    v.backward()
    g = xin.grad.cpu()
    assert g.shape == img.shape
    outside = torch.ones(256, 256, dtype=torch.bool)
    outside[35:223, 32:220] = False
    assert bool((g[:, :, outside] == 0).all())
    _check('188 px window of 256 px, B=2', (v.detach().cpu(), g[win]), (v64, g64), (abs(float(v32) - float(v64)) / float(v64), R.rel_l2(g32, g64)))


def test_loss_at_256_px(full):
    """the golden seeds at 256 px.  The yardstick is computed here, so it carries whatever branch torch's own fp32 run takes otherwise
    than fp64 (on these images none: 2.0e-6; one ReLU or argmax taken the other way is some 1e-3 of an image's gradient)"""
    G = LR.GOLDEN
    _against_fp64('256 px B=2', full, R.images(G['x_seed'], 2, 256), R.images(G['y_seed'], 2, 256))


def test_loss_properties(full):
    """two runs agree bit for bit; an image's gradient does not depend on its batch (B = 3 scaled by 3 is B = 1 bit for bit: the
    incoming gradient 3 / 3 is exactly 1); y receives no gradient; a second backward raises"""
    mod = full['mod']
    x, y = R.images(LR.GOLDEN['x_seed'], 3, 64).to(DEV), R.images(LR.GOLDEN['y_seed'], 3, 64).to(DEV)

    def grad(xs, ys, factor):
        xin, yin = xs.clone().requires_grad_(True), ys.clone().requires_grad_(True)
        v = mod(xin, yin)
        (v * factor).backward()
        assert yin.grad is None
        return v.detach(), xin.grad
    v3, g3 = grad(x, y, 3.0)
    v3b, g3b = grad(x, y, 3.0)
    assert torch.equal(v3, v3b) and torch.equal(g3, g3b)
    v1, g1 = grad(x[:1], y[:1], 1.0)
    assert torch.equal(g1[0], g3[0]) and float(g1.abs().max()) > 0
    v1c, g1c = grad(x[2:], y[2:], 1.0)
    assert torch.equal(g1c[0], g3[2])
    xin = x.clone().requires_grad_(True)
    v = mod(xin, y)
    v.backward()
    with pytest.raises(RuntimeError, match='second time'):
        v.backward()
    with pytest.raises(RuntimeError, match='AlexLPIPS needs a GPU'):
        mod(x.cpu(), y.cpu())
    with pytest.raises(ValueError, match='max pool'):
        mod(x[:, :, :30], y[:, :, :30])


def test_encoder_loss_backward_on_the_gpu(full):
    """EncoderLoss with the LPIPS term and its crop term on the library, L2 beside it: the sum's gradient is the sum of the terms'.
    The lambdas are powers of two, so a term's gradient is its unit gradient scaled exactly (the incoming gradient enters the kernels
    as a factor); what is left is the order in which autograd adds the three terms: two roundings per element, held to 4 x 2^-24"""
    from transeditor_amd.encoder_loss import EncoderLoss
    img, real = R.images(7, 1, 256).to(DEV), R.images(8, 1, 256).to(DEV)
    z, p = torch.randn(1, 16, 32, device=DEV), torch.randn(1, 16, 32, device=DEV)
    crit = EncoderLoss(lpips_loss=full['mod'], id_lambda=0, l2_lambda=1.0, lpips_lambda=0.5, lpips_lambda_crop=0.25)
    xin = img.clone().requires_grad_(True)
    loss, d, logs = crit(real, xin, z, p)
    loss.backward()
    assert logs is None and list(d) == ['loss_l2', 'loss_lpips', 'loss_lpips_crop', 'loss']
    want = torch.zeros_like(img)
    for lam, win in ((0.5, (slice(None),) * 4), (0.25, (slice(None), slice(None), slice(35, 223), slice(32, 220)))):
        xi = img.clone().requires_grad_(True)
        full['mod'](xi[win], real[win]).backward()
        want += lam * xi.grad
    want += 2 * (img - real) / img.numel()
    assert abs(d['loss'] - (d['loss_l2'] + 0.5 * d['loss_lpips'] + 0.25 * d['loss_lpips_crop'])) <= 4 * EPS * d['loss']
    e = R.rel_l2(xin.grad.cpu(), want.cpu())
    print(f'EncoderLoss gradient against the sum of its terms: rel_l2 {e:.3e}')
    assert e <= 4 * EPS

"""The Inception-v3 pool3 feature extractor of the FID (transeditor_amd.inception_features, csrc/conv2d.hip) against fp64 torch and the
plain-torch restatement (tests/inception_restated.py): the general convolution with its slice writes, batch independence and refusals,
the 3 x 3 pools, the bilinear resize, the whole network, and the metric's plumbing around it."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_restated as R
import scorer_checks
from conftest import ROOT, rel_l2
from fp64_check import SENTINEL, U32 as EPS, kink_keep, within

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---------------------------------------------------------------------------------------------------------- 1. the convolution
# (B, Ci, Co, H, W, kh, kw, s, py, px): every kernel geometry of the network, both strides, odd sizes, a pixel tile that spans images,
# K, channel and pixel tails, Co above one tile
CONV_CASES = [(2, 3, 5, 9, 11, 3, 3, 2, 0, 0), (2, 5, 7, 9, 11, 3, 3, 1, 0, 0), (1, 4, 6, 7, 7, 3, 3, 1, 1, 1),
              (3, 6, 130, 5, 7, 1, 1, 1, 0, 0), (2, 5, 9, 9, 8, 5, 5, 1, 2, 2), (2, 7, 10, 6, 17, 1, 7, 1, 0, 3),
              (2, 7, 10, 17, 6, 7, 1, 1, 3, 0), (2, 8, 8, 8, 8, 1, 3, 1, 0, 1), (2, 8, 8, 8, 8, 3, 1, 1, 1, 0),
              (3, 33, 65, 7, 5, 3, 3, 1, 1, 1), (1, 1, 1, 1, 1, 1, 1, 1, 0, 0), (5, 80, 192, 13, 13, 3, 3, 1, 0, 0)]
SPLITS = 1                       # te_conv2d_f32 does not split K


def _conv_case(case, seed=None):
    """x, w ~ N(0, 1); biases of scale 4 sqrt(K), four times the spread of the products' sum, so that few pre-activations lie near 0
    (on the CPU, torch's fp32 convolution leaves out 0 to 0.02 % of the elements of these cases, below the 0.1 % cap)"""
    B, Ci, Co, H, W, kh, kw = case[:7]
    g = torch.Generator().manual_seed(sum(p * v for p, v in zip((3, 5, 7, 11, 13, 17, 19, 23, 29, 31), case)) if seed is None else seed)
    x, w = torch.randn(B, Ci, H, W, generator=g), torch.randn(Co, Ci, kh, kw, generator=g)
    b = torch.randn(Co, generator=g) * 4 * (Ci * kh * kw) ** 0.5
    return x, w, b


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv2d_against_fp64(case, act):
    """|out - out64| <= (K + S + 2) 2^-24 (|w| * |x| + |bias|) elementwise: the bound of an fp32 chain of K products, S partial sums,
    the bias and the final rounding.  Under ReLU, elements whose fp64 pre-activation is within the bound of 0 are left out, at most
    fp64_check.KINK_CAP = 0.1 % of them.  The share is a property of the seeded operands and the fp64 reference: 18 of 116160 elements,
    1.6e-4, in the last case and none in the eleven others."""
    from transeditor_amd import _lib
    B, Ci, Co, H, W, kh, kw, s, py, px = case
    x, w, b = _conv_case(case)
    K = Ci * kh * kw
    out = _lib.conv2d(x.to(DEV), w.to(DEV), b.to(DEV), s, (py, px), act=act)
    pre = F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=(py, px))
    assert out.shape == pre.shape and out.dtype == torch.float32 and out.is_contiguous()
    bound = (K + SPLITS + 2) * EPS * F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=s, padding=(py, px))
    within(f'conv2d {case} act={act}', f'K={K}', out, torch.relu(pre) if act else pre, bound, kink_keep(pre, bound) if act else None)


# ---------------------------------------------------------------------------------------------------------- 2. slice writes
def test_slice_writes():
    from transeditor_amd import _lib
    g = torch.Generator().manual_seed(40)
    x = torch.randn(2, 6, 9, 11, generator=g).to(DEV)
    x3 = x[:, :3].contiguous()
    w1, b1 = torch.randn(5, 6, 3, 3, generator=g).to(DEV), torch.randn(5, generator=g).to(DEV)
    w2, b2 = torch.randn(7, 6, 1, 7, generator=g).to(DEV), torch.randn(7, generator=g).to(DEV)
    alone = [_lib.conv2d(x, w1, b1, 1, (1, 1), act=1), _lib.conv2d(x, w2, b2, 1, (0, 3), act=0), _lib.pool3(x3, _lib.POOL3_AVG_S1)]
    out = torch.full((2, 17, 9, 11), SENTINEL, device=DEV)
    assert _lib.conv2d(x, w1, b1, 1, (1, 1), act=1, out=out, c0=0) is out
    _lib.conv2d(x, w2, b2, 1, (0, 3), act=0, out=out, c0=5)
    _lib.pool3(x3, _lib.POOL3_AVG_S1, out=out, c0=12)
    assert torch.equal(out[:, :15], torch.cat(alone, 1))
    assert bool((out[:, 15:] == SENTINEL).all())
    # the strided pools shrink the plane: a slice of a [2,17,4,5] tensor
    small = torch.full((2, 17, 4, 5), SENTINEL, device=DEV)
    _lib.pool3(x3, _lib.POOL3_MAX_S2, out=small, c0=14)
    _lib.conv2d(x, w1, b1, 2, (0, 0), act=1, out=small, c0=2)
    assert torch.equal(small[:, 14:], _lib.pool3(x3, _lib.POOL3_MAX_S2)) and torch.equal(small[:, 2:7], _lib.conv2d(x, w1, b1, 2, (0, 0), act=1))
    assert bool((small[:, :2] == SENTINEL).all()) and bool((small[:, 7:14] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- 3. batch independence
def test_conv2d_images_do_not_depend_on_the_batch():
    from transeditor_amd import _lib
    case = (5, 80, 192, 13, 13, 3, 3, 1, 0, 0)
    x, w, b = (t.to(DEV) for t in _conv_case(case, seed=3))
    full = _lib.conv2d(x, w, b, 1, (0, 0), act=1)
    for i in (0, 4):
        assert torch.equal(full[i], _lib.conv2d(x[i:i + 1].contiguous(), w, b, 1, (0, 0), act=1)[0])
    assert torch.equal(full, _lib.conv2d(x, w, b, 1, (0, 0), act=1))                         # two runs
    # a batch large enough for the launch with 128-pixel tiles (at least 512 workgroups): the same bits from the other tile shape
    assert torch.equal(_lib.conv2d(x.repeat(37, 1, 1, 1), w, b, 1, (0, 0), act=1)[180:], full)
    # ... also with a K tail (297, scalar weight loads), a channel tail (65) and images smaller than a tile (35 pixels)
    case = (3, 33, 65, 7, 5, 3, 3, 1, 1, 1)
    x, w, b = (t.to(DEV) for t in _conv_case(case, seed=4))
    few = _lib.conv2d(x, w, b, 1, (1, 1), act=0)
    many = _lib.conv2d(x.repeat(313, 1, 1, 1), w, b, 1, (1, 1), act=0)
    assert torch.equal(many[:3], few) and torch.equal(many[936:], few)


# ---------------------------------------------------------------------------------------------------------- 4. refusals
def test_conv2d_refusals():
    from transeditor_amd import _lib
    L = _lib.lib()
    x, w, b = torch.zeros(2, 3, 9, 9, device=DEV), torch.zeros(4, 3 * 8 * 8, device=DEV), torch.zeros(4, device=DEV)
    out = torch.full((2, 6, 9, 9), SENTINEL, device=DEV)
    st = _lib._stream()

    def call(o=out, xx=x, ww=w, bb=b, B=2, Ci=3, Co=4, H=9, W=9, kh=3, kw=3, s=1, py=1, px=1, Ctot=6, c0=0, act=0):
        ptr = lambda t: None if t is None else t.data_ptr()
        return L.te_conv2d_f32(ptr(o), ptr(xx), ptr(ww), ptr(bb), B, Ci, Co, H, W, kh, kw, s, py, px, Ctot, c0, act, st)
    assert call(s=3) == -3 and call(s=0) == -3
    assert call(kh=8, py=0) == -3 and call(kw=0) == -3
    assert call(py=3) == -2 and call(px=3) == -2 and call(py=-1) == -2
    assert call(H=2, kh=3, py=0) == -2 and call(W=1, kw=5, px=1) == -2                        # Ho < 1, Wo < 1
    assert call(o=None) == -1 and call(xx=None) == -1 and call(ww=None) == -1 and call(bb=None) == -1
    assert call(c0=3) == -2 and call(Ctot=3) == -2 and call(c0=-1) == -2                      # the slice leaves Ctot
    assert call(B=0) == -2 and call(Ci=0) == -2 and call(Co=0) == -2 and call(act=2) == -3
    with pytest.raises(RuntimeError, match='stride must be 1 or 2'):
        _lib.conv2d(x, w[:, :27].reshape(4, 3, 3, 3).contiguous(), b, 3, (1, 1))
    assert L.te_pool3_f32(out.data_ptr(), x.data_ptr(), 2, 3, 9, 9, 3, 6, 0, st) == -3         # no such mode
    assert L.te_pool3_f32(out.data_ptr(), x.data_ptr(), 2, 3, 2, 9, 0, 6, 0, st) == -2         # an unpadded window does not fit
    assert L.te_pool3_f32(out.data_ptr(), x.data_ptr(), 2, 3, 9, 9, 1, 6, 4, st) == -2         # the slice leaves Ctot
    assert L.te_resize_bilinear_f32(out.data_ptr(), x.data_ptr(), 6, 9, 9, 0, 9, st) == -2
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                                     # nothing was launched
    assert call() == 0                                                                       # ... and the same call with valid arguments runs
    torch.cuda.synchronize()
    assert bool((out[:, :4] == 0).all()) and bool((out[:, 4:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- 5. the pools
POOL_SHAPES = [(2, 3, 9, 11), (1, 2, 3, 3), (2, 5, 8, 8), (1, 1, 35, 35)]


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pool3_against_fp64(shape):
    from transeditor_amd import _lib
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)))
    xd = x.to(DEV)
    m2, m1, av = _lib.pool3(xd, _lib.POOL3_MAX_S2), _lib.pool3(xd, _lib.POOL3_MAX_S1), _lib.pool3(xd, _lib.POOL3_AVG_S1)
    assert torch.equal(m2.cpu().double(), F.max_pool2d(x.double(), 3, 2))
    assert torch.equal(m1.cpu().double(), F.max_pool2d(x.double(), 3, 1, 1))
    ref = F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=False)
    e = float((av.double().cpu() - ref).abs().max())
    print(f'pool3 average {shape}: max err {e:.3e}, bar {1e-6 * float(ref.abs().max()):.3e}')
    assert av.shape == ref.shape and e <= 1e-6 * float(ref.abs().max())
    # a NaN propagates to every max window that holds it, and to no other
    xn = x.clone()
    xn[0, 0, shape[2] // 2, shape[3] // 2] = float('nan')
    for mode, args in ((_lib.POOL3_MAX_S2, (3, 2)), (_lib.POOL3_MAX_S1, (3, 1, 1))):
        got, want = _lib.pool3(xn.to(DEV), mode).cpu(), F.max_pool2d(xn, *args)
        assert bool(want.isnan().any()) and torch.equal(got.isnan(), want.isnan())
        assert torch.equal(got[~want.isnan()], want[~want.isnan()])


# ---------------------------------------------------------------------------------------------------------- 6. the resize
RESIZE_SIZES = [((64, 64), (299, 299)), ((256, 256), (299, 299)), ((300, 300), (299, 299)), ((1024, 1024), (299, 299)),
                ((48, 80), (299, 299))]


@pytest.mark.parametrize('src,dst', RESIZE_SIZES, ids=lambda s: 'x'.join(map(str, s)))
def test_resize_bilinear_against_fp64(src, dst):
    """white-noise images: neighbouring samples are unrelated, so an error of the source coordinate reaches the output in full"""
    from transeditor_amd import _lib
    x = torch.rand(2, 3, *src, generator=torch.Generator().manual_seed(src[0] + src[1])) * 2 - 1
    y = _lib.resize_bilinear(x.to(DEV), *dst)
    ref = F.interpolate(x.double(), size=dst, mode='bilinear', align_corners=False)
    e = float((y.double().cpu() - ref).abs().max())
    print(f'resize {src} -> {dst}: max err {e:.3e}, bar {1e-6 * float(ref.abs().max()):.3e}')
    assert y.shape == ref.shape and y.dtype == torch.float32
    assert e <= 1e-6 * float(ref.abs().max())


def test_resize_to_the_same_size_is_a_copy():
    from transeditor_amd import _lib
    x = (torch.rand(2, 3, 299, 299, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(DEV)
    assert torch.equal(_lib.resize_bilinear(x, 299, 299), x)


# ---------------------------------------------------------------------------------------------------------- 7. end to end
E2E_CASES = [(2, 64, 64, True), (2, 107, 91, False)]           # (B, H, W, resize_input)


@pytest.fixture(scope='module')
def weights():
    return R.state_dict(seed=11)


@pytest.fixture(scope='module')
def nets(weights):
    from transeditor_amd.inception_features import InceptionV3Features
    return {True: InceptionV3Features(state_dict=weights), False: InceptionV3Features(state_dict=weights, resize_input=False)}


@pytest.fixture(scope='module')
def e2e(nets, weights):
    """per case: the images, the library's features, the fp64 restatement and the yardstick = rel_l2 of the SAME restatement run by
    torch in fp32 (the reference's arithmetic) against fp64.  Computed once, shared and never modified."""
    out = {}
    for B, H, W, resize in E2E_CASES:
        x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(B * H + W)) * 2 - 1
        ref = R.pool3(x, weights, torch.float64, resize)
        out[(B, H, W, resize)] = dict(x=x.to(DEV), lib=nets[resize](x.to(DEV)), ref=ref,
                                      yard=rel_l2(R.pool3(x, weights, torch.float32, resize), ref))
    return out


@pytest.mark.parametrize('B,H,W,resize', E2E_CASES)
def test_features_end_to_end(nets, e2e, B, H, W, resize):
    """Bar, the project's own from the VGG extractor: 4 x the error of the fp32 torch restatement on the same inputs.  Measured on the
    MI355X (library / fp32 torch): see profiles/README.md, 'Inception-v3 pool3 features'."""
    d = e2e[(B, H, W, resize)]
    assert d['lib'].shape == (B, 2048) and d['lib'].dtype == torch.float32 and d['lib'].is_cuda
    e = rel_l2(d['lib'], d['ref'])
    print(f'InceptionV3Features B={B} {H}x{W} resize={resize}: library {e:.3e}, fp32 torch {d["yard"]:.3e} (rel_l2 against fp64), '
          f'ratio {e / d["yard"]:.2f}')
    assert float(d['ref'].norm()) > 1.0 and float((d['ref'] > 0).double().mean()) > 0.1      # the features are not degenerate
    assert e <= 4 * d['yard']
    assert torch.equal(d['lib'][:1], nets[resize](d['x'][:1]))                                # batch independence is exact here


def test_features_input_checks(nets):
    with pytest.raises(ValueError, match='at least 75'):
        nets[False](torch.zeros(1, 3, 74, 80, device=DEV))
    with pytest.raises(ValueError, match=r'\[B,3,H,W\]'):
        nets[True](torch.zeros(1, 1, 64, 64, device=DEV))
    assert nets[False](torch.zeros(1, 3, 75, 75, device=DEV)).shape == (1, 2048)             # the smallest input: Mixed_7a leaves 1 x 1


# ---------------------------------------------------------------------------------------------------------- 8. the metric's plumbing
@pytest.fixture(scope='module')
def generator():
    return scorer_checks.small_generator(DEV)


def test_fid_with_the_extractor(nets, generator):
    from transeditor_amd import fid
    net = nets[True]
    fake = fid.fake_stats(generator, net, n_sample=20, batch=8, seed=3)                       # batches of 8, 8 and 4
    assert fake.count == 20 and fake.dim == 2048
    again = fid.fake_stats(generator, net, n_sample=20, batch=8, seed=3)
    (m1, c1), (m2, c2) = fake.finalize(), again.finalize()
    assert np.array_equal(m1, m2) and np.array_equal(c1, c2)
    g = torch.Generator().manual_seed(21)
    data = [torch.rand(3, 64, 64, generator=g) * 2 - 1 for _ in range(11)]
    real = fid.dataset_stats(data, net, n_sample=11, batch=4, seed=6)                         # batches of 4, 4 and 3
    assert real.count == 11 and real.dim == 2048
    mr, cr = real.finalize()
    each = net(torch.stack(data).to(DEV)).double().cpu().numpy()                              # any order: the moments are sums
    assert np.allclose(mr, each.mean(0), rtol=1e-9, atol=1e-12) and np.allclose(cr, np.cov(each, rowvar=False), rtol=1e-7, atol=1e-10)
    value = fid.evaluate_fid(generator, net, (mr, cr), n_sample=20, batch=8, seed=3)
    assert isinstance(value, float) and np.isfinite(value) and value >= 0
    assert value == fid.compute_fid((m1, c1), (mr, cr))
    scale = float(np.trace(cr))
    assert abs(fid.compute_fid((mr, cr), (mr, cr))) <= 1e-6 * scale


def test_dropin_equals_the_extractor(weights, nets, tmp_path, monkeypatch):
    os.makedirs(tmp_path / 'hub' / 'checkpoints')
    torch.save(weights, str(tmp_path / 'hub' / 'checkpoints' / 'pt_inception-2015-12-05-6726825d.pth'))
    monkeypatch.setattr(torch.hub, 'get_dir', lambda: str(tmp_path / 'hub'))
    spec = importlib.util.spec_from_file_location('te_dropin_metrics_inception', os.path.join(ROOT, 'dropin', 'metrics', 'inception.py'))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)
    x = (torch.rand(3, 3, 64, 64, generator=torch.Generator().manual_seed(31)) * 2 - 1).to(DEV)
    out = D.InceptionV3([3], normalize_input=False)(x)
    assert isinstance(out, list) and len(out) == 1 and out[0].shape == (3, 2048, 1, 1)
    assert torch.equal(out[0].view(3, -1), nets[True](x))
    unit = (x + 1) / 2                                                                        # normalize_input=True takes (0, 1) images
    assert torch.equal(D.InceptionV3([3], resize_input=True, normalize_input=True)(unit)[0].view(3, -1), nets[True](2 * unit - 1))

"""The VGG16 fc7 feature extractor of the PRDC metric (transeditor_amd.vgg_features, csrc/vggfc.hip, te_vgg_stem_fwd_f32) against fp64
restatements (tests/vgg_restated.py): the weight-streaming fc kernel, its batch independence and refusals, the adaptive average pool,
the stem without the scaling layer, the whole network, and the metric's plumbing around it."""
import pytest
import torch
import torch.nn.functional as F

import lpips_restated as LR
import scorer_checks
import vgg_restated as R
from conftest import rel_l2
from fp64_check import U32 as EPS, kink_keep, within

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ---------------------------------------------------------------------------------------------------------- 1. the fc kernel
FC_SHAPES = [(1, 40, 8), (3, 64, 36), (64, 100, 200), (65, 130, 4096), (5, 4096, 1568)]


def _fc_case(I, J, K, seed):
    """A, W ~ N(0, 1); biases of scale 4 sqrt(K), four times the spread of the products' sum, so that few pre-activations lie near 0"""
    g = torch.Generator().manual_seed(seed)
    a, w = torch.randn(I, K, generator=g), torch.randn(J, K, generator=g)
    b = torch.randn(J, generator=g) * 4 * K ** 0.5
    return a.to(DEV), w.to(DEV), b.to(DEV)


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('I,J,K', FC_SHAPES)
def test_fc_stream_against_fp64(I, J, K, act):
    """|c - c64| <= (K + S + 2) 2^-24 (|A| |W|^T + |bias|): the bound of an fp32 chain of K products, S partial sums, the bias and the
    final rounding.  Under ReLU, elements whose fp64 pre-activation is within the bound of 0 are left out, at most 1 % of them: the
    share is a property of the seeded operands and the fp64 reference, and I = 65, J = 130, K = 4096 (S = 32) leaves out 13 of its 8450
    elements, 1.5e-3, more than the 0.1 % of fp64_check.KINK_CAP.  The other shapes: 3.9e-4 at (5, 4096, 1568), none at the first three."""
    from transeditor_amd import _lib
    a, w, b = _fc_case(I, J, K, 1000 * I + J + K)
    S = _lib.fc_stream_splits(J, K)
    assert S >= 1
    c = _lib.fc_stream(a, w, b, act=act)
    assert c.shape == (I, J) and c.dtype == torch.float32
    pre = a.double() @ w.double().T + b.double()
    bound = (K + S + 2) * EPS * (a.double().abs() @ w.double().abs().T + b.double().abs())
    within(f'fc_stream I={I} J={J} K={K} act={act}', f'S={S}', c, torch.relu(pre) if act else pre, bound, kink_keep(pre, bound) if act else None,
           cap=0.01)


# ---------------------------------------------------------------------------------------------------------- 2. batch independence
def test_fc_stream_rows_do_not_depend_on_the_batch():
    from transeditor_amd import _lib
    a, w, b = _fc_case(65, 130, 4096, 3)
    c65 = _lib.fc_stream(a, w, b, act=1)
    c64 = _lib.fc_stream(a[:64].contiguous(), w, b, act=1)
    assert torch.equal(_lib.fc_stream(a[:3].contiguous(), w, b, act=1), c64[:3])
    assert torch.equal(c65[:64], c64)
    assert torch.equal(_lib.fc_stream(a[64:65].contiguous(), w, b, act=1), c65[64:65])      # the row that has a block of its own
    assert torch.equal(_lib.fc_stream(a, w, b, act=1), c65)                                # two runs
    # the split is a function of the weight's shape: the ABI has no batch argument to give it
    L = _lib.lib()
    assert len(L.te_fc_stream_splits.argtypes) == 2
    assert L.te_fc_stream_ws_bytes(65, 130, 4096) == 65 * 130 * 4 * _lib.fc_stream_splits(130, 4096)
    assert L.te_fc_stream_ws_bytes(1, 130, 4096) == 130 * 4 * _lib.fc_stream_splits(130, 4096)


# ---------------------------------------------------------------------------------------------------------- 3. refusals
def test_fc_stream_refusals():
    from transeditor_amd import _lib
    L = _lib.lib()

    def z(*shape):
        return torch.zeros(*shape, device=DEV)
    for a, w, b in [(z(3, 6), z(4, 6), z(4)),            # K = 6
                    (z(3, 0), z(4, 0), z(4)),            # K = 0
                    (z(3, 8), z(0, 8), z(0)),            # J = 0
                    (z(0, 8), z(4, 8), z(4))]:           # I = 0
        with pytest.raises(RuntimeError, match='te_fc_stream_f32 failed'):
            _lib.fc_stream(a, w, b)
    buf = z(3 * 8 + 1)
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        _lib.fc_stream(buf[1:].view(3, 8), z(4, 8), z(4))
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        _lib.fc_stream(z(3, 8), z(4 * 8 + 1)[1:].view(4, 8), z(4))
    a, w, b, c, ws = z(3, 8), z(4, 8), z(4), z(3, 4), z(3 * 4)
    st = _lib._stream()
    assert L.te_fc_stream_f32(c.data_ptr(), ws.data_ptr(), a.data_ptr(), None, b.data_ptr(), 3, 4, 8, 0, st) == -1
    with pytest.raises(RuntimeError, match='NULL'):
        _lib._check(L.te_fc_stream_f32(None, ws.data_ptr(), a.data_ptr(), w.data_ptr(), b.data_ptr(), 3, 4, 8, 0, st), 'te_fc_stream_f32')
    assert L.te_fc_stream_f32(c.data_ptr(), ws.data_ptr(), a.data_ptr(), w.data_ptr(), b.data_ptr(), 3, 4, 6, 0, st) == -2
    assert L.te_fc_stream_f32(c.data_ptr(), ws.data_ptr(), a.data_ptr(), w.data_ptr(), b.data_ptr(), 3, 4, 8, 2, st) == -3
    with pytest.raises(RuntimeError, match='te_fc_stream_splits'):
        _lib.fc_stream_splits(4, 6)
    assert L.te_fc_stream_ws_bytes(0, 4, 8) < 0 and L.te_fc_stream_ws_bytes(3, 0, 8) < 0 and L.te_fc_stream_ws_bytes(3, 4, 0) < 0
    torch.cuda.synchronize()
    assert float(c.abs().max()) == 0.0                   # nothing was launched


# ---------------------------------------------------------------------------------------------------------- 4. the adaptive pool
@pytest.mark.parametrize('H,W', [(7, 7), (8, 8), (1, 1), (2, 2), (4, 4), (32, 32), (8, 16), (5, 9)])
def test_adaptive_avgpool_against_fp64(H, W):
    from transeditor_amd import _lib
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H * 100 + W))          # 6 planes
    y = _lib.adaptive_avgpool(x.to(DEV))
    assert y.shape == (2, 3, 7, 7) and y.is_contiguous()
    ref = F.adaptive_avg_pool2d(x.double(), 7)
    assert float((y.double().cpu() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    if (H, W) == (7, 7):
        assert torch.equal(y.cpu(), x)


# ---------------------------------------------------------------------------------------------------------- 5. the stem
@pytest.mark.parametrize('N,H,W', [(2, 16, 16), (1, 32, 48)])
def test_vgg_stem_against_fp64(N, H, W):
    """the tolerances of tests/test_gpu_lpips.py::test_stem_forward_and_data_gradient"""
    from transeditor_amd import _lib
    sd = R.conv_state_dict(3)
    w, b = sd['features.0.weight'], sd['features.0.bias']
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(7 + N)) * 2 - 1
    y = _lib.vgg_stem_fwd(x.to(DEV), w.to(DEV), b.to(DEV))
    ref = torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    assert y.shape == (N, 64, H, W)
    assert rel_l2(y, ref) < 1e-6
    assert float((y.double().cpu() - ref)[:, :, 0].abs().max()) < 1e-5                       # first row (padding side)


def test_lpips_stem_is_untouched(tmp_path):
    from transeditor_amd import _lib
    from transeditor_amd.lpips import PerceptualLoss
    vp, lp = LR.write_weights(tmp_path)
    percept = PerceptualLoss(vgg_path=vp, lin_path=lp)
    x = (torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(DEV)
    y = _lib.lpips_stem_fwd(x, percept.w0, percept.b0)
    assert torch.equal(y, percept._trunk(x)[0])
    assert not torch.equal(y, _lib.vgg_stem_fwd(x, percept.w0, percept.b0))                   # the two stems are different layers
    vgg = {k: v.double() for k, v in torch.load(vp).items()}
    ref = torch.relu(F.conv2d((x.double().cpu() - LR.SHIFT.double().view(1, 3, 1, 1)) / LR.SCALE.double().view(1, 3, 1, 1),
                              vgg['features.0.weight'], vgg['features.0.bias'], padding=1))
    assert rel_l2(y, ref) < 1e-6


# ---------------------------------------------------------------------------------------------------------- 6. end to end
E2E_SHAPES = [(3, 64, 64), (2, 96, 160)]        # pool5 2 x 2 (smaller than 7 x 7) and 3 x 5 (not square)


@pytest.fixture(scope='module')
def net():
    from transeditor_amd.vgg_features import VGG16Features
    sd = R.full_state_dict(seed=11, device=DEV)
    return VGG16Features(state_dict=sd), sd


@pytest.fixture(scope='module')
def e2e(net):
    """per shape: the images, the library's features, the fp64 restatement and the yardstick = rel_l2 of the SAME restatement run by
    torch in fp32 (the reference's arithmetic) against fp64.  Computed once, shared and never modified."""
    vgg, sd = net
    out = {}
    for B, H, W in E2E_SHAPES:
        x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(B * H + W)) * 2 - 1
        ref = R.fc7(x, sd, torch.float64)
        out[(B, H, W)] = dict(x=x.to(DEV), lib=vgg(x.to(DEV)), ref=ref, yard=rel_l2(R.fc7(x, sd, torch.float32), ref))
    return out


@pytest.mark.parametrize('B,H,W', E2E_SHAPES)
def test_features_end_to_end(net, e2e, B, H, W):
    """Bar: 4 x the error of the fp32 torch restatement on the same inputs (the split convolution routes and the split-K sums reorder
    the additions).  Measured on the MI355X (library / fp32 torch): see profiles/README.md, 'VGG16 fc7 features'."""
    vgg, _ = net
    d = e2e[(B, H, W)]
    assert d['lib'].shape == (B, 4096) and d['lib'].dtype == torch.float32 and d['lib'].is_cuda
    e = rel_l2(d['lib'], d['ref'])
    print(f'VGG16Features B={B} {H}x{W}: library {e:.3e}, fp32 torch {d["yard"]:.3e} (rel_l2 against fp64), ratio {e / d["yard"]:.2f}')
    assert float(d['ref'].norm()) > 1.0 and float((d['ref'] > 0).double().mean()) > 0.1      # the features are not degenerate
    assert e <= 4 * d['yard']
    one = vgg(d['x'][:1])
    e1 = rel_l2(d['lib'][:1], one)
    print(f'    first row of the batch against a batch of one: {e1:.3e}')
    assert e1 <= 4 * d['yard']


def test_features_input_checks(net):
    vgg, _ = net
    with pytest.raises(ValueError, match='multiples of 32'):
        vgg(torch.zeros(1, 3, 48, 64, device=DEV))
    with pytest.raises(ValueError, match=r'\[B,3,H,W\]'):
        vgg(torch.zeros(1, 1, 64, 64, device=DEV))


# ---------------------------------------------------------------------------------------------------------- 7. the metric's plumbing
@pytest.fixture(scope='module')
def generator():
    return scorer_checks.small_generator(DEV)


def test_evaluate_prdc_with_the_extractor(net, generator):
    from transeditor_amd import prdc
    vgg, _ = net
    real = torch.randn(24, 4096, generator=torch.Generator().manual_seed(1)).abs().to(DEV)
    fake = prdc.fake_features(generator, vgg, n_sample=20, batch=8, seed=3)                   # batches of 8, 8 and 4
    assert fake.shape == (20, 4096) and fake.is_cuda
    assert torch.equal(fake, prdc.fake_features(generator, vgg, n_sample=20, batch=8, seed=3))
    res = prdc.evaluate_prdc(generator, vgg, real, n_sample=20, batch=8, nearest_k=3, seed=3)
    assert res == prdc.compute_prdc(real, fake, 3)
    assert set(res) == set(prdc.KEYS)


def test_dataset_features(net, e2e):
    from transeditor_amd import prdc
    vgg, _ = net
    g = torch.Generator().manual_seed(21)
    data = [torch.rand(3, 64, 64, generator=g) * 2 - 1 for _ in range(11)]
    f = prdc.dataset_features(data, vgg, n_sample=11, batch=4, seed=6)                        # batches of 4, 4 and 3
    assert f.shape == (11, 4096) and f.is_cuda and f.dtype == torch.float32
    assert torch.equal(f, prdc.dataset_features(data, vgg, n_sample=11, batch=4, seed=6))
    each = vgg(torch.stack(data).to(DEV))
    a, b = f.double().norm(dim=1).sort().values, each.double().norm(dim=1).sort().values
    assert float(((a - b).abs() / b).max()) <= 4 * e2e[(3, 64, 64)]['yard']                   # a permutation of the per-item features
    assert not torch.equal(f, each)                                                           # ... and not the identity
    head = prdc.dataset_features(data, vgg, n_sample=5, batch=4, seed=6)
    assert head.shape == (5, 4096)
    assert rel_l2(head, f[:5]) <= 4 * e2e[(3, 64, 64)]['yard']

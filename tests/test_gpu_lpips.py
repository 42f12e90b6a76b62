"""LPIPS-VGG (transeditor_amd.lpips, csrc/lpips.hip) and the noise regulariser (op/noisereg.py, csrc/noisereg.hip) against fp64
plain-torch restatements of the reference (tests/lpips_restated.py)."""
import pytest
import torch

import lpips_restated as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def nets(tmp_path_factory):
    from transeditor_amd.lpips import PerceptualLoss
    vp, lp = R.write_weights(tmp_path_factory.mktemp('lpips'))
    vgg = {k: v.double() for k, v in torch.load(vp).items()}
    lin = {k: v.double() for k, v in torch.load(lp).items()}
    return PerceptualLoss(vgg_path=vp, lin_path=lp), vgg, lin


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize('size,n,nt', [(64, 1, 1), (64, 2, 2), (64, 4, 4), (64, 4, 1), (256, 1, 1), (256, 2, 2), (256, 4, 1)])
def test_lpips_distance_and_gradient(nets, size, n, nt):
    percept, vgg, lin = nets
    g = torch.Generator().manual_seed(size + 10 * n + nt)
    pred = (torch.rand(n, 3, size, size, generator=g) * 2 - 1)
    target = (torch.rand(nt, 3, size, size, generator=g) * 2 - 1)
    pd = pred.to(DEV).requires_grad_(True)
    d = percept(pd, target.to(DEV))
    assert d.shape == (n, 1, 1, 1)
    w = torch.rand(n, generator=g) + 0.5
    (d.view(-1) * w.to(DEV)).sum().backward()
    p64 = pred.double().requires_grad_(True)
    ref = R.lpips(p64, target.double(), vgg, lin)
    (ref.view(-1) * w.double()).sum().backward()
    e_d = float(((d.detach().double().cpu() - ref.detach()).abs() / ref.detach().abs()).max())
    e_g = _rel(pd.grad, p64.grad)
    print(f'LPIPS {size}^2 N={n} Nt={nt}: distance rel err {e_d:.2e}, gradient rel L2 {e_g:.2e}')
    # observed on the MI355X: distance <= 4.2e-7 at both sizes; gradient 3.8e-6 at 64^2, 1.3e-3 .. 2.0e-3 at 256^2.  The 256^2 figure is
    # the fp32 conditioning of the loss, not a kernel defect: each trunk convolution matches fp64 to < 1e-6 at these shapes on its own,
    # and the same restatement in plain fp32 torch (CPU, same seeds and weights) is 8.2e-4 / 1.1e-3 / 1.7e-3 off fp64 for the three
    # 256^2 cases (ReLU and max-pool decisions that flip between fp32 and fp64 reroute whole gradient paths)
    assert e_d < 1e-6 and e_g < (1e-5 if size == 64 else 3e-3)


def test_cached_target_is_bit_identical_and_self_distance_zero(nets):
    percept = nets[0]
    g = torch.Generator().manual_seed(5)
    pred = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    target = (torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    tf = percept.target_features(target)
    a, b = percept(pred, target), percept(pred, tf)
    assert torch.equal(a, b)
    pa, pb = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    percept(pa, target).sum().backward()
    percept(pb, tf).sum().backward()
    assert torch.equal(pa.grad, pb.grad)
    assert float(percept(target, target).abs().max()) == 0.0


def test_cached_target_broadcast_against_fp64(nets):
    """the cached path itself against the restatement: one target (batch 1) through the trunk once, three preds"""
    percept, vgg, lin = nets
    g = torch.Generator().manual_seed(17)
    pred = torch.rand(3, 3, 64, 64, generator=g) * 2 - 1
    target = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    tf = percept.target_features(target.to(DEV))
    pd = pred.to(DEV).requires_grad_(True)
    d = percept(pd, tf)
    d.sum().backward()
    p64 = pred.double().requires_grad_(True)
    ref = R.lpips(p64, target.double(), vgg, lin)
    ref.sum().backward()
    assert d.shape == (3, 1, 1, 1)
    assert float(((d.detach().double().cpu() - ref.detach()).abs() / ref.detach().abs()).max()) < 1e-6
    assert _rel(pd.grad, p64.grad) < 1e-5


def test_stem_forward_and_data_gradient(nets):
    from transeditor_amd import _lib
    percept, vgg = nets[0], nets[1]
    g = torch.Generator().manual_seed(7)
    x = torch.rand(2, 3, 32, 48, generator=g) * 2 - 1
    y = _lib.lpips_stem_fwd(x.to(DEV), percept.w0, percept.b0)
    x64 = x.double().requires_grad_(True)
    w, b = vgg['features.0.weight'], vgg['features.0.bias']
    # scaling BEFORE the zero padding: the border pixels see zeros, not (0 - shift) / scale
    ref = torch.relu(torch.nn.functional.conv2d((x64 - R.SHIFT.double().view(1, 3, 1, 1)) / R.SCALE.double().view(1, 3, 1, 1), w, b,
                                                padding=1))
    assert _rel(y, ref) < 1e-6
    assert float((y.double().cpu() - ref.detach())[:, :, 0].abs().max()) < 1e-5          # first row (padding side)
    gy = torch.randn(ref.shape, generator=g)
    ref.backward(gy.double())
    gx = _lib.lpips_stem_dgrad(gy.to(DEV), y, percept.w0)
    assert _rel(gx, x64.grad) < 1e-6
    assert float((gx.double().cpu() - x64.grad)[:, :, :, -1].abs().max()) <= 1e-5 * float(x64.grad.abs().max())


def test_maxpool_ties_and_nan():
    from transeditor_amd import _lib
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 8, 8, generator=g)
    x[0, 0, 0, 0] = x[0, 0, 0, 1] = x[0, 0, 1, 0] = 5.0              # tie: the first in row-major order wins
    x[0, 1, 2, 3] = x[0, 1, 3, 2] = 4.0
    x[1, 2, 4, 4] = float('nan')
    xd = x.to(DEV)
    y = _lib.maxpool2_fwd(xd)
    xr = x.clone().requires_grad_(True)
    ref = torch.nn.functional.max_pool2d(xr, 2, 2)
    assert torch.allclose(y.cpu(), ref.detach(), equal_nan=True, rtol=0, atol=0)
    assert torch.isnan(y[1, 2, 2, 2])
    gy = torch.randn(ref.shape, generator=g)
    ref.backward(gy)
    gx = _lib.maxpool2_bwd(gy.to(DEV), xd)
    assert torch.equal(gx.cpu(), xr.grad)
    assert gx[0, 0, 0, 0] == gy[0, 0, 0, 0] and gx[0, 0, 0, 1] == 0 and gx[0, 0, 1, 0] == 0


def test_head_backward_zero_norm_pixel_and_autograd():
    from transeditor_amd import _lib
    g = torch.Generator().manual_seed(11)
    N, C, H, W = 2, 64, 8, 8
    f = torch.randn(N, C, H, W, generator=g)
    f[1, :, 3, 5] = 0.0                                              # a zero-norm pixel
    t = torch.randn(1, C, H, W, generator=g)
    w = torch.rand(C, generator=g)
    gd = torch.rand(N, generator=g) + 0.5
    th = _lib.lpips_normalize(t.to(DEV))
    gf = _lib.lpips_head_bwd(gd.to(DEV), f.to(DEV), th, w.to(DEV), gin=None, relu_mask=False).cpu().double()
    # autograd of the reference formula (fp64) everywhere but the planted pixel (NaN there, sqrt backward 0/0)
    f64 = f.double().requires_grad_(True)
    th64 = R.normalize_tensor(t.double())
    d = ((R.normalize_tensor(f64) - th64) ** 2 * w.double().view(1, C, 1, 1)).sum(1).mean([1, 2])
    (d * gd.double()).sum().backward()
    assert torch.isnan(f64.grad[1, :, 3, 5]).all()
    mask = torch.ones(N, H, W, dtype=torch.bool)
    mask[1, 3, 5] = False
    a, b = gf.permute(0, 2, 3, 1)[mask], f64.grad.permute(0, 2, 3, 1)[mask]
    assert float((a - b).norm() / b.norm()) < 1e-5
    u = 2 * w.double() * (0 - th.cpu().double()[0, :, 3, 5]) * gd.double()[1] / (H * W)
    lim = u / 1e-10
    assert torch.isfinite(gf[1, :, 3, 5]).all()
    assert float(((gf[1, :, 3, 5] - lim).abs() / lim.abs().clamp_min(1e-30)).max()) < 1e-5
    # the head's forward against the same formula
    part = _lib.lpips_head_fwd(f.to(DEV), th, w.to(DEV))
    dd = _lib.lpips_dist([part], [H * W])
    assert _rel(dd, d.detach()) < 1e-6


@pytest.mark.parametrize('batch', [1, 3])
def test_noise_regularize_and_normalize(batch):
    from transeditor_amd.op.noisereg import noise_normalize_, noise_regularize
    maps = R.noise_list(256, batch, 100 + batch)
    assert len(maps) == 13
    dm = [m.to(DEV).requires_grad_(True) for m in maps]
    loss = noise_regularize(dm)
    loss.backward(torch.tensor(2.5, device=DEV))
    m64 = [m.double().requires_grad_(True) for m in maps]
    ref = R.noise_regularize(m64)
    (2.5 * ref).backward()
    assert abs(float(loss) - float(ref)) <= 1e-4 * abs(float(ref))
    for a, b in zip(dm, m64):
        assert _rel(a.grad, b.grad) < 1e-4
    # a second forward reproduces the first bit for bit
    assert torch.equal(noise_regularize(dm), loss)
    nm = [m.to(DEV) for m in maps]
    noise_normalize_(nm)
    for a, b in zip(nm, R.noise_normalize([m.double() for m in maps])):
        assert float((a.cpu().double() - b).abs().max()) < 1e-5

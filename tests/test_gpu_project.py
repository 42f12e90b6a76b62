"""The projector (transeditor_amd.project): one step's gradients against fp64 autograd through the CPU oracle, convergence and
determinism of a 200-step run, and the CLI end to end (projector_optimization.py:83-276)."""
import os

import numpy as np
import pytest
import torch

import lpips_restated as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZE = 64


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from transeditor_amd import synth
    from transeditor_amd.lpips import PerceptualLoss
    from transeditor_amd.model_spatial_query import Generator
    tmp = tmp_path_factory.mktemp('proj')
    vp, lp = R.write_weights(tmp, seed=1)
    G = Generator(SIZE, 512, 512, 2 * (int(np.log2(SIZE)) - 1), n_trans=8, pixel_norm_op_dim=1)
    sd = G.state_dict()
    synth.fill_state_dict(sd, 21)
    G.load_state_dict(sd)
    G = G.to(DEV)
    return dict(G=G, sd=sd, percept=PerceptualLoss(vgg_path=vp, lin_path=lp), vgg=vp, lin=lp, tmp=tmp,
                vgg_sd={k: v.double() for k, v in torch.load(vp).items()}, lin_sd={k: v.double() for k, v in torch.load(lp).items()})


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize('use_noise', [False, True])
def test_one_step_gradients_match_fp64_oracle(setup, use_noise):
    from oracle import te_oracle as O
    from transeditor_amd.project import step_loss
    G, percept = setup['G'], setup['percept']
    B = 2
    g = torch.Generator().manual_seed(3 + use_noise)
    z = torch.randn(B, 512, 16, generator=g)
    p = torch.randn(B, 512, 16, generator=g)
    target = torch.rand(1, 3, SIZE, SIZE, generator=g) * 2 - 1
    noises = R.noise_list(SIZE, B, 9)
    a = dict(use_noise=use_noise, noise_regularize=1e5, mse=0.3)
    flags = [q.requires_grad for q in G.parameters()]
    for q in G.parameters():
        q.requires_grad_(False)
    try:
        zd, pd = z.to(DEV).requires_grad_(True), p.to(DEV).requires_grad_(True)
        nd = [n.to(DEV).requires_grad_(use_noise) for n in noises]
        loss, p_loss, n_loss, mse_loss = step_loss(G, zd, pd, nd, percept, percept.target_features(target.to(DEV)), target.to(DEV), a)
        loss.backward()
    finally:
        for q, f in zip(G.parameters(), flags):
            q.requires_grad_(f)
    assert all(q.grad is None for q in G.parameters())
    P = {k: v.double() for k, v in setup['sd'].items()}
    z64, p64 = z.double().requires_grad_(True), p.double().requires_grad_(True)
    n64 = [n.double().requires_grad_(use_noise) for n in noises]
    img, _, _ = O.generator_forward(P, z64, p64, SIZE, pixel_norm_dim=1, use_spatial_mapping=False, use_style_mapping=False)
    ref = R.lpips(img, target.double(), setup['vgg_sd'], setup['lin_sd']).sum() + 0.3 * (img - target.double()).pow(2).mean()
    if use_noise:
        ref = ref + 1e5 * R.noise_regularize(n64)
    ref.backward()
    e = (_rel(zd.grad, z64.grad), _rel(pd.grad, p64.grad))
    print(f'one projector step (use_noise={use_noise}): d latent_in {e[0]:.2e}, d param_in {e[1]:.2e}')
    assert max(e) < 1e-4          # observed 4.8e-6 .. 2.7e-5
    if use_noise:
        for a_, b_ in zip(nd, n64):
            assert _rel(a_.grad, b_.grad) < 1e-4


def test_projection_converges_and_is_deterministic(setup):
    from transeditor_amd.project import project
    G, percept = setup['G'], setup['percept']
    flags = [q.requires_grad for q in G.parameters()]
    g = torch.Generator().manual_seed(5)
    z, p = torch.randn(1, 512, 16, generator=g).to(DEV), torch.randn(1, 512, 16, generator=g).to(DEV)
    with torch.no_grad():
        target = G(z, p, use_spatial_mapping=False, use_style_mapping=False)[0].clamp(-1, 1)
    kw = dict(step=200, batch=1, n_mean_latent=1000, seed=7)
    r1 = project(G, target, percept, **kw)
    r2 = project(G, target, percept, **kw)
    pt = r1['perceptual'][0].cpu()
    print(f'perceptual loss: first record {float(pt[0]):.4f}, last {float(pt[-1]):.4f}')
    assert float(pt[-1]) < 0.5 * float(pt[0])
    assert torch.equal(r1['latent'], r2['latent']) and torch.equal(r1['param'], r2['param'])
    assert r1['latent'].shape == (1, 512, 16) and r1['image'].shape == (1, 3, SIZE, SIZE)
    assert [q.requires_grad for q in G.parameters()] == flags
    assert all(q.grad is None for q in G.parameters())


def test_cli_end_to_end(setup):
    from PIL import Image
    from transeditor_amd import project as P
    tmp = setup['tmp']
    ck = tmp / 'ckpt'
    ck.mkdir()
    torch.save({'g_ema': setup['sd']}, str(ck / 'tiny.pt'))
    data = tmp / 'images'
    data.mkdir()
    rng = np.random.RandomState(0)
    for name in ('b.png', 'a.png'):
        Image.fromarray(rng.randint(0, 255, (96, 96, 3), dtype=np.uint8)).save(str(data / name))
    out = P.main(['--ckpt', str(ck / 'tiny.pt'), '--dataset_dir', str(data), '--size', str(SIZE), '--step', '100', '--batch', '2',
                  '--vgg16', setup['vgg'], '--lpips_lin', setup['lin'], '--output_dir', str(tmp / 'out')])
    for f in ('origin_0.png', 'origin_1.png', 'project_0.png', 'project_1.png'):
        assert os.path.exists(os.path.join(out, f))
        assert Image.open(os.path.join(out, f)).size == (SIZE, SIZE)
    assert np.load(os.path.join(out, 'latents.npy')).shape == (4, 512, 16)
    assert np.load(os.path.join(out, 'param.npy')).shape == (4, 512, 16)
    for f in ('perceptual.npy', 'noise.npy', 'mse.npy'):
        assert np.load(os.path.join(out, f)).shape == (2,)

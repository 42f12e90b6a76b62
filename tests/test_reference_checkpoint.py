"""(f.4) A checkpoint laid out as the reference's training loop writes it goes through our restore path.

The layout comes from the reference's own classes: tests/golden/reference_checkpoint32_schema.npz holds the state_dict keys, shapes
and dtypes and the parameter order of the reference's `Generator` / `Discriminator` (model_spatial_query.py) at 32 px with 8 tokens
(oracle/gen_golden.py::gen_checkpoint_schema).  The test fills that layout with seeded values, sets up two `optim.Adam` over the
parameters in the reference's order exactly as train_spatial_query.py:458-473 does, takes one optimiser step each so that the state
exists, and saves the dictionary of :361-371 (`g`, `d`, `g_ema`, `g_optim`, `d_optim`) with torch.save under an iteration-numbered
name.  Our side: drop-in modules + `FusedAdam`, restored with `train_step.load_checkpoint_into` (the body of
`TrainStep.load_checkpoint`): strict state_dict load (every key, every shape), identical tensors afterwards, optimiser
hyper-parameters and per-parameter state identical, start iteration parsed from the file name; a 'g_ema'-only file (the published
inference checkpoints, test_spatial_query.py:285) loads into the EMA generator alone.  CPU only - nothing is computed."""
import os
from collections import OrderedDict

import torch

SIZE, TOKEN = 32, 8


def _state_dict(z, tag):
    """a state_dict with the reference's keys, shapes and dtypes, seeded values"""
    sd = OrderedDict()
    for k, shape, dtype in zip(z[tag + '.keys'], z[tag + '.shapes'], z[tag + '.dtypes']):
        dims = tuple(int(n) for n in str(shape).split(',')) if str(shape) else ()
        sd[str(k)] = torch.randn(dims).to(getattr(torch, str(dtype)))
    return sd


def _reference_checkpoint(tmp_path, golden):
    z = golden('reference_checkpoint32_schema')
    torch.manual_seed(123)
    generator, g_ema, discriminator = _state_dict(z, 'g'), _state_dict(z, 'g'), _state_dict(z, 'd')
    # the parameters in the reference's parameters() order, sharing storage with the state_dict entries (as module parameters do)
    g_params = [torch.nn.Parameter(generator[str(n)]) for n in z['g.param_names']]
    d_params = [torch.nn.Parameter(discriminator[str(n)]) for n in z['d.param_names']]
    g_ratio, d_ratio = 4 / 5, 16 / 17
    g_optim = torch.optim.Adam(g_params, lr=0.002 * g_ratio, betas=(0 ** g_ratio, 0.99 ** g_ratio))
    d_optim = torch.optim.Adam(d_params, lr=0.002 * d_ratio, betas=(0 ** d_ratio, 0.99 ** d_ratio))
    for params, opt in ((g_params, g_optim), (d_params, d_optim)):
        for i, q in enumerate(params):
            if not (params is g_params and i % 17 == 3):         # some parameters without gradient (the unused noise weights)
                q.grad = torch.randn_like(q) * 1e-3
        opt.step()
    path = os.path.join(tmp_path, '790000.pt')
    torch.save({'g': generator, 'd': discriminator, 'g_ema': g_ema, 'g_optim': g_optim.state_dict(), 'd_optim': d_optim.state_dict()},
               path)
    return path, generator, discriminator, g_ema, g_optim, d_optim


def test_reference_written_checkpoint_restores_into_our_modules(tmp_path, golden):
    from transeditor_amd.model_spatial_query import Discriminator, Generator
    from transeditor_amd.optim import FusedAdam
    from transeditor_amd.train_step import load_checkpoint_into
    path, rg, rd, rema, rgo, rdo = _reference_checkpoint(str(tmp_path), golden)
    mk = lambda: Generator(SIZE, 512, 512, TOKEN, n_trans=8, pixel_norm_op_dim=1)
    g, ema, d = mk(), mk(), Discriminator(SIZE)
    go = FusedAdam(g.parameters(), lr=0.1, betas=(0.5, 0.5))          # (deliberately wrong: the checkpoint must overwrite them)
    do = FusedAdam(d.parameters(), lr=0.1, betas=(0.5, 0.5))
    start = load_checkpoint_into(path, ema, g, d, go, do, device='cpu')
    assert start == 790000
    for ours, ref in ((g, rg), (d, rd), (ema, rema)):
        a, b = ours.state_dict(), ref
        assert list(a.keys()) == list(b.keys())
        for k in a:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    for ours, ref in ((go, rgo), (do, rdo)):
        a, b = ours.state_dict(), ref.state_dict()
        ga, gb = a['param_groups'][0], b['param_groups'][0]
        for key in ('lr', 'betas', 'eps', 'weight_decay', 'params'):
            assert ga[key] == gb[key], key
        assert set(a['state'].keys()) == set(b['state'].keys())
        for idx, st in b['state'].items():
            for key in ('step', 'exp_avg', 'exp_avg_sq'):
                assert torch.equal(torch.as_tensor(a['state'][idx][key]).float().cpu(), torch.as_tensor(st[key]).float().cpu()), (idx, key)
    # the published inference checkpoints hold 'g_ema' only (test_spatial_query.py:285)
    only = os.path.join(str(tmp_path), 'published.pt')
    torch.save({'g_ema': rema}, only)
    ema2 = mk()
    assert load_checkpoint_into(only, ema2, device='cpu') is None
    assert all(torch.equal(v, rema[k]) for k, v in ema2.state_dict().items())

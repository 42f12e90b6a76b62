"""Writes tests/golden/lpips_alex_loss_ref.npz and tests/golden/LPIPS_ALEX_LOSS_REPORT.txt: the value and the gradient with respect to x that
the reference's own AlexNet LPIPS of encoder training (pSp/criteria/lpips/lpips.py LPIPS('alex')) gives under torch autograd, in fp32
and in fp64 on the CPU, for the synthetic network weights and images of tests/lpips_alex_restated.py and the heads of the reference's
utils/lpips/weights/v0.1/alex.pth, next to the restatement of tests/lpips_alex_loss_restated.py.  CPU only, a few seconds.

    python tools/lpips_alex_loss_golden.py --reference /path/to/TransEditor [--out tests/golden/lpips_alex_loss_ref.npz]

The reference class would fetch two files from the hub and move itself to a GPU.  So pSp.criteria.lpips is imported with a placeholder
`torchvision.models` whose alexnet is the module-form AlexNet of tests/lpips_alex_restated.py (torchvision's child order and names;
torchvision itself is not needed); get_state_dict is replaced, in pSp.criteria.lpips.utils and in pSp.criteria.lpips.lpips, by a read
of the local alex.pth with the same renaming of its keys; and Module.to is a no-op while the class is constructed.  The seeded
convolution weights are then loaded into the class's own `net.layers`.  z_score, normalize_activation, LinLayers and LPIPS.forward are
the reference's own code.

Stored: the seeds and sizes (lpips_alex_loss_restated.GOLDEN; the convolution weights are regenerated from them), the two image
batches themselves (tanh in fp32 does not give the same last bit on every CPU, and the fp64 results are compared to 1e-13), the
reference's value and gradient in fp32 and in fp64, and the five head weight vectors copied from alex.pth as plain arrays.
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HEADS_FILE = os.path.join('utils', 'lpips', 'weights', 'v0.1', 'alex.pth')


def load_reference(root, alexnet):
    """(pSp.criteria.lpips.lpips, pSp.criteria.lpips.utils) of the reference at `root`, their torchvision.models.alexnet being `alexnet`"""
    names = ('torchvision', 'torchvision.models')
    saved = {k: sys.modules.get(k) for k in names}
    sys.path.insert(0, root)
    try:
        for k in names:
            sys.modules[k] = types.ModuleType(k)
        sys.modules['torchvision.models'].alexnet = alexnet
        sys.modules['torchvision'].models = sys.modules['torchvision.models']
        ref = importlib.import_module('pSp.criteria.lpips.lpips')
        utils = importlib.import_module('pSp.criteria.lpips.utils')
    finally:
        sys.path.remove(root)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return ref, utils


def local_heads(root):
    """alex.pth of the reference tree under the keys LinLayers.load_state_dict expects ({l}.1.weight)"""
    sd = torch.load(os.path.join(root, HEADS_FILE), map_location='cpu')
    return {k.replace('lin', '').replace('model.', ''): v for k, v in sd.items()}, sd


def construct(ref, utils, root):
    """LPIPS('alex') with the local heads and a no-op Module.to"""
    renamed, raw = local_heads(root)
    to, saved = torch.nn.Module.to, (ref.get_state_dict, utils.get_state_dict)
    try:
        torch.nn.Module.to = lambda self, *a, **k: self
        ref.get_state_dict = utils.get_state_dict = lambda *a, **k: renamed
        return ref.LPIPS(net_type='alex'), raw
    finally:
        torch.nn.Module.to = to
        ref.get_state_dict, utils.get_state_dict = saved


def run(model, x, y, dtype):
    model = model.to(dtype)
    xin = x.detach().clone().to(dtype).requires_grad_(True)
    v = model(xin, y.to(dtype))
    g, = torch.autograd.grad(v, xin)
    return v.detach(), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference repository (its pSp/criteria/lpips is imported)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'lpips_alex_loss_ref.npz'))
    a = ap.parse_args()
    import lpips_alex_loss_restated as LR
    import lpips_alex_restated as R
    G = LR.GOLDEN
    root = os.path.abspath(a.reference)
    ref, utils = load_reference(root, R.alexnet)
    model, lin = construct(ref, utils, root)
    model.eval()
    sd = R.state_dict(G['seed'])
    model.net.layers.load_state_dict({k[len('features.'):]: v for k, v in sd.items()})              # strict: torchvision's layout
    x, y = R.images(G['x_seed'], G['B'], G['S']), R.images(G['y_seed'], G['B'], G['S'])
    v32, g32 = run(model, x, y, torch.float32)
    v64, g64 = run(model, x, y, torch.float64)
    r32, rg32 = LR.value_and_grad(x, y, sd, lin, torch.float32)
    r64, rg64 = LR.value_and_grad(x, y, sd, lin, torch.float64)
    heads = LR.heads_of(lin)
    zeros = {S: LR.zero_pixels(R.images(G['x_seed'], 2, *S), sd) for S in ((31, 31), (45, 39), (64, 64), (188, 188), (256, 256))}
    out = {k: np.int64(v) for k, v in G.items()}
    out.update(x=x.numpy(), y=y.numpy(), v_ref=v32.numpy(), g_ref=g32.numpy(), v64=v64.numpy(), g64=g64.numpy(),
               **{f'lin{l}': h.numpy() for l, h in enumerate(heads)})
    lines = ["AlexNet LPIPS loss golden vectors (tools/lpips_alex_loss_golden.py): the reference's LPIPS('alex') (pSp/criteria/lpips/lpips.py)",
             'under torch autograd on the CPU, in fp32 and in fp64, against the restatement of tests/lpips_alex_loss_restated.py.  Its',
             "torchvision.models.alexnet is the module-form AlexNet of lpips_alex_restated.py; z_score, normalize_activation, LinLayers and",
             "LPIPS.forward are the reference's own, and the heads are its own utils/lpips/weights/v0.1/alex.pth.",
             f'convolution weights: lpips_alex_restated.state_dict({G["seed"]}); x: images({G["x_seed"]}, {G["B"]}, {G["S"]}); '
             f'y: images({G["y_seed"]}, {G["B"]}, {G["S"]}).',
             '',
             f'heads: widths {[len(h) for h in heads]} ({sum(len(h) for h in heads)} floats), minimum {min(float(h.min()) for h in heads):.3e}, '
             f'sums {[round(float(h.sum()), 4) for h in heads]}',
             f'value: reference fp32 {float(v32):.9f}, fp64 {float(v64):.12f}; restatement fp32 {float(r32):.9f}, fp64 {float(r64):.12f}',
             f'value, relative to fp64: reference fp32 {abs(float(v32) - float(v64)) / float(v64):.3e}, restatement fp64 '
             f'{abs(float(r64) - float(v64)) / float(v64):.3e}',
             f'gradient, rel_l2 against the reference in fp64: reference fp32 {R.rel_l2(g32, g64):.3e} (the yardstick of the golden test), '
             f'restatement fp64 {R.rel_l2(rg64, g64):.3e}, restatement fp32 {R.rel_l2(rg32, g64):.3e}',
             f'gradient: |g64|_2 {float(g64.norm()):.6e}, max |g64| {float(g64.abs().max()):.6e}',
             'tap pixels that are zero on every channel (2 images of seed 101), by image size: '
             + ', '.join(f'{h}x{w}: {z}' for (h, w), z in zeros.items()), '']
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    report = os.path.join(os.path.dirname(os.path.abspath(a.out)), 'LPIPS_ALEX_LOSS_REPORT.txt')
    with open(report, 'w') as f:
        f.write('\n'.join(lines))
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes) and {report}')


if __name__ == '__main__':
    main()

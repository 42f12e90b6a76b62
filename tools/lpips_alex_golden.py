"""Writes tests/golden/lpips_alex_ref.npz and tests/golden/LPIPS_ALEX_REPORT.txt: what the reference's own AlexNet LPIPS (metrics/lpips.py:49-82
LPIPS) returns, pair by pair in fp32 on the CPU, for the synthetic network weights and images of tests/lpips_alex_restated.py and its own
head weights (metrics/lpips_weights.ckpt), next to the fp64 restatement.  CPU only, a few seconds.

    python tools/lpips_alex_golden.py --reference /path/to/TransEditor [--out tests/golden/lpips_alex_ref.npz]

lpips.py is loaded from its file with a placeholder `torchvision.models` whose alexnet is the module-form AlexNet of
tests/lpips_alex_restated.py (torchvision's child order and names, so that `.features` and the Conv2d / ReLU walk of the reference's
AlexNet class come out as with torchvision; torchvision itself is not needed).  The class calls .cuda() on its constants and opens
metrics/lpips_weights.ckpt by a relative path, so during construction Tensor.cuda is a no-op and the working directory is the reference
root.  The seeded convolution weights are then loaded into the class's own `alexnet.layers`.  normalize, Conv1x1 (dropout in eval mode)
and LPIPS.forward are the reference's own code.

Stored: the seeds and sizes (lpips_alex_restated.GOLDEN; images and convolution weights are regenerated from them), the reference's
N (N - 1) / 2 values in the order i < j row-major, the fp64 restatement's, and the five head weight vectors copied from
lpips_weights.ckpt as plain arrays.  A few KB.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def load_reference(root, alexnet):
    """metrics/lpips.py as a module, its torchvision.models.alexnet being `alexnet`"""
    names = ('torchvision', 'torchvision.models')
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k in names:
            sys.modules[k] = types.ModuleType(k)
        sys.modules['torchvision.models'].alexnet = alexnet
        sys.modules['torchvision'].models = sys.modules['torchvision.models']
        spec = importlib.util.spec_from_file_location('reference_metrics_lpips', os.path.join(root, 'metrics', 'lpips.py'))
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return ref


def construct(ref, root):
    """LPIPS() with a no-op Tensor.cuda, from the reference root"""
    cwd, cuda = os.getcwd(), torch.Tensor.cuda
    try:
        os.chdir(root)
        torch.Tensor.cuda = lambda self, *a, **k: self
        return ref.LPIPS()
    finally:
        torch.Tensor.cuda = cuda
        os.chdir(cwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference repository (its metrics/lpips.py is loaded)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'lpips_alex_ref.npz'))
    a = ap.parse_args()
    import lpips_alex_restated as R
    G = R.GOLDEN
    ref = load_reference(a.reference, R.alexnet)
    model = construct(ref, os.path.abspath(a.reference)).eval()
    sd = R.state_dict(G['seed'])
    model.alexnet.layers.load_state_dict({k[len('features.'):]: v for k, v in sd.items()})          # strict: torchvision's layout
    lin = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith('lpips_weights.')}
    x = R.images(G['image_seed'], G['N'], G['S'])
    pairs = [(i, j) for i in range(G['N'] - 1) for j in range(i + 1, G['N'])]
    with torch.no_grad():
        d_ref = torch.stack([model(x[i:i + 1], x[j:j + 1]) for i, j in pairs])
    d64 = R.triu(R.pairwise(x, sd, lin, torch.float64))
    d32 = R.triu(R.pairwise(x, sd, lin, torch.float32))
    taps64 = R.taps(x, sd, torch.float64)
    zero_pixels = [int(((t ** 2).sum(1) == 0).sum()) for t in taps64]
    heads = R.heads_of(lin)
    rel = lambda p, q: float(((p.double() - q.double()).abs() / q.double().abs()).max())
    out = {k: np.int64(G[k]) for k in ('seed', 'image_seed', 'N', 'S')}
    out.update(d_ref=d_ref.numpy(), d64=d64.numpy(), **{f'lin{l}': h.numpy() for l, h in enumerate(heads)})
    gaps = (d64.view(-1, 1) - d64.view(1, -1)).abs() + torch.eye(len(d64), dtype=torch.float64) * 1e30
    lines = ["AlexNet LPIPS golden vectors (tools/lpips_alex_golden.py): the reference's LPIPS (metrics/lpips.py:49-82) in fp32 on the CPU, pair",
             'by pair, against the fp64 restatement of tests/lpips_alex_restated.py.  Its torchvision.models.alexnet is the module-form AlexNet',
             "of lpips_alex_restated.py (torchvision's child order and names); normalize, Conv1x1 and LPIPS.forward are the reference's own, and",
             'the heads are its own metrics/lpips_weights.ckpt.',
             f'convolution weights: lpips_alex_restated.state_dict({G["seed"]}); images: lpips_alex_restated.images({G["image_seed"]}, {G["N"]}, {G["S"]}).',
             '',
             f'heads: widths {[len(h) for h in heads]}, minimum over all values {min(float(h.min()) for h in heads):.3e} (every value >= 0: '
             f'{all(bool((h >= 0).all()) for h in heads)}), sums {[round(float(h.sum()), 4) for h in heads]}',
             f'tap planes at {G["S"]} px: {[tuple(t.shape[1:]) for t in taps64]}; pixels that are zero on every channel: {zero_pixels}',
             f'{len(pairs)} pairs; reference against fp64: rel_l2 {R.rel_l2(d_ref, d64):.3e}, max relative {rel(d_ref, d64):.3e}',
             f'the restatement in fp32 against fp64: rel_l2 {R.rel_l2(d32, d64):.3e}, max relative {rel(d32, d64):.3e}; reference against that '
             f'restatement: rel_l2 {R.rel_l2(d_ref, d32):.3e}',
             f'values (fp64): min {float(d64.min()):.6f}, max {float(d64.max()):.6f}, smallest gap between two pairs {float(gaps.min()):.3e}',
             f'reference: {[round(float(v), 7) for v in d_ref]}', '']
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    report = os.path.join(os.path.dirname(os.path.abspath(a.out)), 'LPIPS_ALEX_REPORT.txt')
    with open(report, 'w') as f:
        f.write('\n'.join(lines))
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes) and {report}')


if __name__ == '__main__':
    main()

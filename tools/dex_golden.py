"""Writes tests/golden/dex_ref.npz and tests/golden/DEX_REPORT.txt: what the reference's own DEX classes (our_interfaceGAN/ffhq_utils/dex/
models.py: Age, Gender) return for the synthetic weights and images of tests/dex_restated.py, in fp32 on the CPU, next to the fp64
restatement.  CPU only, about a minute (two 4096-wide VGG16s are built and the network runs twice in fp64).

    python tools/dex_golden.py --reference /path/to/TransEditor [--out tests/golden/dex_ref.npz]

models.py is loaded from its file with a placeholder `torchvision.models` (it only needs the name resnet18 to exist for the pose model,
which is not built here).  api.py cannot be loaded: it moves its models to 'cuda' and reads weight files at fixed paths.  So three
steps are RESTATED here (tests/dex_restated.py), not run from the reference: the preprocessing of edit_all_noinversion_ffhq.py:113-116
(channel flip, clamp, +1, /2, *255, round), the centre crop of api.py:62 (CenterCrop(224); estimate_age's own slice at api.py:50-52 is
the same window for a 256 px image) and the score of api.py:42-44, :56-58 (age) and :64 (gender).  Everything between them -- the 13
convolutions, the pools, the flatten, fc1, fc2, cls and the softmax -- is the reference's own forward.

Stored: the seeds and sizes (dex_restated.GOLDEN; the images and weights are regenerated from them), per attribute the reference's
probabilities [B,C] and scores [B] (fp32) and the fp64 restatement's probabilities.  A few KB.
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


def load_reference(root):
    """our_interfaceGAN/ffhq_utils/dex/models.py as a module"""
    names = {'torchvision': [], 'torchvision.models': ['resnet18']}
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k, attrs in names.items():
            m = types.ModuleType(k)
            for a in attrs:
                setattr(m, a, None)
            sys.modules[k] = m
        sys.modules['torchvision'].models = sys.modules['torchvision.models']
        spec = importlib.util.spec_from_file_location('reference_dex_models',
                                                      os.path.join(root, 'our_interfaceGAN', 'ffhq_utils', 'dex', 'models.py'))
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return ref


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference repository (its ffhq_utils/dex/models.py is loaded)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'dex_ref.npz'))
    a = ap.parse_args()
    ref = load_reference(a.reference)
    import dex_restated as R
    G = R.GOLDEN
    x = R.images(G['image_seed'], G['B'], G['S'])
    sds = dict(zip(('age', 'gender'), R.state_dict(G['seed'], classes=(101, 2))))
    crop = R.crop_of(sds['age'])
    v = R.preprocess(x, crop)                                                   # restated: see the module docstring
    out = {k: np.int64(G[k]) for k in ('seed', 'image_seed', 'B', 'S')}
    lines = ['DEX golden vectors (tools/dex_golden.py): the reference\'s Age / Gender (ffhq_utils/dex/models.py) in fp32 on the CPU against',
             'the fp64 restatement of tests/dex_restated.py.',
             f'weights: dex_restated.state_dict({G["seed"]}, classes=(101, 2)); images: dex_restated.images({G["image_seed"]}, {G["B"]}, '
             f'{G["S"]}); crop {crop}.',
             'Restated, not run from the reference: edit_all_noinversion_ffhq.py:113-116 (flip, clamp, +1, /2, *255, round), the centre',
             'crop of api.py:62 (= api.py:50-52 at 256 px) and the scores of api.py:42-44, :56-58, :64.  api.py itself is tied to \'cuda\'',
             'and to fixed weight paths.  The network between them (models.py:49-57) is the reference\'s own forward.', '']
    for attribute, cls in (('age', ref.Age), ('gender', ref.Gender)):
        sd = sds[attribute]
        model = cls()
        model.load_state_dict(sd)                                               # strict: the key layout is the reference's
        model.eval()
        with torch.no_grad():
            p_ref = model(v)
        s_ref = R.score_of(p_ref, attribute)
        p64 = R.probabilities(x, sd, torch.float64)
        p32 = R.probabilities(x, sd, torch.float32)
        s64 = R.score_of(p64, attribute)
        l64 = R.logits(x, sd, torch.float64)
        yard = rel_l2(p_ref, p64)
        bar = R.score_bar(4 * yard, p64, attribute)
        gaps = (s64.view(-1, 1) - s64.view(1, -1)).abs() + torch.eye(len(s64), dtype=torch.float64) * 1e30
        out[f'{attribute}_prob'], out[f'{attribute}_score'] = p_ref.numpy(), s_ref.numpy()
        out[f'{attribute}_prob64'] = p64.numpy()
        lines += [f'{attribute}: classes {p_ref.shape[1]}',
                  f'  reference against fp64: probabilities rel_l2 {yard:.3e} (the restatement in fp32: {rel_l2(p32, p64):.3e}; reference '
                  f'against that restatement: {rel_l2(p_ref, p32):.3e})',
                  f'  scores: reference {[float(s) for s in s_ref]}, fp64 {[float(s) for s in s64]}',
                  f'  |reference score - fp64| / (4 x yardstick Cauchy-Schwarz bar), per row: {[float(q) for q in (s_ref.double() - s64).abs() / bar]}',
                  f'  relative deviation of the score: {[float(q) for q in (s_ref.double() - s64).abs() / s64.abs()]}',
                  f'  non-degeneracy (fp64): logit std per row {[round(float(q), 3) for q in l64.std(1)]}, largest probability '
                  f'{float(p64.max()):.4f}, p_0 per row {[round(float(q), 4) for q in p64[:, 0]]}, smallest score gap between rows / bar '
                  f'{float(gaps.min()) / float(bar.max()):.0f}', '']
        print('\n'.join(lines[-7:]))
        del model
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    report = os.path.join(os.path.dirname(os.path.abspath(a.out)), 'DEX_REPORT.txt')
    with open(report, 'w') as f:
        f.write('\n'.join(lines))
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes) and {report}')


if __name__ == '__main__':
    main()

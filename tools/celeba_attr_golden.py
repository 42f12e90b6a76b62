"""Writes tests/golden/celeba_attr_ref.npz and tests/golden/CELEBA_ATTR_REPORT.txt: what the reference's own attribute classifier
(our_interfaceGAN/celebahq_utils/dex/networks/classifiers/attribute_classifier.py: D) returns for the seeded weights and images of
tests/celeba_attr_restated.py, in fp32 on the CPU, next to the fp64 restatement.  CPU only, well under a minute.

    python tools/celeba_attr_golden.py --reference /path/to/TransEditor [--out tests/golden/celeba_attr_ref.npz]

attribute_classifier.py is loaded from its file (it needs torch and numpy only) and D is built as attribute_utils.py:45-46 builds it:
fixed_size=True, use_mbstd=False.  attribute_utils.py itself cannot be used: load_attribute_classifier moves the network to 'cuda'.
So two steps are RESTATED here (tests/celeba_attr_restated.py), not run from the reference: the preprocessing of
edit_all_noinversion_celebahq.py:175-177 (channel flip, clamp, +1, /2, *255, round) and the score of attribute_utils.py:28-32
(softmax(cat([logit, -logit], 1))[:, 1]).  Everything between them -- fromrgb_lod0, the blocks, the 4x4 block with both dense layers -- is
the reference's own forward.  Both geometries feed images of the network's own resolution, so attribute_utils.downsample is the identity.

Stored per geometry of celeba_attr_restated.GOLDEN ('small': R = 32, fmap_base 256, fmap_max 64; 'true': R = 256, the defaults): the
seeds and sizes (the images and weights are regenerated from them), the reference's logits and scores [B] (fp32) and the fp64
restatement's logits.  A few KB.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

STORED = ('R', 'fmap_base', 'fmap_max', 'B', 'S', 'seed', 'image_seed')


def load_reference(root):
    """our_interfaceGAN/celebahq_utils/dex/networks/classifiers/attribute_classifier.py as a module"""
    path = os.path.join(root, 'our_interfaceGAN', 'celebahq_utils', 'dex', 'networks', 'classifiers', 'attribute_classifier.py')
    spec = importlib.util.spec_from_file_location('reference_attribute_classifier', path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference repository (its attribute_classifier.py is loaded)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'celeba_attr_ref.npz'))
    a = ap.parse_args()
    ref = load_reference(a.reference)
    import celeba_attr_restated as R
    out = {}
    lines = ["CelebA-HQ attribute classifier golden vectors (tools/celeba_attr_golden.py): the reference's D (celebahq_utils/dex/networks/",
             'classifiers/attribute_classifier.py, fixed_size=True, use_mbstd=False) in fp32 on the CPU against the fp64 restatement of',
             'tests/celeba_attr_restated.py.',
             'Restated, not run from the reference: edit_all_noinversion_celebahq.py:175-177 (flip, clamp, +1, /2, *255, round) and the',
             "score of attribute_utils.py:28-32.  attribute_utils.py itself is tied to 'cuda'.  The network between them",
             "(attribute_classifier.py:200-215) is the reference's own forward.", '']
    for name, c in R.GOLDEN.items():
        sd, x = R.case_state_dict(c), R.case_images(c)
        model = ref.D(num_channels=3, resolution=c['R'], fmap_base=c['fmap_base'], fmap_max=c['fmap_max'], fixed_size=True, use_mbstd=False)
        model.load_state_dict(sd)                                               # strict: the key layout is the reference's
        model.eval()
        v = R.preprocess(x)                                                     # restated: see the module docstring
        assert v.shape[2] == c['R']
        with torch.no_grad():
            l_ref = model(v)
            s_ref = torch.softmax(torch.cat([l_ref, -l_ref], dim=1), dim=1)[:, 1]
        l_ref = l_ref[:, 0]
        l64, l32 = R.logits(x, sd, torch.float64), R.logits(x, sd, torch.float32)
        cond = R.conditions(l64, x)
        yard = rel_l2(l_ref, l64)
        for k in STORED:
            out[f'{name}_{k}'] = np.int64(c[k])
        out[f'{name}_logit'], out[f'{name}_score'], out[f'{name}_logit64'] = l_ref.numpy(), s_ref.numpy(), l64.numpy()
        chans = [sd[R.weight_key(p)].shape[0] for p, _, _, _ in R.layers(c['R'], c['fmap_base'], c['fmap_max'])]
        lines += [f'{name}: R {c["R"]}, fmap_base {c["fmap_base"]}, fmap_max {c["fmap_max"]}, B {c["B"]}, weights seed {c["seed"]}, images seed '
                  f'{c["image_seed"]}; output channels per layer {chans}',
                  f'  reference against fp64: logits rel_l2 {yard:.3e} (the restatement in fp32: {rel_l2(l32, l64):.3e}; reference against '
                  f'that restatement: {rel_l2(l_ref, l32):.3e}, bit-equal: {bool(torch.equal(l_ref, l32))})',
                  f'  logits: reference {[float(q) for q in l_ref]}, fp64 {[float(q) for q in l64]}',
                  f'  scores: reference {[float(q) for q in s_ref]}, fp64 {[float(q) for q in R.score_of(l64)]}',
                  f'  reference logit error / logit spread: {float((l_ref.double() - l64).abs().max()) / cond["spread"]:.3e}',
                  f'  conditions (fp64): scores in [{cond["score_min"]:.4f}, {cond["score_max"]:.4f}], logit spread {cond["spread"]:.4f}, '
                  f'pixels clamped to 0 / 255: {cond["clamped_low"]:.3f} / {cond["clamped_high"]:.3f}', '']
        print('\n'.join(lines[-7:]))
        del model
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    report = os.path.join(os.path.dirname(os.path.abspath(a.out)), 'CELEBA_ATTR_REPORT.txt')
    with open(report, 'w') as f:
        f.write('\n'.join(lines))
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes) and {report}')


if __name__ == '__main__':
    main()

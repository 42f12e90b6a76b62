"""Writes tests/golden/pose_ref.npz and tests/golden/POSE_REPORT.txt: what the reference's own pose classifier (our_interfaceGAN/ffhq_utils/
dex/models.py:73-89 ClassifyModel) returns for the synthetic weights and images of tests/pose_restated.py, in fp32 on the CPU, next to the
fp64 restatement.  CPU only, well under a minute.

    python tools/pose_golden.py --reference /path/to/TransEditor [--out tests/golden/pose_ref.npz]

models.py is loaded from its file, as tools/dex_golden.py loads it, with a placeholder `torchvision.models` whose resnet18 is the
module-form ResNet-18 of tests/pose_restated.py (torchvision's child order and names, so that get_resnet's children()[:-1] and the
state dict keys backbone.N.* come out as with torchvision; torchvision itself is not needed).  ClassifyModel - get_resnet, extra_layer,
flatten, softmax - is the reference's own code, run on that backbone.  api.py cannot be loaded (it moves its models to 'cuda' and reads
weight files at fixed paths), so three steps are RESTATED (tests/dex_restated.py): the preprocessing of
edit_all_noinversion_ffhq.py:113-116, the centre crop of api.py:62 and the [:, 0] of api.py:64.

Stored: the seeds and sizes (pose_restated.GOLDEN; the images and every weight but extra_layer are regenerated from them), the
calibrated extra_layer (pose_restated.state_dict calibrates it on the images in fp64; stored so that the GPU test need not run the
network in fp64), the reference's probabilities [B,2] (fp32), the fp64 restatement's, and the reference class's state dict keys with
their shapes.  A few KB.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference repository (its ffhq_utils/dex/models.py is loaded)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'pose_ref.npz'))
    a = ap.parse_args()
    import dex_golden
    import pose_restated as R
    ref = dex_golden.load_reference(a.reference)
    ref.resnet18 = R.resnet18                                                   # models.py did `from torchvision.models import resnet18`
    rel_l2 = dex_golden.rel_l2
    G = R.GOLDEN
    x = R.images(G['image_seed'], G['B'], G['S'])
    sd = R.state_dict(G['seed'], images=x, crop=G['crop'])
    v = R.preprocess(x, G['crop'])                                              # restated: see the module docstring
    model = ref.ClassifyModel()
    keys = {k: tuple(t.shape) for k, t in model.state_dict().items()}
    model.load_state_dict(sd)                                                   # strict: the key layout is the reference's
    model.eval()
    with torch.no_grad():
        p_ref = model(v)
    p64 = R.probabilities(x, sd, torch.float64, G['crop'])
    p32 = R.probabilities(x, sd, torch.float32, G['crop'])
    l64 = R.logits(x, sd, torch.float64, G['crop'])
    yard = rel_l2(p_ref, p64)
    s64 = p64[:, 0]
    bar = R.score_bar(4 * yard, p64, 'gender')
    gaps = (s64.view(-1, 1) - s64.view(1, -1)).abs() + torch.eye(len(s64), dtype=torch.float64) * 1e30
    out = {k: np.int64(G[k]) for k in ('seed', 'image_seed', 'B', 'S', 'crop')}
    out.update(prob=p_ref.numpy(), prob64=p64.numpy(), extra_w=sd['extra_layer.weight'].numpy(), extra_b=sd['extra_layer.bias'].numpy(),
               keys=np.array(list(keys)), shapes=np.array([','.join(map(str, s)) for s in keys.values()]))
    lines = ['Pose golden vectors (tools/pose_golden.py): the reference\'s ClassifyModel (ffhq_utils/dex/models.py:73-89) in fp32 on the CPU',
             'against the fp64 restatement of tests/pose_restated.py.  Its torchvision.models.resnet18 is the module-form ResNet-18 of',
             'pose_restated.py (torchvision\'s child order and names); get_resnet, extra_layer, flatten and softmax are the reference\'s own.',
             f'weights: pose_restated.state_dict({G["seed"]}, images=images, crop={G["crop"]}) (extra_layer calibrated on the images in fp64); '
             f'images: pose_restated.images({G["image_seed"]}, {G["B"]}, {G["S"]}).',
             'Restated, not run from the reference: edit_all_noinversion_ffhq.py:113-116 (flip, clamp, +1, /2, *255, round), the centre',
             'crop of api.py:62 and the [:, 0] of api.py:64.  api.py itself is tied to \'cuda\' and to fixed weight paths.', '',
             f'state dict: {len(keys)} keys, {sum(k.endswith("num_batches_tracked") for k in keys)} of them num_batches_tracked',
             f'reference against fp64: probabilities rel_l2 {yard:.3e} (the restatement in fp32: {rel_l2(p32, p64):.3e}; reference against that '
             f'restatement: {rel_l2(p_ref, p32):.3e})',
             f'p_0: reference {[float(s) for s in p_ref[:, 0]]}, fp64 {[float(s) for s in s64]}',
             f'|reference p_0 - fp64| / (4 x yardstick Cauchy-Schwarz bar), per row: {[float(q) for q in (p_ref[:, 0].double() - s64).abs() / bar]}',
             f'non-degeneracy (fp64): logits {[[round(float(q), 4) for q in r] for r in l64]}, smallest p_0 gap between rows / bar '
             f'{float(gaps.min()) / float(bar.max()):.0f}', '']
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    report = os.path.join(os.path.dirname(os.path.abspath(a.out)), 'POSE_REPORT.txt')
    with open(report, 'w') as f:
        f.write('\n'.join(lines))
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes) and {report}')


if __name__ == '__main__':
    main()

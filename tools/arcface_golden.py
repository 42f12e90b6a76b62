"""Writes tests/golden/arcface_ref.npz and tests/golden/ARCFACE_REPORT.txt: what the reference's own ArcFace network (pSp/models/encoders/
model_irse.py:10-49 Backbone with helpers.py, built as pSp/criteria/id_loss.py:12 builds it: Backbone(input_size=112, num_layers=50,
drop_ratio=0.6, mode='ir_se')) returns for the synthetic weights and images of tests/arcface_restated.py, in fp32 on the CPU, next to
the fp64 restatement.  CPU only, a few seconds.

    python tools/arcface_golden.py --reference /path/to/TransEditor [--out tests/golden/arcface_ref.npz]

model_irse.py and helpers.py are loaded from their files (under the package names model_irse.py imports helpers by; the pSp package
itself is not imported).  id_loss.py cannot be loaded: it reads a weight file at a fixed path.  So its two lines in front of the network
are RESTATED (arcface_restated.extract): the crop x[:, :, 35:223, 32:220] and AdaptiveAvgPool2d((112, 112)).  Everything behind them is
the reference's own forward, l2_norm included.

Stored: the seeds and sizes (arcface_restated.GOLDEN; the images and weights are regenerated from them), the 24 factors by which
arcface_restated.state_dict scaled the units' SE fc2 when it calibrated them on the images in fp64 (so that a test need not walk the
network in fp64, and the weights do not depend on that walk's last bits), the reference's embeddings [B,512] (fp32), the fp64
restatement's, and the reference class's state dict keys with their shapes.  A few KB.
"""
import argparse
import importlib.util
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def load_reference(root):
    """pSp/models/encoders/model_irse.py as a module, with helpers.py under the name it imports it by"""
    pkgs = ['pSp', 'pSp.models', 'pSp.models.encoders']
    saved = {k: sys.modules.get(k) for k in pkgs + ['pSp.models.encoders.helpers']}
    enc = os.path.join(root, 'pSp', 'models', 'encoders')
    try:
        for k in pkgs:
            sys.modules[k] = types.ModuleType(k)
        out = []
        for name, file in (('pSp.models.encoders.helpers', 'helpers.py'), ('reference_model_irse', 'model_irse.py')):
            spec = importlib.util.spec_from_file_location(name, os.path.join(enc, file))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
            out.append(mod)
        sys.modules.pop('reference_model_irse', None)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return out[1]


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference repository (its pSp/models/encoders/model_irse.py is loaded)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'arcface_ref.npz'))
    a = ap.parse_args()
    ref = load_reference(a.reference)
    import arcface_restated as R
    G = R.GOLDEN
    x = R.images(G['image_seed'], G['B'], G['S'])
    sd, scales = R.state_dict(G['seed'], images=x, want_scales=True)
    again = R.state_dict(G['seed'], fc2_scale=scales)
    assert all(torch.equal(sd[k], again[k]) for k in sd)                        # the recorded factors reproduce the weights
    model = ref.Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode='ir_se')      # id_loss.py:12
    keys = {k: tuple(t.shape) for k, t in model.state_dict().items()}
    model.load_state_dict(sd)                                                   # strict: the key layout is the reference's
    model.eval()
    t0 = time.time()
    with torch.no_grad():
        e_ref = model(R.extract(x))                                             # restated: see the module docstring
    t_ref = time.time() - t0
    gates = []
    t0 = time.time()
    e64 = R.embed(x, sd, torch.float64, gates=gates)
    t64 = time.time() - t0
    e32 = R.embed(x, sd, torch.float32)
    yard = rel_l2(e_ref, e64)
    g = torch.cat(gates)
    cos = e64 @ e64.t()
    far = float((1 - cos + 9 * torch.eye(len(cos), dtype=torch.float64)).min())
    slopes = torch.cat([v.flatten() for k, v in sd.items() if k.endswith('res_layer.2.weight') or k == 'input_layer.2.weight'])
    out = {k: np.int64(G[k]) for k in ('seed', 'image_seed', 'B', 'S')}
    out.update(emb=e_ref.numpy(), emb64=e64.numpy(), fc2_scale=np.array(scales, dtype=np.float64), keys=np.array(list(keys)),
               shapes=np.array([','.join(map(str, s)) for s in keys.values()]))
    lines = ["ArcFace golden vectors (tools/arcface_golden.py): the reference's Backbone(112, 50, mode='ir_se') (pSp/models/encoders/",
             'model_irse.py:10-49, helpers.py:16-120, built as pSp/criteria/id_loss.py:12 builds it) in fp32 on the CPU against the fp64',
             'restatement of tests/arcface_restated.py.',
             f'weights: arcface_restated.state_dict({G["seed"]}, images=images) (each unit\'s SE fc2 calibrated on the images in fp64; the 24 factors',
             f'are stored as fc2_scale); images: arcface_restated.images({G["image_seed"]}, {G["B"]}, {G["S"]}).',
             'Restated, not run from the reference: id_loss.py:18-19 (the crop [35:223, 32:220] and AdaptiveAvgPool2d((112, 112))); id_loss.py',
             'itself reads a weight file at a fixed path.', '',
             f'state dict: {len(keys)} keys, {sum(k.endswith("num_batches_tracked") for k in keys)} of them num_batches_tracked; '
             f'{sum(t.numel() for k, t in sd.items() if t.is_floating_point() and "running" not in k) / 1e6:.1f} M parameters',
             f'reference against fp64: embeddings rel_l2 {yard:.3e} (the restatement in fp32: {rel_l2(e32, e64):.3e}; reference against that '
             f'restatement: {rel_l2(e_ref, e32):.3e})',
             f'time on this CPU: the reference in fp32 {t_ref:.1f} s, the restatement in fp64 {t64:.1f} s',
             f'non-degeneracy (fp64): smallest 1 - cos between different images {far:.4f} = {far / (4 * yard):.0f} x the bar (4 x the yardstick); '
             f'SE gates span [{float(g.min()):.4f}, {float(g.max()):.4f}]; {int((slopes < 0).sum())} of {slopes.numel()} PReLU slopes are negative',
             f'SE fc2 factors: {[round(s, 4) for s in scales]}', '']
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    report = os.path.join(os.path.dirname(os.path.abspath(a.out)), 'ARCFACE_REPORT.txt')
    with open(report, 'w') as f:
        f.write('\n'.join(lines))
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes) and {report}')


if __name__ == '__main__':
    main()

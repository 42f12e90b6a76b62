"""Writes tests/golden/id_loss_ref.npz and tests/golden/ID_LOSS_REPORT.txt: what the reference's own identity loss
(pSp/criteria/id_loss.py:8-45 IDLoss on pSp/models/encoders/model_irse.py Backbone(112, 50, mode='ir_se')) returns, and the gradient torch
autograd gives it, for the synthetic weights and images of tests/arcface_restated.py / tests/id_loss_restated.py, in fp32 on the CPU, next
to the fp64 restatement.  CPU only, a minute or two.

    python tools/id_loss_golden.py --reference /path/to/TransEditor [--out tests/golden/id_loss_ref.npz]

model_irse.py and helpers.py are loaded as tools/arcface_golden.py loads them.  id_loss.py is loaded from its file too, with two stand-ins
for what it imports at module level: pSp.configs.paths_config is a module whose model_paths['ir_se50'] names a temporary file that holds
the synthetic state dict (IDLoss.__init__ reads its weights from that fixed entry), and pSp.models.encoders.model_irse is the module
loaded above.  IDLoss.__init__, extract_feats (the crop, the pool) and forward are the reference's own.

Stored: the seeds and sizes (id_loss_restated.GOLDEN; images and weights are regenerated from them, the SE factors are
arcface_ref.npz's), the reference's loss, sim_improvement and logs (fp32), the fp64 restatement's, the fp64 restatement's gradient
d loss / d y_hat for image 0 INSIDE the box [3,188,188] rounded to fp32 (the gradient is 0 outside), that gradient's whole-batch norm
figures, and the yardstick: rel_l2 of the reference's own fp32 gradient (torch autograd) against the fp64 one, over the whole batch and
over the stored part.
"""
import argparse
import importlib.util
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def load_id_loss(root, weights):
    """pSp/criteria/id_loss.py as a module whose IDLoss() loads `weights` (a file holding a Backbone state dict)"""
    from arcface_golden import load_reference
    irse = load_reference(root)
    names = ['pSp', 'pSp.configs', 'pSp.configs.paths_config', 'pSp.models', 'pSp.models.encoders', 'pSp.models.encoders.model_irse']
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k in names:
            sys.modules[k] = types.ModuleType(k)
        sys.modules['pSp.configs.paths_config'].model_paths = {'ir_se50': weights}
        sys.modules['pSp.models.encoders.model_irse'] = irse
        spec = importlib.util.spec_from_file_location('reference_id_loss', os.path.join(root, 'pSp', 'criteria', 'id_loss.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference repository (its pSp/criteria/id_loss.py is loaded)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'id_loss_ref.npz'))
    a = ap.parse_args()
    import arcface_restated as R
    import id_loss_restated as IR
    G = IR.GOLDEN
    y_hat, y, x = (R.images(G[k], G['B'], G['S']) for k in ('image_seed', 'y_seed', 'x_seed'))
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'arcface_ref.npz'), allow_pickle=False)
    sd = R.state_dict(G['seed'], fc2_scale=z['fc2_scale'].tolist())
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'model_ir_se50.pth')
        torch.save(sd, path)
        ref = load_id_loss(a.reference, path).IDLoss()
    t0 = time.time()
    yh = y_hat.clone().requires_grad_(True)
    loss_ref, sim_ref, logs_ref = ref(yh, y, x)
    loss_ref.backward()
    t_ref = time.time() - t0
    g_ref = yh.grad
    t0 = time.time()
    gates, pres = [], []
    loss64, sim64, logs64, g64 = IR.id_loss(y_hat, y, x, sd, torch.float64, gates=gates, pres=pres)
    t64 = time.time() - t0
    y0, y1, x0, x1 = R.BOX
    outside = torch.ones(G['S'], G['S'], dtype=torch.bool)
    outside[y0:y1, x0:x1] = False
    assert bool((g64[:, :, outside] == 0).all()) and bool((g_ref[:, :, outside] == 0).all())
    part64, part_ref = g64[0, :, y0:y1, x0:x1], g_ref[0, :, y0:y1, x0:x1]
    yard, yard_part = rel_l2(g_ref, g64), rel_l2(part_ref, part64)
    keys = ('diff_target', 'diff_input', 'diff_views')
    gt = torch.cat(gates)
    near = min(float(p.abs().min() / p.abs().mean()) for p in pres)
    out = {k: np.int64(G[k]) for k in G}
    out.update(loss=np.float32(float(loss_ref)), sim_improvement=np.float64(sim_ref), logs=np.array([[d[k] for k in keys] for d in logs_ref]),
               loss64=np.float64(float(loss64)), sim_improvement64=np.float64(sim64), logs64=np.array([[d[k] for k in keys] for d in logs64]),
               grad64_image0_box=part64.float().numpy(), grad64_norm=np.float64(float(g64.norm())), grad64_norm_image0=np.float64(float(g64[0].norm())),
               yardstick=np.float64(yard), yardstick_image0=np.float64(yard_part))
    lines = ["Identity loss golden vectors (tools/id_loss_golden.py): the reference's IDLoss (pSp/criteria/id_loss.py:8-45, its own __init__,",
             "extract_feats and forward on its own Backbone(112, 50, mode='ir_se')) and torch autograd of it in fp32 on the CPU against the fp64",
             'restatement of tests/id_loss_restated.py.',
             f'weights: arcface_restated.state_dict({G["seed"]}, fc2_scale=arcface_ref.npz\'s); y_hat, y, x: arcface_restated.images(seed, {G["B"]}, {G["S"]}) with',
             f'seeds {G["image_seed"]}, {G["y_seed"]}, {G["x_seed"]}.', '',
             f'reference: loss {float(loss_ref):.7f}, sim_improvement {sim_ref:.7f}, logs {logs_ref}',
             f'fp64:      loss {float(loss64):.7f}, sim_improvement {sim64:.7f}, logs {logs64}',
             f'gradient d loss / d y_hat: |g64| = {float(g64.norm()):.4e} (image 0: {float(g64[0].norm()):.4e}); the reference\'s fp32 autograd against fp64: '
             f'rel_l2 {yard:.3e} over the batch, {yard_part:.3e} over image 0 inside the box (the stored part, {part64.numel() * 4} bytes)',
             f'every channel of every image has a non-zero gradient inside the box: {bool((g64[:, :, y0:y1, x0:x1].abs().amax((2, 3)) > 0).all())}',
             f'SE gates span [{float(gt.min()):.4f}, {float(gt.max()):.4f}]; the PReLU input nearest 0, relative to its layer\'s mean magnitude: {near:.2e}',
             f'time on this CPU: the reference forward + backward in fp32 {t_ref:.1f} s, the restatement in fp64 {t64:.1f} s', '']
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    report = os.path.join(os.path.dirname(os.path.abspath(a.out)), 'ID_LOSS_REPORT.txt')
    with open(report, 'w') as f:
        f.write('\n'.join(lines))
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes) and {report}')


if __name__ == '__main__':
    main()

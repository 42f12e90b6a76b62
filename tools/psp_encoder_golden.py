"""Writes tests/golden/psp_encoder_ref.npz and tests/golden/PSP_ENCODER_REPORT.txt: what the reference's own dual-space encoder
(pSp/models/encoders/psp_encoders_new.py:35-140 GradualStyleEncoder(50, 'ir_se'), built as pSp/models/psp_new.py:55 builds it) returns
for the synthetic weights and the image of tests/psp_encoder_restated.py, in fp32 on the CPU, next to the fp64 restatement.  CPU only,
about a minute (364.7 M weights are drawn, and the SE gates are calibrated by an fp64 walk).

    python tools/psp_encoder_golden.py --reference /path/to/TransEditor [--out tests/golden/psp_encoder_ref.npz]

psp_encoders_new.py and helpers.py are loaded from their files (helpers under the package name the encoder imports it by; the pSp
package itself is not imported); EqualLinear comes from the reference's model_spatial_query.py through oracle.ref_import.

Stored: the seeds and sizes (psp_encoder_restated.GOLDEN; the image and the weights are regenerated from them), the 24 factors by which
the units' SE fc2 were scaled when they were calibrated on the image in fp64, the reference's (z_out, p_out) [1,512,16] (fp32), the fp64
restatement's, and the reference class's state dict keys with their shapes.  No weights: a few hundred KB at the most.
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def load_reference(root):
    """pSp/models/encoders/psp_encoders_new.py as a module, with helpers.py under the name it imports it by"""
    from oracle import ref_import
    ref_import.REF_ROOT = root
    ref_import.import_reference()                                               # model_spatial_query (EqualLinear) into sys.modules
    pkgs = ['pSp', 'pSp.models', 'pSp.models.encoders']
    saved = {k: sys.modules.get(k) for k in pkgs + ['pSp.models.encoders.helpers']}
    enc = os.path.join(root, 'pSp', 'models', 'encoders')
    try:
        for k in pkgs:
            sys.modules[k] = types.ModuleType(k)
        out = []
        for name, file in (('pSp.models.encoders.helpers', 'helpers.py'), ('reference_psp_encoders_new', 'psp_encoders_new.py')):
            spec = importlib.util.spec_from_file_location(name, os.path.join(enc, file))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
            out.append(mod)
        sys.modules.pop('reference_psp_encoders_new', None)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return out[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference repository')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'psp_encoder_ref.npz'))
    a = ap.parse_args()
    ref = load_reference(a.reference)
    import arcface_restated as R
    import psp_encoder_restated as P
    G = P.GOLDEN
    x = R.images(G['image_seed'], G['B'], G['S'])
    t0 = time.time()
    sd, scales = P.state_dict(G['seed'], images=x, want_scales=True)
    t_draw = time.time() - t0
    again = P.state_dict(G['seed'], fc2_scale=scales)
    assert all(torch.equal(sd[k], again[k]) for k in sd)                        # the recorded factors reproduce the weights
    del again
    model = ref.GradualStyleEncoder(50, 'ir_se', types.SimpleNamespace(input_nc=3))           # psp_new.py:55
    keys = {k: tuple(t.shape) for k, t in model.state_dict().items()}
    n_param = sum(p.numel() for p in model.parameters())
    model.load_state_dict(sd)                                                   # strict: the key layout is the reference's
    model.eval()
    t0 = time.time()
    with torch.no_grad():
        z_ref, p_ref = model(x)
    t_ref = time.time() - t0
    del model
    t0 = time.time()
    z64, p64, lat64 = P.encode(x, sd, torch.float64, want_latents=True)
    t64 = time.time() - t0
    z32, p32 = P.encode(x, sd, torch.float32)
    yard = {'z': P.rel_l2(z_ref, z64), 'p': P.rel_l2(p_ref, p64)}
    heads = {k: v for k, v in sd.items() if k.startswith(('styles', 'spatials')) and '.convs.' in k and k.endswith('weight')}
    out = {k: np.int64(G[k]) for k in ('seed', 'image_seed', 'B', 'S')}
    out.update(z=z_ref.numpy(), p=p_ref.numpy(), z64=z64.numpy(), p64=p64.numpy(), fc2_scale=np.array(scales, dtype=np.float64),
               keys=np.array(list(keys)), shapes=np.array([','.join(map(str, s)) for s in keys.values()]),
               yard_z=np.float64(yard['z']), yard_p=np.float64(yard['p']))
    lines = ["pSp encoder golden vectors (tools/psp_encoder_golden.py): the reference's GradualStyleEncoder(50, 'ir_se')",
             '(pSp/models/encoders/psp_encoders_new.py:35-140, helpers.py:76-120, EqualLinear of model_spatial_query.py:194-221) in fp32 on the CPU',
             'against the fp64 restatement of tests/psp_encoder_restated.py.',
             f'weights: psp_encoder_restated.state_dict({G["seed"]}, images=image) (each unit\'s SE fc2 calibrated on the image in fp64; the 24 factors',
             f'are stored as fc2_scale); image: arcface_restated.images({G["image_seed"]}, {G["B"]}, {G["S"]}).', '',
             f'state dict: {len(keys)} keys, {sum(k.endswith("num_batches_tracked") for k in keys)} of them num_batches_tracked; {n_param / 1e6:.1f} M parameters; '
             f'{len(heads)} head convolutions hold {sum(v.numel() for v in heads.values()) * 4 / 1e9:.2f} GB',
             f'reference against fp64: z_out rel_l2 {yard["z"]:.3e}, p_out rel_l2 {yard["p"]:.3e} (the restatement in fp32: {P.rel_l2(z32, z64):.3e}, '
             f'{P.rel_l2(p32, p64):.3e}; reference against that restatement: {P.rel_l2(z_ref, z32):.3e}, {P.rel_l2(p_ref, p32):.3e})',
             f'time on this CPU: drawing and calibrating the weights {t_draw:.1f} s, the reference in fp32 {t_ref:.1f} s, the restatement in fp64 {t64:.1f} s',
             f'the codes: z_out std {float(z64.std()):.3f}, p_out std {float(p64.std()):.3f}, head latents std {float(lat64.std()):.3f} '
             f'(smallest per-head std {float(lat64.std(2).min()):.3f})',
             f'SE fc2 factors: {[round(s, 4) for s in scales]}', '']
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    report = os.path.join(os.path.dirname(os.path.abspath(a.out)), 'PSP_ENCODER_REPORT.txt')
    with open(report, 'w') as f:
        f.write('\n'.join(lines))
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes) and {report}')


if __name__ == '__main__':
    main()

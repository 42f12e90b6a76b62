"""Writes tests/golden/fid_ref.npz: what the reference's own calc_fid (metrics/fid_query.py: scipy.linalg.sqrtm) returns on np.mean /
np.cov of seeded non-negative features, with the inputs.  CPU only, seconds; needs scipy.

    python tools/fid_golden.py --reference /path/to/TransEditor [--out tests/golden/fid_ref.npz]

Cases (each from np.random.default_rng(2); real drawn first, then fake; cast to float32; tests/fid_restated.py draw()):
    real = max(N(0,1) A + 0.4, 0), A a D x D mixing matrix scaled by 1 / sqrt(D);  fake = max(0.9 N(0,1) + 0.3, 0)
    a: real (257, 96), fake (130, 96)
    b: real (40, 64),  fake (50, 64)      both covariances rank-deficient
    c: real (300, 33), fake (300, 33)
The reference's script is loaded from its file with placeholder modules for the imports that only its command line needs.  Also
printed per case, and stored as <case>_gap_ref / <case>_gap_onepass: the relative gap between the reference's value and the fp64
eigenvalue route (tests/fid_restated.py), and between the FID from one-pass fp64 moments and from two-pass np.cov.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def load_reference(root):
    """metrics/fid_query.py as a module; its __main__ block does not run"""
    names = {'torch.utils.tensorboard': ['SummaryWriter'], 'metrics': [], 'metrics.calc_inception': ['load_patched_inception_v3'],
             'model_spatial_query': ['Generator'], 'utils': [], 'utils.sample': ['prepare_noise_new', 'prepare_param']}
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k, attrs in names.items():
            m = types.ModuleType(k)
            for a in attrs:
                setattr(m, a, None)
            sys.modules[k] = m
        spec = importlib.util.spec_from_file_location('reference_fid_query', os.path.join(root, 'metrics', 'fid_query.py'))
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference repository (its metrics/fid_query.py is loaded)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'fid_ref.npz'))
    a = ap.parse_args()
    ref = load_reference(a.reference)
    import fid_restated as R
    out = {}
    for name, (real, fake) in R.draw_all().items():
        # fid_query.py:162-171: sample = the generated set, real = the statistics file's (calc_inception.py:110-111)
        got = float(np.real(ref.calc_fid(np.mean(fake, 0), np.cov(fake, rowvar=False), np.mean(real, 0), np.cov(real, rowvar=False))))
        mine = R.fid_of_features(fake, real)
        one = R.frechet(*R.one_pass_mean_cov(fake), *R.one_pass_mean_cov(real))
        gap_ref, gap_one = abs(got - mine) / abs(mine), abs(one - mine) / abs(mine)
        print(f'case {name}: real {real.shape} fake {fake.shape}  reference {got!r}  fp64 eigenvalue route {mine!r}  '
              f'relative gap {gap_ref:.2e};  one-pass fp64 moments against two-pass np.cov: relative gap {gap_one:.2e}')
        out[f'{name}_real'], out[f'{name}_fake'] = real, fake
        out[f'{name}_fid'] = np.float64(got)
        out[f'{name}_gap_ref'], out[f'{name}_gap_onepass'] = np.float64(gap_ref), np.float64(gap_one)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes)')


if __name__ == '__main__':
    main()

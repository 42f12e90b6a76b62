"""Writes tests/golden/prdc_ref.npz: what the reference's own metrics/prdc.py (sklearn pairwise_distances, fp32) returns for two seeded
Gaussian cases, with the inputs.  CPU only, seconds.

    python tools/prdc_golden.py --reference /path/to/TransEditor [--out tests/golden/prdc_ref.npz]

Cases (np.random.default_rng(1), real drawn first, then fake, cast to float32):
    a: real (257, 96) ~ N(0,1), fake (130, 96) ~ 0.9 N(0,1) + 0.1, nearest_k = 3
    b: real (129, 33),          fake (67, 33),  the same distributions, nearest_k = 1
Also printed: the fp64 restatement's values (tests/prdc_restated.py) and the smallest relative gap between any squared distance and the
threshold it is compared with, which is what makes the recorded values reproducible by any evaluation accurate to well under that gap.
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CASES = {'a': ((257, 96), (130, 96), 3), 'b': ((129, 33), (67, 33), 1)}
SEED = 1
KEYS = ('precision', 'recall', 'density', 'coverage')


def draw(real_shape, fake_shape, seed=SEED):
    rng = np.random.default_rng(seed)
    real = rng.standard_normal(real_shape).astype(np.float32)
    fake = (0.9 * rng.standard_normal(fake_shape) + 0.1).astype(np.float32)
    return real, fake


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help="root of the reference repository (its metrics/prdc.py is imported)")
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'prdc_ref.npz'))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location('reference_prdc', os.path.join(a.reference, 'metrics', 'prdc.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    import prdc_restated as R
    out = {}
    for name, (rs, fs, k) in CASES.items():
        real, fake = draw(rs, fs)
        with contextlib.redirect_stdout(io.StringIO()):
            got = ref.compute_prdc(real, fake, k)
        d = R.details(real, fake, k)
        mine = R.numbers(d, k)
        print(f'case {name}: real {rs} fake {fs} k={k}  reference {[float(got[x]) for x in KEYS]}  restated {[mine[x] for x in KEYS]}  '
              f'smallest relative gap to a threshold {R.min_relative_gap(d):.2e}')
        out[f'{name}_real'], out[f'{name}_fake'] = real, fake
        out[f'{name}_k'] = np.int64(k)
        out[f'{name}_prdc'] = np.array([float(got[x]) for x in KEYS], np.float64)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes)')


if __name__ == '__main__':
    main()

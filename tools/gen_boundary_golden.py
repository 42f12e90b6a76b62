"""Writes tests/golden/boundary_ref.npz (and with --large tests/golden/boundary_ref_large.npz): what the reference's own train_boundary (our_interfaceGAN/train_boundary.py: sklearn's
SVC(kernel='linear')) and linear_interpolate (our_interfaceGAN/linear_interpolation.py) return on seeded inputs, with the inputs.
CPU only, seconds; needs scikit-learn.

    python tools/gen_boundary_golden.py --reference /path/to/TransEditor [--out tests/golden/boundary_ref.npz]
    python tools/gen_boundary_golden.py --reference /path/to/TransEditor --large [--out tests/golden/boundary_ref_large.npz]

Both functions are executed from the reference's own files; nothing is copied.  One shim: np.int = int (numpy 2 dropped the alias that
train_boundary.py:81 uses).  The cases are tests/svm_restated.py's CASES / draw(): standard normal float32 codes, scores = a random unit
linear functional of the codes plus noise, all from np.random.default_rng(7):
    a: N 1500, D 96, ratio 0.04, noise 0.5  -> n = 120 training rows, separable
    b: N 2000, D 8,  ratio 0.05, noise 2.0  -> n = 200, NOT separable (alphas at the bound C: both clipping branches run)
    c: N 600,  D 33, count 65,   noise 1.0  -> n = 130, separable, the count form of chosen_num_or_ratio
each called with split_ratio = 1.0: the training set is then the whole chosen set and the reference's unseeded shuffle only permutes its
rows, which the optimum does not depend on.  Stored per case: <case>_codes, _scores, _boundary (the reference's), _optimum (the float64
direction of tests/svm_restated.py at eps = 1e-9 on the float64 Gram matrix), _gap_ref / _gap_restated (1 - cos of the reference's and
of the restatement's eps = 1e-3 boundary to that optimum), _gap (1 - cos restatement to reference), _iterations (the restatement's).
li_*: the inputs and outputs of linear_interpolate in its 2-D and its W+ form.
--large writes svm_restated.LARGE_CASES to a file of their own, without the li_* entries; the small file is left alone:
    d: N 6000, D 12, ratio 0.35, noise 1.0  -> n = 4200, the training rows of the reference's default run (150 000 samples, ratio 0.02,
       split 0.7), NOT separable: five rows per thread of the one-workgroup solver of csrc/svm.hip
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


def load_reference(root, name):
    spec = importlib.util.spec_from_file_location('reference_' + name, os.path.join(root, 'our_interfaceGAN', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference repository')
    ap.add_argument('--large', action='store_true', help='the cases above 1024 training rows, to boundary_ref_large.npz')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'tests', 'golden', 'boundary_ref_large.npz' if a.large else 'boundary_ref.npz')
    if not hasattr(np, 'int'):
        np.int = int
    tb = load_reference(a.reference, 'train_boundary')
    li = load_reference(a.reference, 'linear_interpolation')
    import svm_restated as R
    out = {}
    for case in (R.LARGE_CASES if a.large else R.SMALL_CASES):
        N, D, ratio, noise, seed = R.CASES[case]
        codes, scores = R.draw(case)
        with contextlib.redirect_stdout(io.StringIO()):
            boundary = tb.train_boundary(codes, scores, chosen_num_or_ratio=ratio, split_ratio=1.0)
        x, y = R.training_set(codes, scores, ratio)
        alpha, rho, it, conv = R.smo(R.gram32(x), y)
        x64 = x.astype(np.float64)
        alpha9, _, it9, conv9 = R.smo(x64 @ x64.T, y, eps=1e-9)
        assert conv and conv9
        w, w9 = R.direction(x, y, alpha), R.direction(x, y, alpha9)
        gap, gap_ref, gap_rest = R.one_minus_cos(w, boundary), R.one_minus_cos(boundary, w9), R.one_minus_cos(w, w9)
        print(f'case {case}: N {N} D {D} n {len(y)}  restatement: {it} iterations, {int((alpha >= 1.0).sum())} alphas at C, '
              f'{int((alpha > 0).sum())} support vectors' + (f' in slots {R.slots(np.nonzero(alpha > 0)[0])}' if a.large else '')
              + f', rho {rho:.6f};  1 - cos restatement to reference {gap:.2e}, reference to the '
              f'eps=1e-9 optimum {gap_ref:.2e}, restatement to the optimum {gap_rest:.2e}')
        out.update({f'{case}_codes': codes, f'{case}_scores': scores, f'{case}_boundary': boundary.astype(np.float32),
                    f'{case}_optimum': w9, f'{case}_gap': np.float64(gap), f'{case}_gap_ref': np.float64(gap_ref),
                    f'{case}_gap_restated': np.float64(gap_rest), f'{case}_iterations': np.int64(it)})
    if not a.large:
        rng = np.random.default_rng(11)
        b = out['a_boundary']
        code2 = rng.standard_normal((1, b.shape[1])).astype(np.float32)
        code3 = rng.standard_normal((1, 5, b.shape[1])).astype(np.float32)
        out.update(li_boundary=b, li_code2=code2, li_code3=code3, li_start=np.float64(-3.0), li_end=np.float64(2.5), li_steps=np.int64(7),
                   li_out2=li.linear_interpolate(code2, b, start_distance=-3.0, end_distance=2.5, steps=7),
                   li_out3=li.linear_interpolate(code3, b, start_distance=-3.0, end_distance=2.5, steps=7))
        assert out['li_out2'].dtype == np.float32 and out['li_out3'].dtype == np.float32
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f'wrote {a.out} ({os.path.getsize(a.out)} bytes)')


if __name__ == '__main__':
    main()

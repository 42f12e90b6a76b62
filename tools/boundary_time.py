"""Time of the three kernels behind train_boundary (csrc/svm.hip) on the MI355X at the reference's own shape: 150 000 samples at ratio
0.02 and split 0.7 give n = 4200 training rows of D = 8192 (16 tokens x 512).

    python tools/boundary_time.py [--out profiles/edit/boundary_time.json] [--n 4200] [--dim 8192] [--reps 5] [--sklearn]

The rows are drawn as the fixture's (tests/svm_restated.py draw()): standard normal codes, scores = a unit linear functional plus noise
0.5, the n / 2 highest and lowest of 150 000 scores kept; such a set is separable.  Gram, SMO and coef are timed separately: device time
between two events, median of --reps after a warm-up call.  --sklearn also times SVC(kernel='linear').fit on the same rows on this
machine's CPUs (wall time, once), where scikit-learn is importable.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rows(n, dim, total=150000, noise=0.5, seed=7):
    """the n / 2 highest- and the n / 2 lowest-scored of `total` standard normal codes (score = u . code + noise), generated on the
    device in chunks with a running buffer of the extremes, so the 4.9 GB of all codes never exist at once"""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    u = torch.randn(dim, device='cuda', generator=g)
    u /= u.norm()
    half, keep_x, keep_s = n // 2, None, None
    for at in range(0, total, 8192):
        x = torch.randn(min(8192, total - at), dim, device='cuda', generator=g)
        s = x @ u + noise * torch.randn(x.shape[0], device='cuda', generator=g)
        x, s = (x, s) if keep_x is None else (torch.cat([keep_x, x]), torch.cat([keep_s, s]))
        order = torch.argsort(s, descending=True)
        order = order if order.shape[0] <= n else torch.cat([order[:half], order[-half:]])
        keep_x, keep_s = x[order], s[order]
    return keep_x.contiguous()


def device_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return {'ms_all': [round(t, 3) for t in ts], 'ms_median': round(sorted(ts)[len(ts) // 2], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--n', type=int, default=4200)
    ap.add_argument('--dim', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sklearn', action='store_true')
    a = ap.parse_args()
    import numpy as np
    import torch
    from transeditor_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit('boundary_time.py needs a GPU')
    x = rows(a.n, a.dim)
    n = x.shape[0]
    y = np.concatenate([np.ones(n // 2, np.int8), -np.ones(n // 2, np.int8)])
    results = []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)
    r = device_ms(lambda: _lib.gram(x), a.reps)
    r.update(step='gram', n=n, D=a.dim, fp32_tflops_symmetry_counted_once=round(n * (n + 1.0) * a.dim / (r['ms_median'] * 1e-3) / 1e12, 2))
    emit(r)
    K = _lib.gram(x)
    r = device_ms(lambda: _lib.svm_smo(K, y, 1.0, 1e-3), a.reps)
    alpha, rho, info = _lib.svm_smo(K, y, 1.0, 1e-3)
    it, conv = info.tolist()
    r.update(step='smo', n=n, iterations=it, converged=conv, us_per_iteration=round(r['ms_median'] * 1e3 / max(it, 1), 3),
             n_support=int((alpha > 0).sum()), at_bound=int((alpha >= 1.0).sum()))
    emit(r)
    r = device_ms(lambda: _lib.svm_coef(x, alpha, y), a.reps)
    r.update(step='coef', n=n, D=a.dim)
    emit(r)
    if a.sklearn:
        try:
            from sklearn import svm
        except ImportError:
            emit({'step': 'sklearn', 'available': False})
        else:
            xh = x.cpu().numpy()
            t0 = time.perf_counter()
            clf = svm.SVC(kernel='linear').fit(xh, (y > 0).astype(np.int64))
            dt = time.perf_counter() - t0
            w = _lib.svm_coef(x, alpha, y).double().cpu().numpy()
            c = clf.coef_[0]
            emit({'step': 'sklearn', 'available': True, 'n': n, 'D': a.dim, 'wall_s': round(dt, 2), 'iterations': int(clf.n_iter_[0]),
                  'cpus': len(os.sched_getaffinity(0)), 'one_minus_cos_to_gpu': float(1.0 - w @ c / (np.linalg.norm(w) * np.linalg.norm(c)))})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'command': 'python tools/boundary_time.py' + (' --sklearn' if a.sklearn else ''), 'results': results}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

"""Time and accuracy of the PRDC kernels (csrc/prdc.hip) on the MI355X at the reference's defaults: N = M = 50000 samples, D = 4096
features (VGG16 fc7), nearest_k = 3, on random features.

    python tools/prdc_time.py [--out profiles/prdc/prdc_time.json] [--n 50000] [--d 4096] [--k 3] [--reps 3]

The three passes (k-NN radii of the real set, of the fake set, the real x fake counts) and the accuracy check run as separate child
processes, each under a time limit of its own; the first one that fails ends the run.  Each pass is 2 N M D FLOP; the figure to hold
it against is the fp32 matrix peak, 157.3 TFLOP/s (the fp32-input MFMA runs at the fp32 vector rate).
  accuracy: Gaussian features at N = M = 2048, D = 512: how many of the 2 N M + N threshold comparisons (d2 < rr2[i], d2 < rf2[j],
  row_min < rr2) come out differently from float64 (direct sum of squared differences, float64 radii), and the largest error of d2
  itself, probed through row_min and the radii.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3
STEPS = (('knn_real', 240), ('knn_fake', 240), ('counts', 300), ('accuracy', 240))


def features(n, d, seed, shift):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(n, d, device='cuda', generator=g)
    return x * 0.9 + 0.1 if shift else x


def timed(fn, reps):
    import torch
    fn()                                                       # first call: code-object load, allocator growth
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return ts


def step_pass(a):
    from transeditor_amd import _lib
    n, d, k = a.n, a.d, a.k
    if a.step in ('knn_real', 'knn_fake'):
        x = features(n, d, 1 if a.step == 'knn_real' else 2, a.step == 'knn_fake')
        nx = _lib.row_sqnorm(x)
        ts = timed(lambda: _lib.prdc_knn(x, nx, k), a.reps)
    else:
        x, y = features(n, d, 1, False), features(n, d, 2, True)
        nx, ny = _lib.row_sqnorm(x), _lib.row_sqnorm(y)
        rr2, rf2 = _lib.prdc_knn(x, nx, k), _lib.prdc_knn(y, ny, k)
        ts = timed(lambda: _lib.prdc_counts(x, nx, rr2, y, ny, rf2), a.reps)
    med = sorted(ts)[len(ts) // 2]
    tf = 2.0 * n * n * d / (med * 1e-3) / 1e12
    return {'step': a.step, 'N': n, 'M': n, 'D': d, 'k': k, 'ms_all': [round(t, 3) for t in ts], 'ms_median': round(med, 3),
            'tflops': round(tf, 2), 'fraction_of_fp32_matrix_peak': round(tf / PEAK_TFLOPS, 4)}


def step_accuracy(a):
    import torch
    from transeditor_amd import _lib
    n, d, k = 2048, 512, a.k
    x, y = features(n, d, 1, False), features(n, d, 2, True)
    nx, ny = _lib.row_sqnorm(x), _lib.row_sqnorm(y)
    rr2, rf2 = _lib.prdc_knn(x, nx, k), _lib.prdc_knn(y, ny, k)
    cc, ra, rm = _lib.prdc_counts(x, nx, rr2, y, ny, rf2)

    def d2_64(p, q):
        out = torch.empty(p.shape[0], q.shape[0], device='cuda', dtype=torch.float64)
        for s in range(0, p.shape[0], 64):
            out[s:s + 64] = ((p[s:s + 64, None, :].double() - q[None, :, :].double()) ** 2).sum(-1)
        return out
    dxx, dyy, dxy = d2_64(x, x), d2_64(y, y), d2_64(x, y)
    dxx.fill_diagonal_(0)
    dyy.fill_diagonal_(0)
    r64, f64 = dxx.sort(1).values[:, k], dyy.sort(1).values[:, k]
    in_real, in_fake = dxy < r64[:, None], dxy < f64[None, :]
    # the kernel gives the reductions, not the matrix: a differing comparison shows as a differing count / flag
    diff = int((cc.long() - in_real.sum(0)).abs().sum()) + int(((ra != 0) != in_fake.any(1)).sum()) + \
        int(((rm < rr2) != (dxy.min(1).values < r64)).sum())
    scale = (nx.double()[:, None] + ny.double()[None, :]).max()
    return {'step': 'accuracy', 'N': n, 'M': n, 'D': d, 'k': k, 'comparisons': 2 * n * n + n,
            'comparisons_differing_from_fp64': diff,
            'max_abs_err_rr2': float((rr2.double() - r64).abs().max()), 'max_abs_err_rf2': float((rf2.double() - f64).abs().max()),
            'max_abs_err_row_min': float((rm.double() - dxy.min(1).values).abs().max()),
            'max_rel_err_row_min': float(((rm.double() - dxy.min(1).values).abs() / dxy.min(1).values).max()),
            'largest_nx_plus_ny': float(scale),
            'smallest_relative_gap_to_a_threshold_fp64': float(min(((dxy - r64[:, None]).abs() / r64[:, None]).min(),
                                                                   ((dxy - f64[None, :]).abs() / f64[None, :]).min()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--n', type=int, default=50000)
    ap.add_argument('--d', type=int, default=4096)
    ap.add_argument('--k', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--step', choices=[s for s, _ in STEPS], default=None, help='(internal) run one step in this process')
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('prdc_time.py needs a GPU')
        print(json.dumps(step_accuracy(a) if a.step == 'accuracy' else step_pass(a)), flush=True)
        return
    results = []
    for step, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--n', str(a.n), '--d', str(a.d), '--k', str(a.k),
               '--reps', str(a.reps)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f'prdc_time.py: step {step} exceeded its {limit} s limit; nothing further is started')
        if p.returncode != 0:
            raise SystemExit(f'prdc_time.py: step {step} failed with status {p.returncode}; nothing further is started\n{p.stderr[-2000:]}')
        res = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'command': 'python tools/prdc_time.py', 'fp32_matrix_peak_tflops': PEAK_TFLOPS, 'results': results}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

"""Time of the FID feature moments (csrc/fid.hip) on the MI355X at the reference's n_sample = 50000, against the reference's host path.

    python tools/fid_time.py [--out profiles/fid/fid_time.json] [--n 50000] [--reps 5] [--steps moments,stream,host,generator]

  moments   : one te_fid_moments_f64 call on [n, D] features, D = 2048 (Inception pool3) and 4096 (VGG16 fc7): device time between two
              events, median of --reps after a warm-up call.  TFLOP/s counts the symmetric product once: n D (D + 1) FLOP.
  stream    : a full FeatureStats stream of the same features in batches of 64 (chunk = 4096) up to and including finalize()'s copy of
              mean and cov to the host: wall time, the host synchronised before and after.
  host      : what the reference does with the same batches (fid_query.py:38-40, :162-163): feat.to('cpu') per batch, torch.cat, np.mean
              and np.cov on this machine's CPUs: wall time.  D = 2048 only.
  generator : a 256-px GeneratorSampler at batch 64, device time per batch, scaled to the 782 batches of a 50000-image evaluate_fid, to
              state the share of the moments next to it.
Every step runs in a child process under a time limit of its own; the first one that fails ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {'moments': 240, 'stream': 240, 'host': 420, 'generator': 300}
BATCH = 64


def features(n, d):
    """non-negative, like pooled ReLU features; generated on the device in pieces"""
    import torch
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.empty(n, d, device='cuda')
    for a in range(0, n, 8192):
        x[a:a + 8192] = torch.relu(torch.randn(min(8192, n - a), d, device='cuda', generator=g) * 0.9 + 0.3)
    return x


def device_ms(fn, reps):
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


def wall_ms(fn, reps):
    import torch
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def summary(ts):
    return {'ms_all': [round(t, 3) for t in ts], 'ms_median': round(sorted(ts)[len(ts) // 2], 3)}


def step_moments(a):
    import torch
    from transeditor_amd import _lib
    out = []
    for d in (2048, 4096):
        x = features(a.n, d)
        S = torch.empty(d, d, device='cuda', dtype=torch.float64)
        s = torch.empty(d, device='cuda', dtype=torch.float64)
        r = summary(device_ms(lambda: _lib.fid_moments(S, s, x, False), a.reps))
        r.update(step='moments', N=a.n, D=d, ws_bytes=_lib.fid_moments_ws_bytes(a.n, d),
                 fp64_tflops_symmetry_counted_once=round(a.n * d * (d + 1.0) / (r['ms_median'] * 1e-3) / 1e12, 2))
        out.append(r)
        del x, S, s
    return out


def step_stream(a):
    from transeditor_amd import fid
    out = []
    for d in (2048, 4096):
        x = features(a.n, d)

        def run():
            st = fid.FeatureStats(d)
            for at in range(0, a.n, BATCH):
                st.update(x[at:at + BATCH])
            return st.finalize()
        r = summary(wall_ms(run, max(2, a.reps // 2)))
        r.update(step='stream', N=a.n, D=d, batch=BATCH, chunk=4096)
        out.append(r)
        del x
    return out


def step_host(a):
    import numpy as np
    import torch
    d = 2048
    x = features(a.n, d)

    def run():
        feats = [x[at:at + BATCH].to('cpu') for at in range(0, a.n, BATCH)]           # fid_query.py:38
        f = torch.cat(feats, 0).numpy()
        return np.mean(f, 0), np.cov(f, rowvar=False)                                  # :162-163
    r = summary(wall_ms(run, 2))
    r.update(step='host', N=a.n, D=d, batch=BATCH, cpus=len(os.sched_getaffinity(0)), omp_num_threads=os.environ.get('OMP_NUM_THREADS'))
    return [r]


def step_generator(a):
    import math
    import types
    import torch
    from transeditor_amd import synth
    from transeditor_amd.inference import GeneratorSampler
    from transeditor_amd.model_spatial_query import Generator
    from transeditor_amd.utils.sample import prepare_noise_new, prepare_param
    size = 256
    G = Generator(size, 512, 512, 2 * (int(math.log(size, 2)) - 1), n_trans=8, pixel_norm_op_dim=1)
    sd = G.state_dict()
    synth.fill_state_dict(sd, 21)
    G.load_state_dict(sd)
    g = GeneratorSampler(G.to('cuda'))
    args = types.SimpleNamespace(latent=512, para_num=16)
    z, p = prepare_noise_new(BATCH, args, 'cuda', method='query'), prepare_param(BATCH, args, 'cuda', method='spatial')
    with torch.no_grad():
        g(z, p)
        r = summary(device_ms(lambda: g(z, p), a.reps))
    batches = -(-a.n // BATCH)
    r.update(step='generator', size=size, batch=BATCH, batches_per_evaluation=batches, ms_per_evaluation=round(r['ms_median'] * batches, 1))
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--n', type=int, default=50000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', default='moments,stream,host,generator')
    ap.add_argument('--step', choices=list(LIMITS), default=None, help='(internal) run one step in this process')
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('fid_time.py needs a GPU')
        for r in globals()['step_' + a.step](a):
            print(json.dumps(r), flush=True)
        return
    results = []
    for step in a.steps.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--n', str(a.n), '--reps', str(a.reps)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=LIMITS[step], text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f'fid_time.py: step {step} exceeded its {LIMITS[step]} s limit; nothing further is started')
        if p.returncode != 0:
            raise SystemExit(f'fid_time.py: step {step} failed with status {p.returncode}; nothing further is started\n{p.stderr[-2000:]}')
        for line in p.stdout.strip().splitlines():
            if line.startswith('{'):
                print(line, flush=True)
                results.append(json.loads(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'command': 'python tools/fid_time.py', 'results': results}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

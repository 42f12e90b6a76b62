"""Time of the DEX age / gender scorer (transeditor_amd.dex, csrc/dex.hip) on the MI355X, random weights of the true geometry (224 px
crop, 4096 / 4096, 101 classes).

    python tools/dex_time.py [--batches 16 64] [--size 256] [--reps 5] [--no-torch] [--out profiles/dex/net_time.json]

Reports, per batch size, for images in [-1, 1]:
  library : DEXScorer.forward, images/s from HIP events around whole forward passes (median of --reps after one untimed call);
  shares  : one more pass with a pair of HIP events around every library call, summed per kernel family (the fused stem, the trunk
            convolutions, their ReLU passes, the max-pools, the two fc layers, the softmax / score head).  The events of a single call
            include its launch gap, so the families add up to a little more than the whole pass; the shares are of their own sum;
  torch   : the SAME network (the same weights) written in plain torch ops on the same device: indexing, clamp / add / div / mul / round,
            slicing, F.conv2d, F.max_pool2d, F.linear, F.softmax.  A yardstick, not a part of the product; the largest relative
            difference between the two score vectors is printed.
Run under `rocprofv3 --kernel-trace --stats -- python tools/dex_time.py --batches 64 --no-torch` for per-kernel times
(tools/rocpd_stats.py summarises the trace).  GPU only.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, reps):
    fn()                                                       # first call: code-object load, allocator growth, weight packing
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return sorted(ts)[len(ts) // 2], ts


FAMILIES = {'dex_stem_fwd': 'stem (te_dex_stem_fwd_f32)', 'conv': 'trunk convolutions', 'maxpool2_fwd': 'max-pools',
            'fc_stream': 'fc1 + fc2 (te_fc_stream_f32)', 'cls_score': 'head (te_cls_score_f32)'}


def shares(scorer, x):
    """one forward pass with HIP events around every library call -> {family: (ms, calls)}"""
    from transeditor_amd import _lib, lpips
    log = []

    def wrap(fn, family):
        def run(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            log.append((family, s, e))
            return out
        return run
    saved = {n: getattr(_lib, n) for n in FAMILIES}
    relu = lpips._relu_
    try:
        for n, family in FAMILIES.items():
            setattr(_lib, n, wrap(saved[n], family))
        lpips._relu_ = wrap(relu, 'trunk ReLU passes')
        scorer(x)
        torch.cuda.synchronize()
    finally:
        for n, fn in saved.items():
            setattr(_lib, n, fn)
        lpips._relu_ = relu
    out = {}
    for family, s, e in log:
        ms, calls = out.get(family, (0.0, 0))
        out[family] = (ms + s.elapsed_time(e), calls + 1)
    return out


def torch_network(scorer):
    """the scorer in plain torch ops on the device, with the scorer's own weights"""
    crop, mode = scorer.crop, scorer.mode
    pool_before = (2, 4, 7, 10)

    @torch.no_grad()
    def run(x):
        o = (x.shape[2] - crop) // 2
        h = x[:, [2, 1, 0]].clamp(-1, 1).add(1).div(2).mul(255).round()[:, :, o:o + crop, o:o + crop]
        for i in range(13):
            if i in pool_before:
                h = F.max_pool2d(h, 2, 2)
            h = F.relu(F.conv2d(h, getattr(scorer, f'w{i}'), getattr(scorer, f'b{i}'), padding=1))
        h = F.max_pool2d(h, 2, 2).flatten(1)
        h = F.relu(F.linear(h, scorer.fc1_w, scorer.fc1_b))
        h = F.relu(F.linear(h, scorer.fc2_w, scorer.fc2_b))
        p = F.softmax(F.linear(h, scorer.cls_w, scorer.cls_b), 1)
        if mode == 0:
            return (p * torch.arange(1, p.shape[1] + 1, device=p.device, dtype=p.dtype)).sum(1)
        return p[:, 0]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[16, 64])
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch yardstick')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dex_time.py needs a GPU')
    import dex_restated as R
    from transeditor_amd.dex import DEXScorer
    scorer = DEXScorer(state_dict=R.state_dict(2), attribute='age')
    ref_run = None if a.no_torch else torch_network(scorer)
    res = {'command': ' '.join(['python tools/dex_time.py'] + sys.argv[1:]), 'size': a.size, 'crop': scorer.crop, 'runs': []}
    for batch in a.batches:
        x = 0.6 * torch.randn(batch, 3, a.size, a.size, device='cuda', generator=torch.Generator(device='cuda').manual_seed(batch))
        med, ts = timed(lambda: scorer(x), a.reps)
        one = {'batch': batch, 'library': {'ms_median': round(med, 3), 'ms_all': [round(t, 3) for t in ts],
                                           'images_per_s': round(batch / (med * 1e-3), 1)}}
        sh = shares(scorer, x)
        total = sum(v[0] for v in sh.values())
        one['shares'] = {k: {'ms': round(ms, 3), 'calls': n, 'share': round(ms / total, 4)} for k, (ms, n) in
                         sorted(sh.items(), key=lambda kv: -kv[1][0])}
        one['shares_sum_ms'] = round(total, 3)
        if ref_run is not None:
            medt, tst = timed(lambda: ref_run(x), a.reps)
            one['torch'] = {'ms_median': round(medt, 3), 'ms_all': [round(t, 3) for t in tst], 'images_per_s': round(batch / (medt * 1e-3), 1)}
            lib, ref = scorer(x).double(), ref_run(x).double()
            one['max_relative_score_difference_from_torch'] = float(((lib - ref).abs() / ref.abs()).max())
            one['library_time_over_torch_time'] = round(med / medt, 3)
        res['runs'].append(one)
        print(json.dumps(one), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

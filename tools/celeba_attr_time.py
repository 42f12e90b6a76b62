"""Time of the CelebA-HQ attribute scorer (transeditor_amd.celeba_attr, csrc/celeba_attr.hip) on the MI355X, random weights of the true
geometry (R = 256, 64 ... 512 channels, 13 3x3 convolutions).

    python tools/celeba_attr_time.py [--batches 16 64] [--size 256] [--reps 7] [--no-torch] [--out profiles/celeba_attr/net_time.json]

Reports, per batch size, for images in [-1, 1]:
  library : CelebAAttributeScorer.forward, images/s from HIP events around whole forward passes (median of --reps after one untimed call);
  shares  : one more pass with a pair of HIP events around every library call, summed per kernel family (the fused stem, the
            convolutions by route, the pool passes, dense0, the score head).  The events of a single call include its launch gap, so the
            families add up to a little more than the whole pass; the shares are of their own sum;
  torch   : the SAME network (the same scaled weights) written in plain torch ops on the same device: indexing, clamp / add / div / mul /
            round, the view + mean box filter, F.conv2d, F.leaky_relu, F.avg_pool2d, F.linear, F.softmax.  A yardstick, not a part of
            the product; the largest absolute difference between the two score vectors is printed.
Run under `rocprofv3 --kernel-trace --stats -- python tools/celeba_attr_time.py --batches 64 --no-torch --reps 3` for per-kernel times
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


FAMILIES = {'attr_stem_fwd': 'stem (te_attr_stem_fwd_f32)', 'avgpool2_act': 'pool passes (te_avgpool2_act_f32)',
            'fc_stream': 'dense0 (te_fc_stream_f32)', 'attr_score': 'head (te_attr_score_f32)'}


def shares(scorer, x):
    """one forward pass with HIP events around every library call -> {family: (ms, calls)}"""
    from transeditor_amd import _lib
    routes = {_lib.CONV_3X3: 'convolutions, TE_CONV_3X3', _lib.CONV_3X3W: 'convolutions, TE_CONV_3X3W', _lib.CONV_3X3W6: 'convolutions, TE_CONV_3X3W6'}
    log = []

    def wrap(fn, family):
        def run(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            log.append((family(a) if callable(family) else family, s, e))
            return out
        return run
    saved = {n: getattr(_lib, n) for n in list(FAMILIES) + ['conv']}
    try:
        for n, family in FAMILIES.items():
            setattr(_lib, n, wrap(saved[n], family))
        _lib.conv = wrap(saved['conv'], lambda a: routes[a[2]])                 # conv(x, wp, kind, ...)
        scorer(x)
        torch.cuda.synchronize()
    finally:
        for n, fn in saved.items():
            setattr(_lib, n, fn)
    out = {}
    for family, s, e in log:
        ms, calls = out.get(family, (0.0, 0))
        out[family] = (ms + s.elapsed_time(e), calls + 1)
    return out


def torch_network(scorer):
    """the scorer in plain torch ops on the device, with the scorer's own (scaled) weights"""
    R, n = scorer.resolution, scorer.n_convs

    @torch.no_grad()
    def run(x):
        h = x[:, [2, 1, 0]].clamp(-1, 1).add(1).div(2).mul(255).round()
        f = h.shape[2] // R
        if f > 1:
            h = h.view(h.shape[0], 3, R, f, R, f).mean(dim=[3, 5])
        h = F.leaky_relu(F.conv2d(h, scorer.stem_w.view(-1, 3, 1, 1), scorer.stem_b), 0.2)
        for i in range(0, n - 1, 2):
            h = F.leaky_relu(F.conv2d(h, getattr(scorer, f'w{i}'), getattr(scorer, f'b{i}'), padding=1), 0.2)
            h = F.leaky_relu(F.avg_pool2d(F.conv2d(h, getattr(scorer, f'w{i + 1}'), getattr(scorer, f'b{i + 1}'), padding=1), 2, 2), 0.2)
        h = F.leaky_relu(F.conv2d(h, getattr(scorer, f'w{n - 1}'), getattr(scorer, f'b{n - 1}'), padding=1), 0.2).flatten(1)
        h = F.leaky_relu(F.linear(h, scorer.dense0_w, scorer.dense0_b), 0.2)
        l = F.linear(h, scorer.dense1_w.view(1, -1), scorer.dense1_b)
        return F.softmax(torch.cat([l, -l], 1), 1)[:, 1]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[16, 64])
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch yardstick')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('celeba_attr_time.py needs a GPU')
    import celeba_attr_restated as R
    from transeditor_amd.celeba_attr import CelebAAttributeScorer
    scorer = CelebAAttributeScorer(state_dict=R.state_dict(2, 256))
    ref_run = None if a.no_torch else torch_network(scorer)
    res = {'command': ' '.join(['python tools/celeba_attr_time.py'] + sys.argv[1:]), 'size': a.size, 'resolution': scorer.resolution,
           'channels': list(scorer.channels), 'runs': []}
    for batch in a.batches:
        x = R.images(batch, batch, a.size).to('cuda')
        med, ts = timed(lambda: scorer(x), a.reps)
        one = {'batch': batch, 'library': {'ms_median': round(med, 3), 'ms_all': [round(t, 3) for t in ts],
                                           'images_per_s': round(batch / (med * 1e-3), 1)},
               'routes': [[H, kind] for H, kind in scorer.conv_routes(batch)]}
        sh = shares(scorer, x)
        total = sum(v[0] for v in sh.values())
        one['shares'] = {k: {'ms': round(ms, 3), 'calls': n, 'share': round(ms / total, 4)} for k, (ms, n) in
                         sorted(sh.items(), key=lambda kv: -kv[1][0])}
        one['shares_sum_ms'] = round(total, 3)
        if ref_run is not None:
            medt, tst = timed(lambda: ref_run(x), a.reps)
            one['torch'] = {'ms_median': round(medt, 3), 'ms_all': [round(t, 3) for t in tst], 'images_per_s': round(batch / (medt * 1e-3), 1)}
            lib, ref = scorer(x).double(), ref_run(x).double()
            one['score_range'] = [float(lib.min()), float(lib.max())]
            one['max_absolute_score_difference_from_torch'] = float((lib - ref).abs().max())
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

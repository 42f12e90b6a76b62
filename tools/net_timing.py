"""What the timing tools of the frozen evaluation networks share (dex_time.py, celeba_attr_time.py, vgg_features_time.py,
inception_time.py): the import path, timed(), the event-wrapping of library calls, the JSON writing, and the main loop of the two
scorer tools.  Each tool keeps its own family table and its own torch yardstick network.  GPU only."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402


def timed(fn, reps):
    """-> (median ms, [ms]) of `reps` calls between HIP events, after one untimed call"""
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


def event_log(run, wraps):
    """run() once with a pair of HIP events around every call of the wrapped functions.  wraps: [(owner, attribute, tag)], where tag is
    the call's label or a function (out, *args, **kwargs) -> label.  -> [(label, ms)] in call order"""
    log = []

    def wrap(fn, tag):
        def call(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            log.append((tag(out, *a, **k) if callable(tag) else tag, s, e))
            return out
        return call
    saved = [(owner, name, getattr(owner, name)) for owner, name, _ in wraps]
    try:
        for owner, name, tag in wraps:
            setattr(owner, name, wrap(getattr(owner, name), tag))
        run()
        torch.cuda.synchronize()
    finally:
        for owner, name, fn in saved:
            setattr(owner, name, fn)
    return [(label, s.elapsed_time(e)) for label, s, e in log]


def shares(run, wraps):
    """event_log summed per label -> {label: (ms, calls)}"""
    out = {}
    for label, t in event_log(run, wraps):
        ms, calls = out.get(label, (0.0, 0))
        out[label] = (ms + t, calls + 1)
    return out


def rate(med, ts, batch, digits=3):
    return {'ms_median': round(med, digits), 'ms_all': [round(t, digits) for t in ts], 'images_per_s': round(batch / (med * 1e-3), 1)}


def write_json(res, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


def scorer_main(tool, reps, build, images, wraps, torch_network, compare, per_batch=lambda scorer, batch: {}):
    """the command line and the per-batch loop of dex_time.py / celeba_attr_time.py.  build() -> (scorer, the report's own header
    fields); images(batch, size) -> the input; compare(library scores, torch scores) -> the tool's difference fields."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[16, 64])
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=reps)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch yardstick')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f'{tool} needs a GPU')
    scorer, header = build()
    ref_run = None if a.no_torch else torch_network(scorer)
    res = {'command': ' '.join([f'python tools/{tool}'] + sys.argv[1:]), 'size': a.size, **header, 'runs': []}
    for batch in a.batches:
        x = images(batch, a.size)
        med, ts = timed(lambda: scorer(x), a.reps)
        one = {'batch': batch, 'library': rate(med, ts, batch), **per_batch(scorer, batch)}
        sh = shares(lambda: scorer(x), wraps)
        total = sum(v[0] for v in sh.values())
        one['shares'] = {k: {'ms': round(ms, 3), 'calls': n, 'share': round(ms / total, 4)} for k, (ms, n) in
                         sorted(sh.items(), key=lambda kv: -kv[1][0])}
        one['shares_sum_ms'] = round(total, 3)
        if ref_run is not None:
            medt, tst = timed(lambda: ref_run(x), a.reps)
            one['torch'] = rate(medt, tst, batch)
            one.update(compare(scorer(x).double(), ref_run(x).double()))
            one['library_time_over_torch_time'] = round(med / medt, 3)
        res['runs'].append(one)
        print(json.dumps(one), flush=True)
    write_json(res, a.out)

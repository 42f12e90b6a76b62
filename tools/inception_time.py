"""Time of the Inception-v3 pool3 feature extractor (transeditor_amd.inception_features, csrc/conv2d.hip) on the MI355X, random weights.

    python tools/inception_time.py [--batch 64] [--size 256] [--reps 5] [--no-torch] [--out profiles/inception/net_time.json]

Reports, for a batch of images in [-1, 1]:
  library : InceptionV3Features.forward, images/s from HIP events around whole forward passes (median of --reps after one untimed call);
  shares  : one more pass with a pair of HIP events around every library call, summed per layer kind (the convolutions by kernel
            geometry and stride, the pools, the resize, the global average).  The events of a single call include its launch gap, so
            the kinds add up to a little more than the whole pass; the shares are of their own sum;
  torch   : the SAME network (the same folded weights, the restatement's graph with torch.cat) run by torch on the device: F.conv2d,
            F.max_pool2d, F.avg_pool2d, F.interpolate.  A yardstick, not a part of the product; rel_l2 between the two outputs is printed.
Run under `rocprofv3 --kernel-trace --stats -- python tools/inception_time.py --no-torch` for per-kernel times.  GPU only.
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
    fn()                                                       # first call: code-object load, allocator growth, kernel selection
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


def conv_kind(w, stride):
    kh, kw = w.shape[2:]
    if (kh, kw) in ((1, 7), (7, 1)):
        return 'conv 1x7 / 7x1'
    if (kh, kw) in ((1, 3), (3, 1)):
        return 'conv 1x3 / 3x1'
    return f'conv {kh}x{kw}' + (' stride 2' if stride == 2 else '')


def shares(net, x):
    """one forward pass with HIP events around every library call -> {kind: (ms, calls, GFLOP)}"""
    from transeditor_amd import _lib
    log = []

    def wrap(fn, kind_of, flop_of):
        def run(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            log.append((kind_of(*a, **k), s, e, flop_of(out, *a, **k)))
            return out
        return run
    saved = {n: getattr(_lib, n) for n in ('conv2d', 'pool3', 'resize_bilinear', 'adaptive_avgpool')}

    def conv_flop(out, x_, w, *a, c0=0, **k):
        Co, Ci, kh, kw = w.shape
        return 2.0 * x_.shape[0] * out.shape[2] * out.shape[3] * Co * Ci * kh * kw
    try:
        _lib.conv2d = wrap(saved['conv2d'], lambda x_, w, b, stride=1, *a, **k: conv_kind(w, stride), conv_flop)
        _lib.pool3 = wrap(saved['pool3'], lambda *a, **k: 'pool 3x3', lambda *a, **k: 0.0)
        _lib.resize_bilinear = wrap(saved['resize_bilinear'], lambda *a, **k: 'resize', lambda *a, **k: 0.0)
        _lib.adaptive_avgpool = wrap(saved['adaptive_avgpool'], lambda *a, **k: 'global average', lambda *a, **k: 0.0)
        net(x)
        torch.cuda.synchronize()
    finally:
        for n, fn in saved.items():
            setattr(_lib, n, fn)
    out = {}
    for kind, s, e, flop in log:
        ms, calls, gf = out.get(kind, (0.0, 0, 0.0))
        out[kind] = (ms + s.elapsed_time(e), calls + 1, gf + flop / 1e9)
    return out


def torch_network(net):
    """the restatement's graph on the device with the library's folded weights: conv + bias + ReLU by F.conv2d"""
    import inception_restated as R

    class DeviceNet(R._Net):
        def __init__(self):
            pass

        def conv(self, name, x, stride=1, padding=0):
            i = net._spec[name][0]
            return F.relu(F.conv2d(x, getattr(net, f'w{i}'), getattr(net, f'b{i}'), stride=stride, padding=padding))
    dn = DeviceNet()

    @torch.no_grad()
    def run(x):
        if net.resize_input:
            x = F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False)
        return F.adaptive_avg_pool2d(dn.trunk(x), 1).flatten(1)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch yardstick')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('inception_time.py needs a GPU')
    import inception_restated as R
    from transeditor_amd.inception_features import InceptionV3Features
    net = InceptionV3Features(state_dict=R.state_dict(seed=2))
    x = torch.rand(a.batch, 3, a.size, a.size, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * 2 - 1
    res = {'command': ' '.join(['python tools/inception_time.py'] + sys.argv[1:]), 'batch': a.batch, 'size': a.size}
    med, ts = timed(lambda: net(x), a.reps)
    res['library'] = {'ms_median': round(med, 2), 'ms_all': [round(t, 2) for t in ts], 'images_per_s': round(a.batch / (med * 1e-3), 1)}
    sh = shares(net, x)
    total = sum(v[0] for v in sh.values())
    res['shares'] = {k: {'ms': round(ms, 3), 'calls': n, 'share': round(ms / total, 4), 'gflop': round(gf, 1),
                         'tflops': round(gf / ms, 1) if gf else None}
                     for k, (ms, n, gf) in sorted(sh.items(), key=lambda kv: -kv[1][0])}
    res['shares_sum_ms'] = round(total, 2)
    res['conv_gflop'] = round(sum(v[2] for v in sh.values()), 1)
    res['conv_tflops_of_the_whole_pass'] = round(res['conv_gflop'] / med, 1)
    if not a.no_torch:
        ref_run = torch_network(net)
        medt, tst = timed(lambda: ref_run(x), a.reps)
        res['torch'] = {'ms_median': round(medt, 2), 'ms_all': [round(t, 2) for t in tst], 'images_per_s': round(a.batch / (medt * 1e-3), 1)}
        lib, ref = net(x).double(), ref_run(x).double()
        res['rel_l2_library_against_torch'] = float((lib - ref).norm() / ref.norm())
        res['library_time_over_torch_time'] = round(med / medt, 2)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

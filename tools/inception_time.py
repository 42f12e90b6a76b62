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
import sys

import torch
import torch.nn.functional as F

from net_timing import event_log, rate, timed, write_json


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

    def conv(out, x_, w, b, stride=1, *a, **k):
        Co, Ci, kh, kw = w.shape
        return conv_kind(w, stride), 2.0 * x_.shape[0] * out.shape[2] * out.shape[3] * Co * Ci * kh * kw
    log = event_log(lambda: net(x), [(_lib, 'conv2d', conv), (_lib, 'pool3', ('pool 3x3', 0.0)), (_lib, 'resize_bilinear', ('resize', 0.0)),
                                     (_lib, 'adaptive_avgpool', ('global average', 0.0))])
    out = {}
    for (kind, flop), t in log:
        ms, calls, gf = out.get(kind, (0.0, 0, 0.0))
        out[kind] = (ms + t, calls + 1, gf + flop / 1e9)
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
    res['library'] = rate(med, ts, a.batch, 2)
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
        res['torch'] = rate(medt, tst, a.batch, 2)
        lib, ref = net(x).double(), ref_run(x).double()
        res['rel_l2_library_against_torch'] = float((lib - ref).norm() / ref.norm())
        res['library_time_over_torch_time'] = round(med / medt, 2)
    print(json.dumps(res), flush=True)
    write_json(res, a.out)


if __name__ == '__main__':
    main()

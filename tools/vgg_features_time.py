"""Time of the VGG16 fc7 feature extractor (transeditor_amd.vgg_features, csrc/vggfc.hip) on the MI355X, random weights.

    python tools/vgg_features_time.py fc6 [--reps 10] [--out profiles/vgg_features/fc6_time.json]
    python tools/vgg_features_time.py net [--batch 64] [--size 256] [--reps 5] [--out profiles/vgg_features/net_time.json]

fc6: te_fc_stream_f32 at I = 64, J = 4096, K = 25088 (bias, no activation) and, on the same operands in the same process, the route the
     library had before it: te_small_gemm_splitk_f32 with W addressed through strides, at every split it accepts of 8 ... 64.  HIP events
     around each call after one untimed call; the two results are compared.  GB/s = the weight's 411 MB over the time; the floors to
     hold it against are 85 us (2 I J K FLOP at the 155 TFLOP/s fp32-MFMA rate) and 65 us (the weight at 6.3 TB/s).
net: VGG16Features.forward on a batch of images: images/s from HIP events.
Run either under `rocprofv3 --kernel-trace --stats -- python tools/vgg_features_time.py ...` for per-kernel times (tools/rocpd_stats.py
summarises the trace): the events include launch gaps, the trace does not.  GPU only.
"""
import argparse
import json
import sys

import torch

import net_timing


def timed(fn, reps):
    """net_timing.timed in microseconds"""
    med, ts = net_timing.timed(fn, reps)
    return med * 1e3, [t * 1e3 for t in ts]


def fc6(a):
    from transeditor_amd import _lib
    I, J, K = 64, 4096, 25088
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(I, K, device='cuda', generator=g).relu_()
    w = torch.randn(J, K, device='cuda', generator=g) * (2.0 / K) ** 0.5
    b = torch.randn(J, device='cuda', generator=g) * 0.05
    res = {'I': I, 'J': J, 'K': K, 'weight_MB': J * K * 4 / 1e6, 'fc_stream_splits': _lib.fc_stream_splits(J, K)}
    med, ts = timed(lambda: _lib.fc_stream(x, w, b, act=0), a.reps)
    res['te_fc_stream_f32'] = {'us_median': round(med, 1), 'us_all': [round(t, 1) for t in ts], 'weight_GB_per_s': round(J * K * 4 / med / 1e3, 1),
                               'tflops': round(2.0 * I * J * K / med / 1e6, 1)}
    c = _lib.fc_stream(x, w, b, act=0)
    old = {}
    for S in (8, 16, 32, 64):
        if K % S or (K // S) % 8:
            continue
        med, ts = timed(lambda: _lib.small_gemm_splitk(I, J, K, S, x, K, 1, w, 1, K, bias=b)[0], a.reps)
        old[S] = {'us_median': round(med, 1), 'us_all': [round(t, 1) for t in ts]}
        c0 = _lib.small_gemm_splitk(I, J, K, S, x, K, 1, w, 1, K, bias=b)[0]
        old[S]['rel_l2_difference_from_fc_stream'] = float((c0.double() - c.double()).norm() / c.double().norm())
    res['te_small_gemm_splitk_f32'] = old
    ref = x.double() @ w.double().T + b.double()
    res['fc_stream_rel_l2_error_against_fp64'] = float((c.double() - ref).norm() / ref.norm())
    return res


def net(a):
    import vgg_restated as R
    from transeditor_amd.vgg_features import VGG16Features
    vgg = VGG16Features(state_dict=R.full_state_dict(seed=2, device='cuda'))
    x = torch.rand(a.batch, 3, a.size, a.size, device='cuda') * 2 - 1
    med, ts = timed(lambda: vgg(x), a.reps)
    return {'batch': a.batch, 'size': a.size, 'ms_median': round(med / 1e3, 2), 'ms_all': [round(t / 1e3, 2) for t in ts],
            'images_per_s': round(a.batch / (med * 1e-6), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['fc6', 'net'])
    ap.add_argument('--reps', type=int, default=None)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vgg_features_time.py needs a GPU')
    if a.reps is None:
        a.reps = 10 if a.what == 'fc6' else 5
    res = {'command': ' '.join(['python tools/vgg_features_time.py'] + [x for x in sys.argv[1:]])}
    res.update(fc6(a) if a.what == 'fc6' else net(a))
    print(json.dumps(res), flush=True)
    net_timing.write_json(res, a.out)


if __name__ == '__main__':
    main()

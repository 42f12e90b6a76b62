"""Time of the AlexNet LPIPS loss (transeditor_amd.lpips_alex.AlexLPIPSLoss, csrc/lpips_alex_bwd.hip) on the MI355X, random weights of
the true geometry (widths 64 / 192 / 384 / 256 / 256).

    python tools/lpips_alex_loss_time.py [--batch 8] [--size 256] [--reps 9] [--out profiles/lpips_alex_loss/time.json]

Reports, for --batch image pairs in [-1, 1]:
  loss      : forward + backward of AlexLPIPSLoss, HIP events around whole calls (median of --reps after one untimed call); the forward
              alone beside it;
  eval      : AlexLPIPS.forward (the diversity score's class, no gradient) on the same 2 x --batch images, timed the same way;
  shares    : one more forward + backward with a pair of HIP events around every library call, summed per kind.  The events of a
              single call include its launch gap, so the parts add up to more than the whole call; the shares are of their own sum;
  kernels   : te_alex_stem_dgrad_f32 beside te_alex_stem_fwd_f32, te_pool3s2_max_bwd_f32 beside te_pool3_f32 at both planes, and
              conv2's data gradient (te_conv2d_dgrad_f32, 5 x 5, 192 -> 64 at the pooled plane), each alone on tensors that are
              already there, median of --reps.
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/lpips_alex_loss_time.py --once 20`, a run of its own.
GPU only.
"""
import argparse
import json
import sys

import torch

from net_timing import rate, shares, timed, write_json


def _dgrad_label(out, g, wt, x_shape, kernel, *a, **k):
    return f'conv dgrad {kernel[0]}x{kernel[1]} {g.shape[1]}->{x_shape[1]} @{x_shape[2]} (te_conv2d_dgrad_f32)'


def _conv_label(out, x, w, bias, stride, *a, **k):
    return f'conv {w.shape[2]}x{w.shape[3]} {w.shape[1]}->{w.shape[0]} @{out.shape[2]} (te_conv2d_f32)'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--once', type=int, default=0, help='run this many forward + backward pairs and nothing else (for a kernel trace)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lpips_alex_loss_time.py needs a GPU')
    import lpips_alex_loss_restated as LR
    import lpips_alex_restated as R
    from transeditor_amd import _lib
    from transeditor_amd.lpips_alex import AlexLPIPS, AlexLPIPSLoss
    B = a.batch
    sd = R.state_dict(2)
    loss = AlexLPIPSLoss(state_dict=sd, lin_state_dict=LR.lin_state_dict(3))
    ev = AlexLPIPS(state_dict=sd, lin_state_dict=R.lin_state_dict(3))
    x, y = R.images(B, B, a.size).to('cuda'), R.images(B + 1, B, a.size).to('cuda')
    res = {'command': ' '.join(['python tools/lpips_alex_loss_time.py'] + sys.argv[1:]), 'batch': B, 'size': a.size, 'widths': list(loss.widths)}

    def fwd_bwd():
        xin = x.clone().requires_grad_(True)
        loss(xin, y).backward()
        return xin.grad
    if a.once:                                                   # for a kernel trace: forward + backward pairs and nothing else
        for _ in range(a.once):
            fwd_bwd()
        torch.cuda.synchronize()
        return
    med, ts = timed(fwd_bwd, a.reps)
    res['loss_forward_backward'] = rate(med, ts, B)
    with torch.no_grad():
        medf, tsf = timed(lambda: loss(x, y), a.reps)
    res['loss_forward'] = rate(medf, tsf, B)
    mede, tse = timed(lambda: ev(x, y), a.reps)
    res['eval_forward'] = rate(mede, tse, B)
    res['loss_time_over_eval_time'] = round(med / mede, 3)
    wraps = [(_lib, 'alex_stem_fwd', 'stem (te_alex_stem_fwd_f32)'), (_lib, 'pool3', 'max pool (te_pool3_f32)'), (_lib, 'conv2d', _conv_label),
             (_lib, 'lpips_normalize', 'target normalisation (te_lpips_normalize_f32)'), (_lib, 'lpips_head_fwd', 'heads (te_lpips_head_fwd_f32)'),
             (_lib, 'lpips_dist', 'sum of the layers (te_lpips_dist_f32)'), (_lib, 'lpips_head_bwd', 'heads backward (te_lpips_head_bwd_f32)'),
             (_lib, 'conv2d_dgrad', _dgrad_label), (_lib, 'pool3s2_max_bwd', 'max pool backward (te_pool3s2_max_bwd_f32)'),
             (_lib, 'alex_stem_dgrad', 'stem gradient (te_alex_stem_dgrad_f32)')]
    sh = shares(fwd_bwd, wraps)
    total = sum(v[0] for v in sh.values())
    res['shares'] = {k: {'ms': round(ms, 4), 'calls': n, 'share': round(ms / total, 4)} for k, (ms, n) in sorted(sh.items(), key=lambda kv: -kv[1][0])}
    res['shares_sum_ms'] = round(total, 4)
    print(json.dumps({k: res[k] for k in ('loss_forward_backward', 'loss_forward', 'eval_forward', 'loss_time_over_eval_time', 'shares', 'shares_sum_ms')}),
          flush=True)
    # the new kernels alone, beside their forward counterparts and conv2's data gradient
    taps = loss._trunk(x)
    g0 = torch.randn_like(taps[0])
    p1 = _lib.pool3(taps[0], _lib.POOL3_MAX_S2)
    p2 = _lib.pool3(taps[1], _lib.POOL3_MAX_S2)
    gp1, gp2, g1 = torch.randn_like(p1), torch.randn_like(p2), torch.randn_like(taps[1])
    alone = {
        'te_alex_stem_dgrad_f32': lambda: _lib.alex_stem_dgrad(g0, loss.wt0, tuple(x.shape)),
        'te_alex_stem_fwd_f32': lambda: _lib.alex_stem_fwd(x, loss.w0, loss.b0),
        f'te_pool3s2_max_bwd_f32 @{taps[0].shape[2]}': lambda: _lib.pool3s2_max_bwd(gp1, taps[0]),
        f'te_pool3_f32 @{taps[0].shape[2]}': lambda: _lib.pool3(taps[0], _lib.POOL3_MAX_S2),
        f'te_pool3s2_max_bwd_f32 @{taps[1].shape[2]}': lambda: _lib.pool3s2_max_bwd(gp2, taps[1]),
        f'te_pool3_f32 @{taps[1].shape[2]}': lambda: _lib.pool3(taps[1], _lib.POOL3_MAX_S2),
        f'te_conv2d_dgrad_f32 conv2 5x5 {g1.shape[1]}->{p1.shape[1]} @{p1.shape[2]}': lambda: _lib.conv2d_dgrad(g1, loss.wt1, tuple(p1.shape), (5, 5), 1, (2, 2)),
    }
    res['kernels'] = {}
    for name, fn in alone.items():
        m, t = timed(fn, a.reps)
        res['kernels'][name] = {'ms_median': round(m, 4), 'ms_all': [round(v, 4) for v in t]}
    print(json.dumps({'kernels': res['kernels']}), flush=True)
    write_json(res, a.out)


if __name__ == '__main__':
    main()

"""Time of the identity loss (transeditor_amd.id_loss, ArcFaceID.embed_grad, csrc/irse_bwd.hip) on the MI355X, random weights of the true
geometry (IR-SE50: 24 units, 112 px plane, 512-d embedding), 256 px images.

    python tools/id_loss_time.py [--batches 1 8 16] [--size 256] [--reps 7] [--no-torch] [--out profiles/id_loss/net_time.json]
    python tools/id_loss_time.py --once 8        # one IDLoss forward + backward and nothing else: the run to put under a kernel trace

Reports, per batch size (HIP events, median of --reps after one untimed call):
  embed          : ArcFaceID.embed, the forward-only path (unchanged by the backward pass: the figure to hold the backward against);
  embed_grad fwd : the differentiable forward, which also stores the pre-activations;
  backward       : (e * c).sum().backward() through it, for a fixed cotangent c;
  id_loss        : IDLoss(y_hat, y, x) and loss.backward(): two embeds, one embed_grad, its backward, the dot products, the logs;
  shares         : one more backward with a pair of HIP events around every library call, summed per layer geometry.  The events of a
                   single call include its launch gap; the shares are of their own sum;
  stride 2       : each stride-2 3x3 layer of the network alone, te_conv2d_f32 forwards against te_conv2d_dgrad_f32 (four phases)
                   backwards on the same tensors;
  torch          : the SAME network (the same folded weights) written in plain torch ops under torch autograd on the same device, the
                   whole loss forward + backward.  Context, not a part of the product; the largest gradient difference is printed.
Nothing here is held to a speed bar.  GPU only.
"""
import argparse
import json
import sys

import torch
import torch.nn.functional as F

from net_timing import rate, shares, timed, write_json


def _dgrad_label(out, g, wt, x_shape, kernel, stride=1, pad=(0, 0), **k):
    epi = "prelu'" if k.get('pre') is not None else ('bn scale + add' if k.get('in_scale') is not None else 'plain')
    return f'dgrad {kernel[0]}x{kernel[1]} s{stride} {g.shape[1]}->{x_shape[1]} @{g.shape[2]}->{x_shape[2]} ({epi})'


def torch_loss(net):
    """the loss on the network in plain torch ops with the module's own (folded) weights, under torch autograd"""
    y0, y1, x0, x1 = net.box

    def embed(x):
        h = F.adaptive_avg_pool2d(x[:, :, y0:y1, x0:x1], (net.pool, net.pool))
        h = F.prelu(F.conv2d(h, net.stem_w, net.stem_b, 1, 1), net.stem_slope)
        for i, (_, _, stride) in enumerate(net.units):
            g = lambda k: getattr(net, f'u{i}_{k}', None)
            v = F.pad(h * g('scale').view(1, -1, 1, 1) + g('shift').view(1, -1, 1, 1), (1, 1, 1, 1))
            r = F.conv2d(F.prelu(F.conv2d(v, g('w1')), g('slope')), g('w2'), g('b2'), stride, 1)
            if net.se[i]:
                r = r * torch.sigmoid(F.relu(r.mean((2, 3)) @ g('fc1').t()) @ g('fc2').t())[:, :, None, None]
            sc = F.conv2d(h, g('sc_w'), g('sc_b'), stride, 0) if g('sc_w') is not None else h[:, :, ::stride, ::stride]
            h = r + sc
        e = F.linear(h.flatten(1), net.fc_w, net.fc_b)
        return e / e.norm(dim=1, keepdim=True)

    def run(y_hat, y, x):
        with torch.no_grad():
            ey, ex = embed(y), embed(x)
        eh = embed(y_hat)
        loss = (1 - (eh * ey).sum(1)).mean()
        logs = torch.stack([(eh * ey).sum(1).detach(), (eh.detach() * ex).sum(1), (ey * ex).sum(1)]).cpu()
        loss.backward()
        return loss, logs
    return run


def stride2_layers(net, batch, reps):
    """per stride-2 unit: its second convolution forwards and backwards (with the PReLU' epilogue), on random tensors of its shapes"""
    from transeditor_amd import _lib
    from transeditor_amd.irse_units import dgrad_weights
    out, side = [], net.pool
    for i, (cin, depth, stride) in enumerate(net.units):
        if stride == 2:
            g = lambda k: getattr(net, f'u{i}_{k}')
            t = torch.randn(batch, depth, side, side, device='cuda')
            gr = torch.randn(batch, depth, (side - 1) // 2 + 1, (side - 1) // 2 + 1, device='cuda')
            wt = dgrad_weights(net, i)['w2']
            fwd, fts = timed(lambda: _lib.conv2d(t, g('w2'), g('b2'), 2, (1, 1), act=0), reps)
            bwd, bts = timed(lambda: _lib.conv2d_dgrad(gr, wt, tuple(t.shape), (3, 3), 2, (1, 1), pre=t, slope=g('slope')), reps)
            out.append({'layer': f'3x3 s2 {depth}->{depth} @{side}->{gr.shape[2]}', 'forward_ms': round(fwd, 4), 'dgrad_phases_ms': round(bwd, 4),
                        'dgrad_over_forward': round(bwd / fwd, 3), 'forward_ms_all': [round(v, 4) for v in fts],
                        'dgrad_ms_all': [round(v, 4) for v in bts]})
        side = (side - 1) // stride + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 16])
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch autograd yardstick')
    ap.add_argument('--once', type=int, default=None, metavar='BATCH', help='one IDLoss forward + backward at this batch, nothing else')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('id_loss_time.py needs a GPU')
    import arcface_restated as R
    from transeditor_amd import _lib
    from transeditor_amd.id_loss import IDLoss
    mod = IDLoss(state_dict=R.state_dict(2))
    net = mod.facenet

    def images(batch):
        return [R.images(batch + s, batch, a.size).to('cuda') for s in (0, 1000, 2000)]

    def whole(y_hat, y, x):
        y_hat.grad = None
        loss, _, _ = mod(y_hat, y, x)
        loss.backward()
    if a.once is not None:
        y_hat, y, x = images(a.once)
        whole(y_hat.requires_grad_(True), y, x)                                   # (loads the code objects, builds the backward weights)
        torch.cuda.synchronize()
        whole(y_hat, y, x)
        torch.cuda.synchronize()
        return
    ref = None if a.no_torch else torch_loss(net)
    res = {'command': ' '.join(['python tools/id_loss_time.py'] + sys.argv[1:]), 'size': a.size, 'box': list(net.box), 'pool': net.pool,
           'units': len(net.units), 'dim': net.dim, 'runs': []}
    wraps = [(_lib, 'rows_unit_bwd', 'unit rows (te_rows_unit_bwd_f32)'), (_lib, 'fc_stream', 'output layer (te_fc_stream_f32, transposed)'),
             (_lib, 'se_bwd', 'gate (te_se_bwd_f32)'), (_lib, 'conv2d_dgrad', _dgrad_label), (_lib, 'id_stem_bwd', 'stem (te_id_stem_bwd_f32)')]
    for batch in a.batches:
        y_hat, y, x = images(batch)
        y_hat.requires_grad_(True)
        c = torch.randn(batch, net.dim, device='cuda')
        one = {'batch': batch}
        med, ts = timed(lambda: net.embed(y_hat), a.reps)
        one['embed'] = rate(med, ts, batch)
        med, ts = timed(lambda: net.embed_grad(y_hat), a.reps)
        one['embed_grad_forward'] = rate(med, ts, batch)
        # the backward alone: a fresh forward in front of every timed backward, outside the events
        bts = []
        for rep in range(a.reps + 1):
            y_hat.grad = None
            s = (net.embed_grad(y_hat) * c).sum()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            s.backward()
            t1.record()
            torch.cuda.synchronize()
            if rep:
                bts.append(t0.elapsed_time(t1))
        one['backward'] = rate(sorted(bts)[len(bts) // 2], bts, batch)
        one['backward_over_embed'] = round(one['backward']['ms_median'] / one['embed']['ms_median'], 3)
        med, ts = timed(lambda: whole(y_hat, y, x), a.reps)
        one['id_loss_forward_backward'] = rate(med, ts, batch)
        s = (net.embed_grad(y_hat) * c).sum()
        sh = shares(s.backward, wraps)
        total = sum(v[0] for v in sh.values())
        one['backward_shares'] = {k: {'ms': round(ms, 3), 'calls': n, 'share': round(ms / total, 4)} for k, (ms, n) in
                                  sorted(sh.items(), key=lambda kv: -kv[1][0])}
        one['backward_shares_sum_ms'] = round(total, 3)
        one['stride2'] = stride2_layers(net, batch, a.reps)
        if ref is not None:
            def torch_whole():
                y_hat.grad = None
                ref(y_hat, y, x)
            medt, tst = timed(torch_whole, a.reps)
            one['torch_autograd_id_loss'] = rate(medt, tst, batch)
            g_ref = y_hat.grad.clone()
            whole(y_hat, y, x)
            one['max_abs_gradient_difference_from_torch'] = float((y_hat.grad - g_ref).abs().max())
            one['max_abs_gradient'] = float(g_ref.abs().max())
            one['library_time_over_torch_time'] = round(one['id_loss_forward_backward']['ms_median'] / medt, 3)
        res['runs'].append(one)
        print(json.dumps(one), flush=True)
    write_json(res, a.out)


if __name__ == '__main__':
    main()

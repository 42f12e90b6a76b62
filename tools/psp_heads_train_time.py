"""Time and deviation of encoder head training (transeditor_amd.psp_heads_train, csrc/psp_heads_bwd.hip) on the MI355X at the true geometry:
the heads of GradualStyleEncoder(50, 'ir_se') (D = 512, styles (3, 4, 7), 16 spatials) on random weights, B = 8 at 256 px.

    python tools/psp_heads_train_time.py [--batch 8] [--reps 5] [--no-torch] [--no-step] [--fp64] [--out profiles/psp_heads_train/time.json]

One process; every step runs under its own time limit (SIGALRM) and the tool stops at the first step that fails or runs out of time, with
what it has measured so far already written.  HIP events, the median of --reps after one untimed call.  Steps:
  node      : the heads' forward, forward + backward, and the backward broken down by binding (one pair of events around every call);
              the weight gradient's achieved bandwidth against the bytes of gw it must write (its floor); two backward passes compared
              bit for bit, and the gradients' finiteness;
  torch     : the SAME stage under torch autograd on the same device, F.conv2d per head (the form the reference runs), forward + backward;
              a yardstick, not a part of the product;
  step      : a full heads_step through a 256 px generator (random weights) with the L2 and w-norm terms (no identity / LPIPS weight
              files are read: those terms have lambda 0), the L2 target being the generator's own rendering of the untrained codes, perturbed,
              at a rate of 1e-10 (random weights: the reference's 1e-4 overflows);
  fp64      : (--fp64) the pinned fp64 restatement of the stage under autograd on the CPU, with the same restatement in fp32 as the
              yardstick: rel_l2 of every gradient, summarised per kind.
Nothing here is held to a speed bar.  GPU only.
"""
import argparse
import contextlib
import json
import signal
import sys
import time

from net_timing import shares, timed, write_json

import torch
import torch.nn.functional as F


@contextlib.contextmanager
def limited(name, seconds):
    """the step `name` under its own time limit"""
    def stop(signum, frame):
        raise TimeoutError(f'step {name!r} ran past its limit of {seconds} s')
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(seconds)
    t0 = time.time()
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)
        print(f'[{name}: {time.time() - t0:.1f} s]', file=sys.stderr, flush=True)


def torch_stage(heads):
    """the head stage in plain differentiable torch ops on the device, head by head as the reference's loops run it, on parameters of its
    own (copies of the module's, in the module's layout) -> (run(c1, c2, c3) -> (z, p), the parameters)"""
    D, Ns, Np = heads.dim, heads.n_styles, heads.n_spatials
    Pm = {k: getattr(heads, k).detach().clone().requires_grad_(True) for k in heads.names}

    def run(c1, c2, c3):
        bufs = {'c3': c3}
        bufs['p2'] = F.interpolate(c3, size=c2.shape[2:], mode='bilinear', align_corners=True) + F.conv2d(c2, Pm['lat1_w'], Pm['lat1_b'])
        bufs['p1'] = F.interpolate(bufs['p2'], size=c1.shape[2:], mode='bilinear', align_corners=True) + F.conv2d(c1, Pm['lat2_w'], Pm['lat2_b'])
        parts = {}
        for i, src, dst, shared, c0, G in heads.program:
            w, b = Pm[f'h{i}_w'], Pm[f'h{i}_b']
            for n in range(G):
                xi = bufs[src] if shared else parts[src][n]
                parts.setdefault(dst, {})[c0 + n] = F.leaky_relu(F.conv2d(xi, w[n * D:(n + 1) * D], b[n * D:(n + 1) * D], 2, 1), 0.01)
        lat = torch.stack([F.linear(parts['r0'][n].flatten(1), Pm['lin_w'][n * D:(n + 1) * D] * heads.lin_scale, Pm['lin_b'][n * D:(n + 1) * D])
                           for n in range(Ns + Np)], 1)
        z = F.linear(lat[:, :Ns].permute(0, 2, 1), Pm['adjust_w'] * heads.adjust_scale, Pm['adjust_b'])
        return z, lat[:, Ns:].permute(0, 2, 1)
    return run, Pm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch yardstick')
    ap.add_argument('--no-step', action='store_true', help='skip the full heads_step through the generator')
    ap.add_argument('--fp64', action='store_true', help='also run the fp64 autograd reference of the stage on the CPU')
    ap.add_argument('--fp64-limit', type=int, default=420)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('psp_heads_train_time.py needs a GPU')
    import arcface_restated as R
    import psp_encoder_restated as P
    import psp_heads_bwd_restated as HB
    from transeditor_amd import _lib
    from transeditor_amd.psp_encoder import DualSpaceEncoder
    from transeditor_amd.psp_heads_train import TrainableHeads, heads_step, unpack
    res = {'command': ' '.join(['python tools/psp_heads_train_time.py'] + sys.argv[1:]), 'batch': a.batch, 'size': a.size}
    B = a.batch

    with limited('build', 300):
        sd = P.state_dict(2)
        enc = DualSpaceEncoder(state_dict=sd)
        heads = TrainableHeads(enc)
        x = R.images(B, B, a.size).to('cuda')
        with torch.no_grad():
            c = enc.backbone(x)
        gen = torch.Generator().manual_seed(11)
        gz, gp = (torch.randn(B, heads.dim, n, generator=gen).to('cuda') for n in (heads.tokens, heads.n_spatials))
        params = [getattr(heads, k) for k in heads.names]
        conv_weights = sum(getattr(heads, f'h{i}_w').numel() for i, *_ in heads.program)
        res.update(parameters=sum(p.numel() for p in params), head_conv_weights=conv_weights, launches=len(heads.program) + 1,
                   wgrad_splits={'latlayer1': _lib.conv2d_heads_wgrad_splits(512, c[1].shape[1], 1, 1, B, *c[1].shape[2:]),
                                 'latlayer2': _lib.conv2d_heads_wgrad_splits(512, c[0].shape[1], 1, 1, B, *c[0].shape[2:]),
                                 'heads 64 -> 32 px': _lib.conv2d_heads_wgrad_splits(512, 512, 3, 3, B, 32, 32),
                                 'heads 2 -> 1 px': _lib.conv2d_heads_wgrad_splits(512, 512, 3, 3, B, 1, 1)})
    write_json(res, a.out)

    def both(leaves=None):
        z, p = heads(*(leaves or c))
        return torch.autograd.grad([z, p], (leaves or []) + params, [gz, gp])

    with limited('node', 240):
        med_f, ts_f = timed(lambda: heads(*c), a.reps)
        med_b, ts_b = timed(both, a.reps)
        node = {'forward_ms': round(med_f, 3), 'forward_ms_all': [round(t, 3) for t in ts_f], 'forward_backward_ms': round(med_b, 3),
                'forward_backward_ms_all': [round(t, 3) for t in ts_b]}
        names = ('conv2d_heads', 'conv2d', 'upsample_add', 'psp_codes', 'conv2d_heads_wgrad', 'conv2d_heads_dgrad', 'conv2d_dgrad', 'upsample_add_bwd',
                 'psp_codes_bwd', 'heads_dgrad_weight', 'dgrad_weight')
        sh = shares(both, [(_lib, name, name) for name in names])
        node['by_binding'] = {k: {'ms': round(ms, 3), 'calls': n} for k, (ms, n) in sorted(sh.items(), key=lambda kv: -kv[1][0])}
        # the weight gradient of the head launches alone against the gw it writes
        log = shares(both, [(_lib, 'conv2d_heads_wgrad', lambda out, g, x, w_shape, *r, **k: 'heads' if w_shape[3] == 3 else 'laterals and linears')])
        ms = log['heads'][0]
        node['wgrad_heads'] = {'ms': round(ms, 3), 'gw_bytes': conv_weights * 4, 'achieved_GB_per_s': round(conv_weights * 4 / (ms * 1e-3) / 1e9, 1)}
        node['wgrad_laterals_and_linears_ms'] = round(log['laterals and linears'][0], 3)
        leaves = [t.clone().requires_grad_(True) for t in c]
        g1, g2 = both(leaves), both(leaves)
        node['two_backward_passes_bit_equal'] = all(torch.equal(u, v) for u, v in zip(g1, g2))
        node['gradients_finite'] = all(bool(torch.isfinite(u).all()) for u in g1)
        res['node'] = node
        print(json.dumps({'node': node}), flush=True)
    write_json(res, a.out)
    if not (node['two_backward_passes_bit_equal'] and node['gradients_finite']):
        raise SystemExit('the backward pass is not reproducible or not finite')

    if not a.no_torch:
        with limited('torch', 240):
            run, Pm = torch_stage(heads)
            plist = [Pm[k] for k in heads.names]

            def tboth():
                z, p = run(*c)
                return torch.autograd.grad([z, p], plist, [gz, gp])
            with torch.no_grad():
                med_tf, _ = timed(lambda: run(*c), a.reps)
            med_tb, ts_tb = timed(tboth, a.reps)
            gt = tboth()
            diff = max(float((u - v).norm() / v.norm()) for u, v in zip(g1[3:], gt))
            res['torch'] = {'forward_ms': round(med_tf, 3), 'forward_backward_ms': round(med_tb, 3), 'forward_backward_ms_all': [round(t, 3) for t in ts_tb],
                            'library_time_over_torch_time': round(med_b / med_tb, 3), 'largest_rel_l2_between_the_two_gradients': diff}
            print(json.dumps({'torch': res['torch']}), flush=True)
            del run, Pm, plist, gt
            torch.cuda.empty_cache()
        write_json(res, a.out)

    if not a.no_step:
        with limited('step', 300):
            from transeditor_amd import synth
            from transeditor_amd.encoder_loss import EncoderLoss
            from transeditor_amd.model_spatial_query import Generator
            from transeditor_amd.optim import encoder_optimizer
            from transeditor_amd.psp_heads_train import generator_decoder
            g = Generator(a.size, 512, 512, 2 * (a.size.bit_length() - 2), n_trans=8, pixel_norm_op_dim=1)       # the token count of a size-px generator
            gsd = g.state_dict()
            synth.fill_state_dict(gsd, 21)
            g.load_state_dict(gsd)
            decode = generator_decoder(g.to('cuda'), True)
            crit = EncoderLoss(id_lambda=0, lpips_lambda=0, l2_lambda=1.0, w_norm_lambda=0.005)
            # random weights on both sides make the loss surface steep: against the images themselves the loss starts near 1e5, and at the
            # reference's rate of 1e-4 the first, unrectified Ranger steps overflow within three iterations.  The target is what the
            # generator renders for the untrained codes, perturbed, and the rate is 1e-10: the work of a step depends on neither
            opt = encoder_optimizer(heads.parameters(), 'ranger', 1e-10)
            with torch.no_grad():
                z0, p0 = heads(*c)
                target = decode(z0 + enc.z_avg, p0 + enc.p_avg) if enc.z_avg is not None else decode(z0, p0)
                target = target + 0.01 * target.std() * torch.randn(target.shape, generator=torch.Generator().manual_seed(5)).to('cuda')
            near = lambda real, inversed, *rest: crit(target, inversed, *rest)
            losses = []
            med_s, ts_s = timed(lambda: losses.append(float(heads_step(enc, heads, decode, near, opt, x)[0])), a.reps)
            with torch.no_grad():
                med_bb, _ = timed(lambda: enc.backbone(x), a.reps)
            res['step'] = {'ms_median': round(med_s, 3), 'ms_all': [round(t, 3) for t in ts_s], 'losses': losses, 'backbone_forward_ms': round(med_bb, 3),
                           'terms': 'l2 1.0, w_norm 0.005; id and lpips have lambda 0 (no weight files); Ranger at lr 1e-10'}
            print(json.dumps({'step': res['step']}), flush=True)
        write_json(res, a.out)

    if a.fp64:
        with limited('fp64', a.fp64_limit):
            fresh = TrainableHeads(enc)                                          # the step above moved `heads`; the reference reads sd
            fp = [getattr(fresh, k) for k in fresh.names]
            leaves = [t.clone().requires_grad_(True) for t in c]
            z, p = fresh(*leaves)
            masks = HB.library_masks(z.grad_fn.kept[1], fresh.program, fresh.launch_heads, fresh.dim)
            got = torch.autograd.grad([z, p], leaves + fp, [gz, gp])
            named = unpack(dict(zip(fresh.names, got[3:])), fresh.launch_heads, fresh.dim, fresh.n_styles, fresh.n_spatials)
            named.update(zip(('c1', 'c2', 'c3'), got[:3]))
            c_cpu = [t.cpu() for t in c]
            t0 = time.time()
            r64 = HB.gradients(c_cpu, sd, gz.cpu(), gp.cpu(), torch.float64, masks=masks)['grads']
            t64 = time.time() - t0
            r32 = HB.gradients(c_cpu, sd, gz.cpu(), gp.cpu(), torch.float32, masks=masks)['grads']
            kinds = {}
            for key, want in r64.items():
                kind = ('convs.weight' if '.convs.' in key and key.endswith('weight') else 'convs.bias' if '.convs.' in key else 'linear' if '.linear.' in key
                        else 'latlayer' if key.startswith('lat') else 'adjust_style' if key.startswith('adjust') else 'c1 c2 c3')
                e = float((named[key].double().cpu() - want).norm() / want.norm())
                y = float((r32[key].double() - want).norm() / want.norm())
                if kind not in kinds or e * kinds[kind]['torch_fp32'] > kinds[kind]['library'] * y:
                    kinds[kind] = {'key': key, 'library': e, 'torch_fp32': y, 'ratio': round(e / y, 2)}
            res['fp64'] = {'seconds_fp64_autograd_on_the_cpu': round(t64, 1), 'worst_ratio_per_kind': kinds,
                           'keys': len(r64), 'mask_elements': sum(m.numel() for m in masks.values())}
            print(json.dumps({'fp64': res['fp64']}), flush=True)
        write_json(res, a.out)


if __name__ == '__main__':
    main()

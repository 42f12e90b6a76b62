"""Time of the dual-space pSp encoder (transeditor_amd.psp_encoder, csrc/psp_heads.hip) on the MI355X, random weights of the true geometry
(GradualStyleEncoder(50, 'ir_se'): 24 units, 14 styles and 16 spatials of width 512, 256 px images).

    python tools/psp_encoder_time.py [--batches 1 16] [--reps 7] [--no-torch] [--out profiles/psp_encoder/net_time.json]

HIP events, the median of --reps after one untimed call.  Reports, per batch size:
  stages     : stem, body, laterals + upsample-add, head chain, codes, each timed on its own with its inputs ready, and the whole encode;
  head chain : three ways in one process: as built (te_conv2d_heads_f32 with its split rule), with the split route off, and issued head
               by head through te_conv2d_f32 + te_bias_act_f32 (what the ABI allowed before the grouped kernel: 168 + 138 launches);
  rules      : the chain under other split rules: planes of at most `plane` pixels cut `ways` ways (K >= 2048);
  torch      : the SAME network (the same folded weights) in plain torch operators on the same device, and the largest difference
               between the codes.  A yardstick, not a part of the product.
Nothing here is held to a speed bar.  GPU only.
"""
import argparse
import json
import sys

from net_timing import rate, timed, write_json

import torch
import torch.nn.functional as F


def torch_network(enc):
    """the encoder in plain torch ops on the device, with the module's own (folded, packed) weights"""
    D, Ns, Np = enc.dim, enc.n_styles, enc.n_spatials

    @torch.no_grad()
    def run(x):
        h = F.prelu(F.conv2d(x, enc.stem_w, enc.stem_b, 1, 1), enc.stem_slope)
        c = []
        for i, (_, _, stride) in enumerate(enc.units):
            g = lambda k: getattr(enc, f'u{i}_{k}', None)
            v = F.pad(h * g('scale').view(1, -1, 1, 1) + g('shift').view(1, -1, 1, 1), (1, 1, 1, 1))
            r = F.conv2d(F.prelu(F.conv2d(v, g('w1')), g('slope')), g('w2'), g('b2'), stride, 1)
            if enc.se[i]:
                r = r * torch.sigmoid(F.relu(r.mean((2, 3)) @ g('fc1').t()) @ g('fc2').t())[:, :, None, None]
            sc = F.conv2d(h, g('sc_w'), g('sc_b'), stride, 0) if g('sc_w') is not None else h[:, :, ::stride, ::stride]
            h = r + sc
            if i in enc.taps:
                c.append(h)
        bufs = {'c3': c[2]}
        bufs['p2'] = F.interpolate(c[2], size=c[1].shape[2:], mode='bilinear', align_corners=True) + F.conv2d(c[1], enc.lat1_w, enc.lat1_b)
        bufs['p1'] = F.interpolate(bufs['p2'], size=c[0].shape[2:], mode='bilinear', align_corners=True) + F.conv2d(c[0], enc.lat2_w, enc.lat2_b)
        parts = {}
        for i, src, dst, shared, c0, G in enc.program:                              # head by head, as the reference's loops do
            w, b = getattr(enc, f'h{i}_w'), getattr(enc, f'h{i}_b')
            for n in range(G):                                                      # (an own-input launch reads ALL heads of its source, in order)
                xi = bufs[src] if shared else parts[src][n]
                parts.setdefault(dst, {})[c0 + n] = F.leaky_relu(F.conv2d(xi, w[n], b[n * D:(n + 1) * D], 2, 1), 0.01)
        lat = torch.stack([F.linear(parts['r0'][n].flatten(1), enc.lin_w[n, :, :, 0, 0], enc.lin_b[n * D:(n + 1) * D]) for n in range(Ns + Np)], 1)
        z = torch.einsum('tj,bjc->bct', enc.adjust_w, lat[:, :Ns]) + enc.adjust_b.view(1, 1, -1)
        return z, lat[:, Ns:].permute(0, 2, 1)
    return run


def head_by_head(enc, feats):
    """the chain as the ABI allowed before te_conv2d_heads_f32: per head and convolution te_conv2d_f32 and te_bias_act_f32 (leaky ReLU in
    place), the linear as te_conv2d_f32 1x1; the packed weights are read in place"""
    from transeditor_amd import _lib
    D, n = enc.dim, enc.n_styles + enc.n_spatials
    parts = {}
    for i, src, dst, shared, c0, G in enc.program:
        w, b = getattr(enc, f'h{i}_w'), getattr(enc, f'h{i}_b')
        for g in range(G):
            x = feats[src] if shared else parts[src][g]               # (an own-input launch reads ALL heads of its source, in order)
            y = _lib.conv2d(x, w[g], b[g * D:(g + 1) * D], 2, (1, 1), act=0)
            _lib._launch('te_bias_act_f32', _lib._ptr(y), _lib._ptr(y), None, None, 3, 0, 0.01, 1.0, y.numel(), 1, 1)
            parts.setdefault(dst, {})[c0 + g] = y
    return torch.stack([_lib.conv2d(parts['r0'][g], enc.lin_w[g], enc.lin_b[g * D:(g + 1) * D], 1, (0, 0), act=0).flatten(1) for g in range(n)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch yardstick')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('psp_encoder_time.py needs a GPU')
    import arcface_restated as R
    import psp_encoder_restated as P
    from transeditor_amd import _lib
    from transeditor_amd.irse_units import unit_forward
    from transeditor_amd.psp_encoder import DualSpaceEncoder
    enc = DualSpaceEncoder(state_dict=P.state_dict(2))
    ref_run = None if a.no_torch else torch_network(enc)
    K = 512 * 9
    res = {'command': ' '.join(['python tools/psp_encoder_time.py'] + sys.argv[1:]), 'size': a.size, 'units': len(enc.units), 'dim': enc.dim,
           'styles': enc.n_styles, 'spatials': enc.n_spatials, 'head_launches': len(enc.program) + 1,
           'split_rule': {f'{s}x{s}': _lib.conv2d_heads_splits(512, 3, 3, s, s) for s in (1, 2, 4, 8, 16)}, 'runs': []}
    for batch in a.batches:
        x = R.images(batch, batch, a.size).to('cuda')
        stem = lambda: _lib.conv2d_prelu(x, enc.stem_w, enc.stem_b, enc.stem_slope, None, None, 1, (1, 1))
        h0, c = stem(), []

        def body():
            h, c[:] = h0, []
            for i in range(len(enc.units)):
                h = unit_forward(enc, i, h)
                if i in enc.taps:
                    c.append(h)
        body()

        def pyramid():
            p2 = _lib.upsample_add(c[2], _lib.conv2d(c[1], enc.lat1_w, enc.lat1_b, 1, (0, 0), act=0))
            return {'c3': c[2], 'p2': p2, 'p1': _lib.upsample_add(p2, _lib.conv2d(c[0], enc.lat2_w, enc.lat2_b, 1, (0, 0), act=0))}
        feats = pyramid()
        lat = enc.heads(feats)
        codes = lambda: _lib.psp_codes(lat, enc.adjust_w, enc.adjust_b, enc.n_spatials, enc.z_avg, enc.p_avg)
        one = {'batch': batch, 'stages': {}}
        for name, fn in (('stem', stem), ('body', body), ('laterals + upsample-add', pyramid), ('head chain', lambda: enc.heads(feats)), ('codes', codes)):
            med, ts = timed(fn, a.reps)
            one['stages'][name] = {'ms_median': round(med, 3), 'ms_min': round(min(ts), 3), 'ms_max': round(max(ts), 3)}
        med, ts = timed(lambda: enc.encode(x), a.reps)
        one['library'] = rate(med, ts, batch)
        chain = {}
        for name, fn in (('as built', lambda: enc.heads(feats)), ('split route off', lambda: enc.heads(feats, splits=1)),
                         ('head by head (te_conv2d_f32 + te_bias_act_f32)', lambda: head_by_head(enc, feats))):
            med, ts = timed(fn, a.reps)
            chain[name] = {'ms_median': round(med, 3), 'ms_all': [round(t, 3) for t in ts]}
        one['head_chain'] = chain
        one['head_chain_max_abs_difference'] = {'split off': float((enc.heads(feats, splits=1) - lat).abs().max()),
                                                'head by head': float((head_by_head(enc, feats) - lat).abs().max()), 'scale': float(lat.abs().max())}
        rules = {}
        for plane in (1, 4, 16, 64, 256):
            for ways in (2, 4, 8, 16):
                rule = lambda Kk, HoWo, plane=plane, ways=ways: ways if HoWo <= plane and Kk >= 2048 else 1
                med, ts = timed(lambda: enc.heads(feats, splits=rule), a.reps)
                rules[f'plane <= {plane} px, {ways} ways'] = {'ms_median': round(med, 3), 'ms_min': round(min(ts), 3), 'ms_max': round(max(ts), 3)}
        one['rules'] = rules
        print(json.dumps(one), flush=True)
        if ref_run is not None:
            medt, tst = timed(lambda: ref_run(x), a.reps)
            one['torch'] = rate(medt, tst, batch)
            (z, p), (zt, pt) = enc.encode(x), ref_run(x)
            one['max_abs_code_difference_from_torch'] = {'z': float((z - zt).abs().max()), 'p': float((p - pt).abs().max()), 'scale': float(z.abs().max())}
            one['library_time_over_torch_time'] = round(one['library']['ms_median'] / medt, 3)
            print(json.dumps({k: one[k] for k in ('torch', 'max_abs_code_difference_from_torch', 'library_time_over_torch_time')}), flush=True)
        res['runs'].append(one)
        write_json(res, a.out)


if __name__ == '__main__':
    main()

"""Time of the LPIPS diversity score's scoring path (transeditor_amd.lpips_alex, csrc/lpips_alex.hip) on the MI355X for one group, random
weights of the true geometry (widths 64 / 192 / 384 / 256 / 256).

    python tools/lpips_alex_time.py [--group 40] [--size 256] [--reps 7] [--no-generator] [--no-baseline] [--out profiles/lpips_alex/time.json]

Reports, for a group of --group images in [-1, 1]:
  library   : AlexLPIPS.pairwise, HIP events around whole calls (median of --reps after one untimed call);
  shares    : one more call with a pair of HIP events around every library call, summed per kind: the network (stem, the two pools,
              conv2 ... conv5), the five normalisations, the five all-pairs launches, the final sum.  The events of a single call
              include its launch gap, so the parts add up to a little more than the whole call; the shares are of their own sum;
  heads     : the five all-pairs launches and the final sum alone, on taps that are already there (timed as a unit);
  generator : for proportion, the same number of images through GeneratorSampler (a 256 px generator with synthetic weights, the
              captured graph replayed), timed the same way;
  baseline  : the way of scoring the same group that existed before: every pair's two taps laid side by side as an interleaved batch
              of N (N - 1) / 2 pairs and te_lpips_pair_head_fwd_f32 + te_lpips_dist_f32 run over it.  That head has the VGG eps form,
              so this is a comparison of TIMES only; the gather that builds the interleaved batch is timed separately (4 GB for a
              group of 40 at 256 px: it fits in one batch).
Run under `rocprofv3 --kernel-trace --stats -- python tools/lpips_alex_time.py --no-generator --no-baseline` for per-kernel times.
GPU only.
"""
import argparse
import json
import sys

import torch

from net_timing import rate, shares, timed, write_json


def _conv_label(out, x, w, bias, stride, *a, **k):
    return f'conv {w.shape[2]}x{w.shape[3]} {w.shape[1]}->{w.shape[0]} @{out.shape[2]}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--group', type=int, default=40)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-generator', action='store_true')
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lpips_alex_time.py needs a GPU')
    import lpips_alex_restated as R
    from transeditor_amd import _lib
    from transeditor_amd.lpips_alex import AlexLPIPS
    N = a.group
    lp = AlexLPIPS(state_dict=R.state_dict(2), lin_state_dict=R.lin_state_dict(3))
    x = R.images(N, N, a.size).to('cuda')
    res = {'command': ' '.join(['python tools/lpips_alex_time.py'] + sys.argv[1:]), 'group': N, 'pairs': N * (N - 1) // 2, 'size': a.size,
           'widths': list(lp.widths)}
    med, ts = timed(lambda: lp.pairwise(x), a.reps)
    res['library'] = rate(med, ts, N)
    wraps = [(_lib, 'alex_stem_fwd', 'stem (te_alex_stem_fwd_f32)'), (_lib, 'pool3', 'max pool (te_pool3_f32)'), (_lib, 'conv2d', _conv_label),
             (_lib, 'lpips_unit', 'normalisation (te_lpips_unit_f32)'), (_lib, 'lpips_allpairs_fwd', 'all-pairs head (te_lpips_allpairs_fwd_f32)'),
             (_lib, 'lpips_allpairs_dist', 'sum of the layers (te_lpips_allpairs_dist_f32)')]
    sh = shares(lambda: lp.pairwise(x), wraps)
    total = sum(v[0] for v in sh.values())
    res['shares'] = {k: {'ms': round(ms, 4), 'calls': n, 'share': round(ms / total, 4)} for k, (ms, n) in sorted(sh.items(), key=lambda kv: -kv[1][0])}
    res['shares_sum_ms'] = round(total, 4)
    taps = lp._taps(x)
    hws = [t.shape[2] * t.shape[3] for t in taps]
    res['tap_planes'] = [list(t.shape[1:]) for t in taps]

    def heads():
        return _lib.lpips_allpairs_dist([_lib.lpips_allpairs_fwd(t, getattr(lp, f'lin{l}')) for l, t in enumerate(taps)],
                                        [(t.shape[1], hw) for t, hw in zip(taps, hws)], N)
    med, ts = timed(heads, a.reps)
    res['heads'] = {'ms_median': round(med, 4), 'ms_all': [round(t, 4) for t in ts]}
    print(json.dumps({k: res[k] for k in ('library', 'shares', 'shares_sum_ms', 'heads')}), flush=True)
    if not a.no_baseline:
        i, j = torch.triu_indices(N, N, 1, device='cuda')
        idx = torch.stack([i, j], 1).reshape(-1)                                # images 2n, 2n + 1 are pair n
        raw = lp._taps(x)                                                       # (normalised already: the pair head normalises again; times only)

        def gather():
            return [t.index_select(0, idx) for t in raw]
        med_g, ts_g = timed(gather, a.reps)
        inter = gather()

        def pair_heads():
            return _lib.lpips_dist([_lib.lpips_pair_head_fwd(f, getattr(lp, f'lin{l}')) for l, f in enumerate(inter)], hws)
        med_p, ts_p = timed(pair_heads, a.reps)
        res['baseline'] = {'pairs': len(i), 'interleaved_bytes': sum(f.numel() * 4 for f in inter),
                           'gather': {'ms_median': round(med_g, 4), 'ms_all': [round(t, 4) for t in ts_g]},
                           'pair_heads': {'ms_median': round(med_p, 4), 'ms_all': [round(t, 4) for t in ts_p]},
                           'heads_time_over_all_pairs_heads_time': round(med_p / res['heads']['ms_median'], 2)}
        del inter, raw
        print(json.dumps({'baseline': res['baseline']}), flush=True)
    if not a.no_generator:
        import math
        from transeditor_amd import synth
        from transeditor_amd.inference import GeneratorSampler
        from transeditor_amd.model_spatial_query import Generator
        G = Generator(a.size, 512, 512, 2 * (int(math.log2(a.size)) - 1), n_trans=8, pixel_norm_op_dim=1)
        sd = G.state_dict()
        synth.fill_state_dict(sd, 5)
        G.load_state_dict(sd)
        s = GeneratorSampler(G.to('cuda'))
        z, p = torch.randn(N, 512, 16, device='cuda'), torch.randn(N, 512, 16, device='cuda')
        med_gen, ts_gen = timed(lambda: s(z, p), a.reps)
        res['generator'] = rate(med_gen, ts_gen, N)
        res['scoring_time_over_generator_time'] = round(res['library']['ms_median'] / med_gen, 4)
        res['heads_time_over_generator_time'] = round(res['heads']['ms_median'] / med_gen, 4)
        print(json.dumps({k: res[k] for k in ('generator', 'scoring_time_over_generator_time', 'heads_time_over_generator_time')}), flush=True)
    write_json(res, a.out)


if __name__ == '__main__':
    main()

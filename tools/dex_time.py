"""Time of the DEX age / gender scorer (transeditor_amd.dex, csrc/dex.hip) on the MI355X, random weights of the true geometry (224 px
crop, 4096 / 4096, 101 classes).

    python tools/dex_time.py [--batches 16 64] [--size 256] [--reps 5] [--no-torch] [--out profiles/dex/net_time.json]

Reports, per batch size, for images in [-1, 1]:
  library : DEXScorer.forward, images/s from HIP events around whole forward passes (median of --reps after one untimed call);
  shares  : one more pass with a pair of HIP events around every library call, summed per kernel family (the fused stem, the trunk
            convolutions, their ReLU passes, the max-pools, the two fc layers, the softmax / score head).  The events of a single call
            include its launch gap, so the families add up to a little more than the whole pass; the shares are of their own sum;
  torch   : the SAME network (the same weights) written in plain torch ops on the same device: indexing, clamp / add / div / mul / round,
            slicing, F.conv2d, F.max_pool2d, F.linear, F.softmax.  A yardstick, not a part of the product; the largest relative
            difference between the two score vectors is printed.
Run under `rocprofv3 --kernel-trace --stats -- python tools/dex_time.py --batches 64 --no-torch` for per-kernel times
(tools/rocpd_stats.py summarises the trace).  GPU only.
"""
import torch
import torch.nn.functional as F

from net_timing import scorer_main

FAMILIES = {'dex_stem_fwd': 'stem (te_dex_stem_fwd_f32)', 'conv': 'trunk convolutions', 'maxpool2_fwd': 'max-pools',
            'fc_stream': 'fc1 + fc2 (te_fc_stream_f32)', 'cls_score': 'head (te_cls_score_f32)'}


def torch_network(scorer):
    """the scorer in plain torch ops on the device, with the scorer's own weights"""
    crop, mode = scorer.crop, scorer.mode
    pool_before = (2, 4, 7, 10)

    @torch.no_grad()
    def run(x):
        o = (x.shape[2] - crop) // 2
        h = x[:, [2, 1, 0]].clamp(-1, 1).add(1).div(2).mul(255).round()[:, :, o:o + crop, o:o + crop]
        for i in range(13):
            if i in pool_before:
                h = F.max_pool2d(h, 2, 2)
            h = F.relu(F.conv2d(h, getattr(scorer, f'w{i}'), getattr(scorer, f'b{i}'), padding=1))
        h = F.max_pool2d(h, 2, 2).flatten(1)
        h = F.relu(F.linear(h, scorer.fc1_w, scorer.fc1_b))
        h = F.relu(F.linear(h, scorer.fc2_w, scorer.fc2_b))
        p = F.softmax(F.linear(h, scorer.cls_w, scorer.cls_b), 1)
        if mode == 0:
            return (p * torch.arange(1, p.shape[1] + 1, device=p.device, dtype=p.dtype)).sum(1)
        return p[:, 0]
    return run


def main():
    import dex_restated as R
    from transeditor_amd import _lib, frozen_net
    from transeditor_amd.dex import DEXScorer

    def build():
        scorer = DEXScorer(state_dict=R.state_dict(2), attribute='age')
        return scorer, {'crop': scorer.crop}
    scorer_main('dex_time.py', 5, build,
                lambda batch, size: 0.6 * torch.randn(batch, 3, size, size, device='cuda',
                                                      generator=torch.Generator(device='cuda').manual_seed(batch)),
                [(_lib, n, family) for n, family in FAMILIES.items()] + [(frozen_net, '_relu_', 'trunk ReLU passes')], torch_network,
                lambda lib, ref: {'max_relative_score_difference_from_torch': float(((lib - ref).abs() / ref.abs()).max())})


if __name__ == '__main__':
    main()

"""Time of the CelebA-HQ attribute scorer (transeditor_amd.celeba_attr, csrc/celeba_attr.hip) on the MI355X, random weights of the true
geometry (R = 256, 64 ... 512 channels, 13 3x3 convolutions).

    python tools/celeba_attr_time.py [--batches 16 64] [--size 256] [--reps 7] [--no-torch] [--out profiles/celeba_attr/net_time.json]

Reports, per batch size, for images in [-1, 1]:
  library : CelebAAttributeScorer.forward, images/s from HIP events around whole forward passes (median of --reps after one untimed call);
  shares  : one more pass with a pair of HIP events around every library call, summed per kernel family (the fused stem, the
            convolutions by route, the pool passes, dense0, the score head).  The events of a single call include its launch gap, so the
            families add up to a little more than the whole pass; the shares are of their own sum;
  torch   : the SAME network (the same scaled weights) written in plain torch ops on the same device: indexing, clamp / add / div / mul /
            round, the view + mean box filter, F.conv2d, F.leaky_relu, F.avg_pool2d, F.linear, F.softmax.  A yardstick, not a part of
            the product; the largest absolute difference between the two score vectors is printed.
Run under `rocprofv3 --kernel-trace --stats -- python tools/celeba_attr_time.py --batches 64 --no-torch --reps 3` for per-kernel times
(tools/rocpd_stats.py summarises the trace).  GPU only.
"""
import torch
import torch.nn.functional as F

from net_timing import scorer_main

FAMILIES = {'attr_stem_fwd': 'stem (te_attr_stem_fwd_f32)', 'avgpool2_act': 'pool passes (te_avgpool2_act_f32)',
            'fc_stream': 'dense0 (te_fc_stream_f32)', 'attr_score': 'head (te_attr_score_f32)'}


def torch_network(scorer):
    """the scorer in plain torch ops on the device, with the scorer's own (scaled) weights"""
    R, n = scorer.resolution, scorer.n_convs

    @torch.no_grad()
    def run(x):
        h = x[:, [2, 1, 0]].clamp(-1, 1).add(1).div(2).mul(255).round()
        f = h.shape[2] // R
        if f > 1:
            h = h.view(h.shape[0], 3, R, f, R, f).mean(dim=[3, 5])
        h = F.leaky_relu(F.conv2d(h, scorer.stem_w.view(-1, 3, 1, 1), scorer.stem_b), 0.2)
        for i in range(0, n - 1, 2):
            h = F.leaky_relu(F.conv2d(h, getattr(scorer, f'w{i}'), getattr(scorer, f'b{i}'), padding=1), 0.2)
            h = F.leaky_relu(F.avg_pool2d(F.conv2d(h, getattr(scorer, f'w{i + 1}'), getattr(scorer, f'b{i + 1}'), padding=1), 2, 2), 0.2)
        h = F.leaky_relu(F.conv2d(h, getattr(scorer, f'w{n - 1}'), getattr(scorer, f'b{n - 1}'), padding=1), 0.2).flatten(1)
        h = F.leaky_relu(F.linear(h, scorer.dense0_w, scorer.dense0_b), 0.2)
        l = F.linear(h, scorer.dense1_w.view(1, -1), scorer.dense1_b)
        return F.softmax(torch.cat([l, -l], 1), 1)[:, 1]
    return run


def main():
    import celeba_attr_restated as R
    from transeditor_amd import _lib
    from transeditor_amd.celeba_attr import CelebAAttributeScorer
    routes = {_lib.CONV_3X3: 'convolutions, TE_CONV_3X3', _lib.CONV_3X3W: 'convolutions, TE_CONV_3X3W', _lib.CONV_3X3W6: 'convolutions, TE_CONV_3X3W6'}

    def build():
        scorer = CelebAAttributeScorer(state_dict=R.state_dict(2, 256))
        return scorer, {'resolution': scorer.resolution, 'channels': list(scorer.channels)}
    scorer_main('celeba_attr_time.py', 7, build, lambda batch, size: R.images(batch, batch, size).to('cuda'),
                [(_lib, n, family) for n, family in FAMILIES.items()] + [(_lib, 'conv', lambda out, x, wp, kind, *a, **k: routes[kind])],
                torch_network,
                lambda lib, ref: {'score_range': [float(lib.min()), float(lib.max())],
                                  'max_absolute_score_difference_from_torch': float((lib - ref).abs().max())},
                per_batch=lambda scorer, batch: {'routes': [[H, kind] for H, kind in scorer.conv_routes(batch)]})


if __name__ == '__main__':
    main()

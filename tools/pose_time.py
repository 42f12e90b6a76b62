"""Time of the pose scorer (transeditor_amd.pose, csrc/resnet.hip) on the MI355X, random weights of the true geometry (224 px crop,
widths 64 ... 512, 2 classes).

    python tools/pose_time.py [--batches 16 64] [--size 256] [--reps 5] [--no-torch] [--out profiles/pose/net_time.json]

Reports, per batch size, for images in [-1, 1]:
  library : PoseScorer.forward, images/s from HIP events around whole forward passes (median of --reps after one untimed call);
  shares  : one more pass with a pair of HIP events around every library call, summed per layer geometry (the fused stem, the max
            pool, every convolution shape of the eight blocks with and without the residual, the global average, the head).  The
            events of a single call include its launch gap, so the layers add up to a little more than the whole pass; the shares
            are of their own sum;
  torch   : the SAME network (the same folded weights) written in plain torch ops on the same device: indexing, clamp / add / div /
            mul / round, slicing, F.conv2d, F.max_pool2d, mean, F.linear, F.softmax.  A yardstick, not a part of the product; the
            largest relative difference between the two score vectors is printed.
Run under `rocprofv3 --kernel-trace --stats -- python tools/pose_time.py --batches 16 --no-torch` for per-kernel times
(tools/rocpd_stats.py summarises the trace).  GPU only.
"""
import torch
import torch.nn.functional as F

from net_timing import scorer_main


def _conv_label(out, x, w, bias, stride, *a, **k):
    return f'conv {w.shape[2]}x{w.shape[3]} s{stride} {w.shape[1]}->{w.shape[0]} @{out.shape[2]}'


def _res_label(out, x, w, bias, res, stride, *a, **k):
    return _conv_label(out, x, w, bias, stride) + ' + residual'


def torch_network(scorer):
    """the scorer in plain torch ops on the device, with the scorer's own (folded) weights"""
    from transeditor_amd.pose import LAYERS
    crop = scorer.crop

    def conv(key, h):
        i, stride, pad = scorer._spec[key]
        return F.conv2d(h, getattr(scorer, f'w{i}'), getattr(scorer, f'b{i}'), stride=stride, padding=pad)

    @torch.no_grad()
    def run(x):
        o = (x.shape[2] - crop) // 2
        h = x[:, [2, 1, 0]].clamp(-1, 1).add(1).div(2).mul(255).round()[:, :, o:o + crop, o:o + crop]
        h = F.max_pool2d(F.relu(conv('backbone.0', h)), 3, 2, 1)
        for at, layer in enumerate(LAYERS):
            for blk in (0, 1):
                n = f'backbone.{layer}.{blk}'
                t = F.relu(conv(f'{n}.conv1', h))
                if at > 0 and blk == 0:
                    h = conv(f'{n}.downsample.0', h)
                h = F.relu(conv(f'{n}.conv2', t) + h)
        return F.softmax(F.linear(h.mean((2, 3)), scorer.extra_w, scorer.extra_b), 1)[:, 0]
    return run


def main():
    import pose_restated as R
    from transeditor_amd import _lib
    from transeditor_amd.pose import PoseScorer

    def build():
        scorer = PoseScorer(state_dict=R.state_dict(2))
        return scorer, {'crop': scorer.crop, 'widths': list(scorer.widths)}
    scorer_main('pose_time.py', 5, build,
                lambda batch, size: 0.6 * torch.randn(batch, 3, size, size, device='cuda',
                                                      generator=torch.Generator(device='cuda').manual_seed(batch)),
                [(_lib, 'pose_stem_fwd', 'stem (te_pose_stem_fwd_f32)'), (_lib, 'maxpool3s2p1', 'max pool (te_maxpool3s2p1_f32)'),
                 (_lib, 'conv2d', _conv_label), (_lib, 'conv2d_res', _res_label), (_lib, 'adaptive_avgpool', 'global average'),
                 (_lib, 'cls_score', 'head (te_cls_score_f32)')], torch_network,
                lambda lib, ref: {'max_relative_score_difference_from_torch': float(((lib - ref).abs() / ref.abs()).max())})


if __name__ == '__main__':
    main()

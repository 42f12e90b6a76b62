"""Time of the ArcFace identity network (transeditor_amd.arcface, csrc/irse.hip) on the MI355X, random weights of the true geometry
(IR-SE50: 24 units, 112 px plane, 512-d embedding).

    python tools/arcface_time.py [--batches 16 64] [--size 256] [--reps 5] [--no-torch] [--out profiles/arcface/net_time.json]

Reports, per batch size, for images in [-1, 1]:
  library : ArcFaceID.embed, images/s from HIP events around whole forward passes (median of --reps after one untimed call);
  shares  : one more pass with a pair of HIP events around every library call, summed per layer geometry.  The events of a single
            call include its launch gap, so the layers add up to a little more than the whole pass; the shares are of their own sum;
  torch   : the SAME network (the same folded weights, the leading batch norms as scale and shift) written in plain torch ops on the
            same device.  A yardstick, not a part of the product; the largest difference between the two embeddings is printed.
Nothing here is held to a speed bar.  GPU only.
"""
import torch
import torch.nn.functional as F

from net_timing import scorer_main


def _conv_label(out, x, w, *a, **k):
    stride = a[1] if len(a) > 1 else k.get('stride', 1)
    return f'conv {w.shape[2]}x{w.shape[3]} s{stride} {w.shape[1]}->{w.shape[0]} @{out.shape[2]}'


def _prelu_label(out, x, w, *a, **k):
    return f'bn + conv 3x3 + prelu {w.shape[1]}->{w.shape[0]} @{out.shape[2]}'


def torch_network(net):
    """the network in plain torch ops on the device, with the module's own (folded) weights"""
    y0, y1, x0, x1 = net.box

    @torch.no_grad()
    def run(x):
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
    return run


def main():
    import arcface_restated as R
    from transeditor_amd import _lib
    from transeditor_amd.arcface import ArcFaceID

    def build():
        net = ArcFaceID(state_dict=R.state_dict(2))
        return net, {'box': list(net.box), 'pool': net.pool, 'units': len(net.units), 'dim': net.dim}
    scorer_main('arcface_time.py', 5, build, lambda batch, size: R.images(batch, batch, size).to('cuda'),
                [(_lib, 'id_stem_fwd', 'stem (te_id_stem_fwd_f32)'), (_lib, 'conv2d_prelu', _prelu_label), (_lib, 'conv2d', _conv_label),
                 (_lib, 'adaptive_avgpool', 'squeeze (te_adaptive_avgpool_f32)'), (_lib, 'se_excite', 'excite (te_se_excite_f32)'),
                 (_lib, 'se_scale_add', 'res * gate + shortcut (te_se_scale_add_f32)'), (_lib, 'fc_stream', 'output layer (te_fc_stream_f32)'),
                 (_lib, 'rows_unit', 'unit rows (te_rows_unit_f32)')], torch_network,
                lambda lib, ref: {'max_abs_embedding_difference_from_torch': float((lib - ref).abs().max())})


if __name__ == '__main__':
    main()

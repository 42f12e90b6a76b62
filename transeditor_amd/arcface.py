"""The ArcFace identity network of edit evaluation on the gfx950 kernels (the reference's pSp/models/encoders/model_irse.py:10-49 Backbone
with helpers.py:16-120, as pSp/criteria/id_loss.py:8-21 applies it: Backbone(112, 50, mode='ir_se') behind the crop [35:223, 32:220] and
AdaptiveAvgPool2d((112, 112))): is an edited image still the same person?

    net = ArcFaceID('model_ir_se50.pth')                            # the reference's own weight file
    e = net(images)                                                 # [B,3,S,S] in [-1, 1] -> [B,512] unit rows on the device
    s = net.similarity(net(a), net(b))                              # [B]: the paired dot products (calc_id_loss_parallel.py:67)
    f = edit_eval.feature_sweeps(net, origin, sweeps, batch=16)     # an instance is an `embed` of transeditor_amd.edit_eval

    python -m transeditor_amd.arcface --weights model_ir_se50.pth --a A.pt --b B.pt [--batch 16]

Weights come from a local file with the reference Backbone's keys (input_layer.{0,1,2}, body.N.res_layer.{0,1,2,3,4},
body.N.res_layer.5.fc{1,2}, body.N.shortcut_layer.{0,1}, output_layer.{0,3,4}; num_batches_tracked is ignored); nothing is downloaded.
The geometry is read from the shapes: the units are body.0, body.1, ... as long as the keys go on, a unit's (in, depth) are its first
convolution's, it has a squeeze-and-excitation where it has res_layer.5 (mode 'ir' has none) and a convolution shortcut where it has
shortcut_layer.0.  A stride is not stored in a state dict; the reference's rule is taken (helpers.py:26-27 get_block: the first unit of
a stage has stride 2, and a stage starts at body.0 and wherever in != depth), which gives get_blocks(50) for the real file; `units`
names another list of (in, depth, stride), which must be the one the keys describe.  An output_layer.4 without weight and bias is taken
as affine-less (IR_SE_50() builds it so, IDLoss with affine=True).

Layers: te_id_stem_fwd_f32 (the crop, the adaptive average and input_layer in one pass), then per unit te_conv2d_prelu_f32 (the
leading BatchNorm2d as an affine GATHER in front of the zero-padded convolution: its shift cannot be a bias, the padded taps do not
carry it; then PReLU), te_conv2d_f32 (the second convolution, stride 1 or 2, its batch norm folded in), te_adaptive_avgpool_f32 to 1 x 1
and te_se_excite_f32 (the gates), the shortcut (the unit's input read with the stride, or te_conv2d_f32 1x1 with its batch norm folded)
and te_se_scale_add_f32 (res * gate + shortcut).  output_layer is folded exactly on the host in fp64 (BatchNorm2d into the columns of
the Linear - there is no padding there -, BatchNorm1d into its rows and bias; Dropout is the identity in eval mode) and runs as
te_fc_stream_f32; te_rows_unit_f32 normalises.  Every convolution is the exact-fp32 implicit GEMM of csrc/conv2d_body.h.  An image's
embedding is bitwise the same whatever batch it is in.  The unit parse and the unit forward live in irse_units.py, which the inversion
encoder (psp_encoder.py) runs too.  Measured deviations and times: profiles/README.md, 'Identity embedding'.

    e = net.embed_grad(images)                                      # the same bits, and a gradient for `images`

The network is frozen (eval-mode batch norms, no weight gradient), but it has a backward pass with respect to its input: embed_grad is
the same chain as one once-differentiable autograd.Function (_Embed, written as lpips._Distance is) on the kernels of csrc/irse_bwd.hip:
te_rows_unit_bwd_f32, te_fc_stream_f32 on the transposed folded weight, irse_units.unit_backward per unit (te_se_bwd_f32 and
te_conv2d_dgrad_f32, a stride-2 layer in its four output phases) and te_id_stem_bwd_f32.  The forward keeps per unit the first
convolution's pre-activation and, for the gate, the residual branch, the gates and the pooled vector; nothing else.  id_loss.IDLoss
is the reference's training loss on it.  Times: profiles/README.md, 'Identity loss'.
"""
import argparse
import json
import sys

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .frozen_net import check_images, no_gpu, resolve, weight_bias
from .irse_units import (BN_EPS, bn_affine, check_unit_list, parse_stem, parse_units, reader, register_units, unit_backward, unit_forward,
                         unit_forward_keep)

BOX = (35, 223, 32, 220)                                              # id_loss.py:18: rows 35:223, columns 32:220
POOL = 112                                                            # id_loss.py:14
_NO_GPU = no_gpu('ArcFaceID')
_HINT = 'not a Backbone state dict: input_layer.*, body.N.res_layer.*, output_layer.*'


def default_units():
    """helpers.py:30-37 get_blocks(50): [(in, depth, stride)] * 24"""
    out = []
    for cin, depth, n in ((64, 64, 3), (64, 128, 4), (128, 256, 14), (256, 512, 3)):
        out += [(cin, depth, 2)] + [(depth, depth, 1)] * (n - 1)
    return out


def _out_side(h, units):
    for _, _, s in units:
        h = (h - 1) // s + 1
    return h


def parse_state_dict(sd, path='state_dict', units=None, pool=POOL, dtype=torch.float32):
    """-> dict(stem (w', b', slope), units [dict(cin, depth, stride, scale, shift, w1, slope, w2, b2, fc1, fc2, sc)], fc (w'', b''), keys):
    the batch norms folded as the module docstring says, `keys` the set of keys that were read; ValueError naming the key that is missing,
    has the wrong shape or does not fit the unit list.  dtype=torch.float64: the folded values before their one rounding"""
    get, read = reader(sd, 'ArcFaceID', path, _HINT)

    def affine(key, c):
        return bn_affine(get, key, c)
    stem = parse_stem(get, dtype)
    parsed = parse_units(sd, get, stem[0].shape[0], check_unit_list(units, 'ArcFaceID'), 'ArcFaceID', path, _HINT, dtype)
    ci = parsed[-1]['depth']
    # output_layer: BatchNorm2d(ci) -> Flatten -> Linear(ci * h * h, D) -> BatchNorm1d(D), folded in fp64 and rounded once
    h = _out_side(pool, [(u['cin'], u['depth'], u['stride']) for u in parsed])
    read.add('output_layer.3.bias')
    wl, bl = weight_bias(sd, 'output_layer.3.weight', 'output_layer.3.bias', (None, ci * h * h), 'ArcFaceID', path, _HINT,
                         want=f'[D, {ci} * {h} * {h}]: {len(parsed)} units take a {pool} px plane to {h} px')
    read.add('output_layer.3.weight')
    D = wl.shape[0]
    if (ci * h * h) % 4:
        raise ValueError(f'ArcFaceID: output_layer.3.weight is {tuple(wl.shape)}: the flattened features must be a multiple of 4')
    s2, t2 = affine('output_layer.0', ci)
    wl, bl = wl.double(), bl.double()
    bl = bl + wl @ t2.repeat_interleave(h * h)
    wl = wl * s2.repeat_interleave(h * h).view(1, -1)
    has = [f'output_layer.4.{t}' in sd for t in ('weight', 'bias')]
    if has[0] != has[1]:
        raise ValueError(f'ArcFaceID: {path} has only one of output_layer.4.weight / output_layer.4.bias')
    mean, var = (get(f'output_layer.4.{t}', (D,)).detach().double().cpu() for t in ('running_mean', 'running_var'))
    g1 = 1.0 / torch.sqrt(var + BN_EPS)
    b1 = torch.zeros(D, dtype=torch.float64)
    if has[0]:
        g1 = g1 * get('output_layer.4.weight', (D,)).detach().double().cpu()
        b1 = get('output_layer.4.bias', (D,)).detach().double().cpu()
    fc = ((wl * g1.view(-1, 1)).to(dtype).contiguous(), ((bl - mean) * g1 + b1).to(dtype).contiguous())
    return dict(stem=stem, units=parsed, fc=fc, keys=read, affine=has[0], side=h)


class _Embed(Function):
    """e = ArcFaceID.embed(images), bit for bit; backward -> the gradient w.r.t. images (the network is frozen)"""

    @staticmethod
    def forward(ctx, images, net):
        a, stem_pre = _lib.id_stem_keep(images, net.stem_w, net.stem_b, net.stem_slope, net.box, net.pool)
        kept = []
        for i in range(len(net.units)):
            a, k = unit_forward_keep(net, i, a)
            kept.append(k)
        f = _lib.fc_stream(a.view(a.shape[0], -1), net.fc_w, net.fc_b, act=0)
        e = _lib.rows_unit(f)
        ctx.net, ctx.kept, ctx.stem_pre, ctx.rows, ctx.shapes = net, kept, stem_pre, (e, f), (tuple(images.shape), tuple(a.shape))
        return e

    @staticmethod
    @once_differentiable
    def backward(ctx, ge):
        net, kept = ctx.net, ctx.kept
        image_shape, feature_shape = ctx.shapes
        stem_wt, fc_wt, fc_zero = net._backward_weights()
        g = _lib.rows_unit_bwd(ge.contiguous(), *ctx.rows)
        g = _lib.fc_stream(g, fc_wt, fc_zero, act=0).view(feature_shape)          # the Linear backwards: the transposed folded weight
        for i in range(len(net.units) - 1, -1, -1):
            g = unit_backward(net, i, kept[i], g)
            kept[i] = None
        gimg = _lib.id_stem_bwd(g, stem_wt, ctx.stem_pre, net.stem_slope, image_shape, net.box, net.pool)
        ctx.kept = ctx.stem_pre = ctx.rows = None
        return gimg, None


class ArcFaceID(torch.nn.Module):
    def __init__(self, path=None, state_dict=None, box=BOX, pool=POOL, units=None):
        super().__init__()
        if not isinstance(pool, int) or not 1 <= pool <= 32768:
            raise ValueError(f'ArcFaceID: pool must be an integer in [1, 32768], got {pool!r}')
        box = tuple(box)
        if len(box) != 4 or not all(isinstance(v, int) for v in box) or not (0 <= box[0] < box[1] and 0 <= box[2] < box[3]):
            raise ValueError(f'ArcFaceID: box must be (y0, y1, x0, x1) with 0 <= y0 < y1 and 0 <= x0 < x1, got {box!r}')
        state_dict, path = resolve(path, state_dict, 'ArcFaceID', 'ArcFace IR-SE weight')
        net = parse_state_dict(state_dict, path, units, pool)
        self.box, self.pool, self.keys, self.affine = box, pool, frozenset(net['keys']), net['affine']
        self.dim = net['fc'][0].shape[0]
        for name, t in zip(('stem_w', 'stem_b', 'stem_slope', 'fc_w', 'fc_b'), (*net['stem'], *net['fc'])):
            self.register_buffer(name, t)
        register_units(self, net['units'])
        self.eval()
        if torch.cuda.is_available():
            self.to('cuda')

    def _unit(self, i, x):
        return unit_forward(self, i, x)

    @torch.no_grad()
    def embed(self, images):
        """[B,3,S,S] in [-1, 1] -> [B,D] fp32 unit rows on the device"""
        check_images(images, 'ArcFaceID', '[B,3,S,S]', square=True)
        S = images.shape[2]
        if self.box[1] > S or self.box[3] > S:
            raise ValueError(f'ArcFaceID: the box {self.box} does not lie inside a {S} px image')
        if not images.is_cuda:
            raise RuntimeError(_NO_GPU)
        a = _lib.id_stem_fwd(images.detach().float(), self.stem_w, self.stem_b, self.stem_slope, self.box, self.pool)
        for i in range(len(self.units)):
            a = self._unit(i, a)
        return _lib.rows_unit(_lib.fc_stream(a.view(a.shape[0], -1), self.fc_w, self.fc_b, act=0))

    forward = embed

    def _backward_weights(self):
        """(made once per device: the weights never change) the stem weight in _lib.conv2d_dgrad's layout, the transposed folded Linear
        [C * h * h, D] and its zero bias"""
        cache = self.__dict__.setdefault('_bwd_weights', {})
        if self.fc_w.device not in cache:
            cache[self.fc_w.device] = (_lib.dgrad_weight(self.stem_w, 1, (1, 1)), self.fc_w.t().contiguous(),
                                       torch.zeros(self.fc_w.shape[1], device=self.fc_w.device))
        return cache[self.fc_w.device]

    def embed_grad(self, images):
        """embed with a backward pass: [B,3,S,S] in [-1, 1] -> [B,D] fp32 unit rows, bitwise embed's, differentiable w.r.t. images (once)"""
        check_images(images, 'ArcFaceID', '[B,3,S,S]', square=True)
        S = images.shape[2]
        if self.box[1] > S or self.box[3] > S:
            raise ValueError(f'ArcFaceID: the box {self.box} does not lie inside a {S} px image')
        if not images.is_cuda:
            raise RuntimeError(_NO_GPU)
        return _Embed.apply(images.float(), self)

    @torch.no_grad()
    def similarity(self, a, b):
        """the paired dot products of two sets of embeddings [B,D] -> [B] (id_loss.py:34-36, calc_id_loss_parallel.py:67)"""
        if a.ndim != 2 or tuple(a.shape) != tuple(b.shape):
            raise ValueError(f'ArcFaceID: similarity expects two [B,D] tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}')
        if not (a.is_cuda and b.is_cuda):
            raise RuntimeError(_NO_GPU)
        return _lib.rows_dot(a.detach().float().contiguous(), b.detach().float().contiguous())


# ------------------------------------------------------------------------------------------------------------------------ CLI
def build_parser():
    parser = argparse.ArgumentParser(description='identity similarity of two sets of images with the ArcFace IR-SE50 network '
                                                 '(pSp/criteria/id_loss.py:8-21, pSp/scripts/calc_id_loss_parallel.py:58-67, :100-103)')
    parser.add_argument('--weights', required=True, help="the Backbone state dict in the reference's layout (model_ir_se50.pth)")
    parser.add_argument('--a', required=True, help='a torch file holding [N,3,S,S] images in [-1, 1]')
    parser.add_argument('--b', required=True, help='a second file of the same shape: image i of --a is paired with image i of --b')
    parser.add_argument('--batch', type=int, default=16)
    parser.add_argument('--box', type=int, nargs=4, default=list(BOX), metavar=('Y0', 'Y1', 'X0', 'X1'), help='the crop in front of the pool')
    parser.add_argument('--pool', type=int, default=POOL, help='side of the plane the network sees')
    return parser


def result_line(scores):
    """calc_id_loss_parallel.py:100-103 (np.mean, np.std: the population deviation)"""
    s = torch.as_tensor(scores, dtype=torch.float64)
    return 'New Average score is {:.2f}+-{:.2f}'.format(float(s.mean()), float(s.std(unbiased=False)))


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.batch < 1:
        raise SystemExit('--batch must be positive')
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    net = ArcFaceID(args.weights, box=tuple(args.box), pool=args.pool)
    a, b = (torch.load(p, map_location='cpu') for p in (args.a, args.b))
    if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.shape != b.shape:
        raise SystemExit('--a and --b must hold two image tensors of one shape')
    sims = []
    for at in range(0, a.shape[0], args.batch):
        ea, eb = (net(t[at:at + args.batch].to('cuda')) for t in (a, b))
        sims.append(net.similarity(ea, eb).double().cpu())
    sims = torch.cat(sims)
    print(result_line(sims))
    print(json.dumps({'metric': 'arcface_id_similarity', 'n': int(sims.numel()), 'mean': float(sims.mean()),
                      'std': float(sims.std(unbiased=False)), 'units': len(net.units), 'dim': net.dim, 'box': list(net.box),
                      'pool': net.pool}))
    return sims


if __name__ == '__main__':
    main(sys.argv[1:])

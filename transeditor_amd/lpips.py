"""LPIPS-VGG perceptual distance on the gfx950 kernels (the reference's `utils.lpips.PerceptualLoss(model='net-lin', net='vgg')`,
utils/lpips/__init__.py:12-39, dist_model.py:55-67 and :90, networks_basic.py:21-87, pretrained_networks.py:98-136).

    percept = PerceptualLoss(vgg_path='vgg16-397923af.pth', lin_path='vgg.pth')
    d = percept(pred, target)                      # [N,1,1,1]; target of batch 1 broadcasts over pred
    tf = percept.target_features(target)           # a fixed target through the trunk once ...
    d = percept(pred, tf)                          # ... and reused: bit-identical to percept(pred, target)
    d = percept.pair_distance(images)              # [2N,3,H,W] -> [N]: images 2n and 2n+1, forward only (the PPL metric)

Weights come from local files only (nothing is downloaded, torchvision is not imported): `vgg_path` is a torchvision vgg16 state
dict (features.{0,2,...,28}.{weight,bias}), `lin_path` the LPIPS v0.1 head file (lin{0..4}.model.1.weight [1,C,1,1]).  The trunk is
frozen (buffers): the distance is differentiable with respect to `pred` only; the target is a constant.

Hot path: the stem (scaling layer + conv1_1 + ReLU), the max-pools and the five heads are csrc/lpips.hip; conv1_2 ... conv5_3 run on
the project's plain 3x3 convolution (op/modconv.py planner: split Winograd, Winograd or direct) with the bias in the epilogue and
ReLU as te_bias_act_f32 with alpha 0.  Eval mode: the reference's dropout in the heads is the identity.
"""
import os

import torch
from torch.autograd import Function

from . import _lib
from .frozen_net import POOL_AFTER, VGGTrunk, check_images, load, weight_bias  # noqa: F401  (POOL_AFTER, VGGTrunk: importable from here)
from .op import modconv

VGG_CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # conv layers of torchvision vgg16.features[0:30]
VGG_CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
TAPS = (1, 3, 6, 9, 12)          # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (pretrained_networks.py:98-136, five slices)
LIN_CHANNELS = (64, 128, 256, 512, 512)


def default_vgg_path():
    """where torchvision would have cached the ImageNet vgg16 weights (never fetched from here)"""
    return os.path.join(torch.hub.get_dir(), 'checkpoints', 'vgg16-397923af.pth')


def vgg16_convs(sd, path, who='LPIPS'):
    """[(weight [Co,Ci,3,3], bias [Co])] * 13 from a torchvision vgg16 state dict (other keys ignored); `path` names it in messages"""
    out, ci = [], 3
    for idx, co in zip(VGG_CONV_INDEX, VGG_CHANNELS):
        out.append(weight_bias(sd, f'features.{idx}.weight', f'features.{idx}.bias', (co, ci, 3, 3), who, path,
                               'not a torchvision vgg16 state dict'))
        ci = co
    return out


def load_vgg16(path):
    """vgg16_convs of the state dict in the file `path`"""
    return vgg16_convs(load(path, 'vgg16', 'LPIPS'), path)


def load_lin(path):
    """[w [C]] * 5 from the LPIPS v0.1 head file (lin{l}.model.1.weight [1,C,1,1])"""
    sd = load(path, 'LPIPS lin', 'LPIPS')
    return [weight_bias(sd, f'lin{l}.model.1.weight', None, (1, c, 1, 1), 'LPIPS', path, 'not an LPIPS v0.1 vgg head file')
            .detach().float().reshape(c).contiguous() for l, c in enumerate(LIN_CHANNELS)]


class TargetFeatures:
    """normalised relu1_2 ... relu5_3 features of a fixed target (PerceptualLoss.target_features)"""

    def __init__(self, feats, shape):
        self.feats, self.shape = feats, shape


class _Distance(Function):
    """d[n] = LPIPS(pred[n], target); backward -> gradient w.r.t. pred only"""

    @staticmethod
    def forward(ctx, pred, net, tfeats):
        acts = net._trunk(pred)
        partials = [_lib.lpips_head_fwd(acts[i], t, net._lin(l)) for l, (i, t) in enumerate(zip(TAPS, tfeats))]
        d = _lib.lpips_dist(partials, [acts[i].shape[2] * acts[i].shape[3] for i in TAPS])
        ctx.net, ctx.acts, ctx.tfeats = net, acts, tfeats
        return d

    @staticmethod
    def backward(ctx, gd):
        net, acts, tfeats = ctx.net, ctx.acts, ctx.tfeats
        gd = gd.contiguous()
        g = None                           # gradient w.r.t. acts[i] (a ReLU output)
        for i in range(12, 0, -1):
            if i in TAPS:
                l = TAPS.index(i)
                gpre = _lib.lpips_head_bwd(gd, acts[i], tfeats[l], net._lin(l), gin=g, relu_mask=True)
            else:
                gpre = _lib.bias_act(g, None, acts[i], 3, 1, 0.0, 1.0)          # ReLU mask (grad 31, alpha 0)
            gin = net._conv_dgrad(i, gpre)
            g = _lib.maxpool2_bwd(gin, acts[i - 1]) if (i - 1) in POOL_AFTER else gin
        ctx.acts = None
        return _lib.lpips_stem_dgrad(g, acts[0], net._w(0)), None, None


class PerceptualLoss(VGGTrunk, torch.nn.Module):
    def __init__(self, model='net-lin', net='vgg', colorspace='rgb', spatial=False, use_gpu=True, gpu_ids=[0], vgg_path=None,
                 lin_path=None):
        super().__init__()
        if model != 'net-lin':
            raise NotImplementedError(f"PerceptualLoss: model '{model}' (only 'net-lin' is built)")
        if net != 'vgg':
            raise NotImplementedError(f"PerceptualLoss: net '{net}' (only 'vgg' is built)")
        if spatial:
            raise NotImplementedError('PerceptualLoss: spatial=True is not built')
        if lin_path is None:
            raise ValueError('PerceptualLoss: lin_path (the LPIPS v0.1 vgg head file) is required; nothing is downloaded')
        self.model, self.net, self.colorspace, self.spatial = model, net, colorspace, spatial   # (colorspace: unused by net-lin)
        vgg = load_vgg16(vgg_path if vgg_path is not None else default_vgg_path())
        lin = load_lin(lin_path)
        self._freeze(vgg, [(f'lin{l}', w) for l, w in enumerate(lin)], device=f'cuda:{gpu_ids[0]}' if use_gpu else None, evaluate=False)

    def _lin(self, l):
        return getattr(self, f'lin{l}')

    def _conv_dgrad(self, i, g):
        w = self._w(i)
        B, _, H, W = g.shape
        pk, ck = modconv.bwd_kinds('3x3', B, w, H, W)
        return _lib.conv(g, self._packed(i, pk), ck, w.shape[1], H, W)

    def _stem(self, x, who='PerceptualLoss', dims='[N,3,H,W]', pairs=False):
        """relu1_1 of x in [-1, 1], after the input checks"""
        check_images(x, who, dims, pairs=pairs)
        if x.shape[2] % 16 or x.shape[3] % 16:
            raise ValueError(f'PerceptualLoss: H and W must be multiples of 16, got {x.shape[2]}x{x.shape[3]}')
        return _lib.lpips_stem_fwd(x, self._w(0), self.b0)

    def _trunk(self, x):
        """the 13 ReLU outputs of vgg16.features[0:30] for x in [-1, 1]"""
        acts = []
        self._walk(lambda: self._stem(x), lambda i, a: acts.append(a))
        return acts

    @torch.no_grad()
    def target_features(self, target, normalize=False):
        """the target's normalised tap features, computed once (pass the result as `target` to forward)"""
        if normalize:
            target = 2 * target - 1
        target = target.detach().contiguous()
        acts = self._trunk(target)
        return TargetFeatures([_lib.lpips_normalize(acts[i]) for i in TAPS], tuple(target.shape))

    @torch.no_grad()
    def pair_distance(self, images, normalize=False):
        """[2N,3,H,W] -> [N]: the distance of images 2n and 2n+1 (metrics/evaluate_query.py:234: percept(image[::2], image[1::2])).
        Forward only.  The trunk runs once over the interleaved batch; an activation is dropped once its tap's head and the next
        layer have read it; the heads normalise both sides themselves (te_lpips_pair_head_fwd_f32), so no normalised features are
        stored."""
        if normalize:
            images = 2 * images - 1
        partials, hws = [], []

        def head(i, a):
            if i in TAPS:
                partials.append(_lib.lpips_pair_head_fwd(a, self._lin(TAPS.index(i))))
                hws.append(a.shape[2] * a.shape[3])
        self._walk(lambda: self._stem(images.detach(), 'PerceptualLoss.pair_distance', '[2N,3,H,W]', pairs=True), head)
        return _lib.lpips_dist(partials, hws)

    def forward(self, pred, target, normalize=False):
        """[N,1,1,1]: the reference calls model.forward(target, pred); the squared difference is symmetric"""
        if normalize:
            pred = 2 * pred - 1
        tf = target if isinstance(target, TargetFeatures) else self.target_features(target, normalize)
        if tf.shape[1:] != tuple(pred.shape[1:]) or tf.shape[0] not in (1, pred.shape[0]):
            raise ValueError(f'PerceptualLoss: target {tf.shape} does not match pred {tuple(pred.shape)} (batch 1 or equal)')
        d = _Distance.apply(pred.contiguous(), self, tf.feats)
        return d.view(-1, 1, 1, 1)

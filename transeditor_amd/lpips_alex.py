"""The AlexNet LPIPS of the diversity score on the gfx950 kernels (the reference's metrics/lpips.py:49-82 LPIPS, as
metrics/evaluate_query.py:82-133 uses it): torchvision's alexnet().features with a tap after each of the five ReLUs, each tap
normalised as f * rsqrt(sum_c f^2 + 1e-10), and per layer the spatial mean of sum_c w_l[c] (fa - fb)^2, summed over the layers.

    lp = AlexLPIPS('alexnet-owt-7be5be79.pth', 'lpips_weights.ckpt')
    D = lp.pairwise(images)                                         # [N,3,H,W] in [-1, 1] -> [N,N]: every pair of the group
    v = lp.group_mean(images)                                       # the mean of the N (N - 1) / 2 pairs: the reference's figure for a group
    d = lp(x, y)                                                    # LPIPS.forward(x, y): the mean over the batch of the paired distances

The reference scores a group of 40 images as 780 calls of LPIPS.forward, each of which runs the network on both images again.  Here
the network runs once over the group and the pairs are a property of the head: te_lpips_allpairs_fwd_f32 reads each normalised tap
about N / 8 + 1 times.  This is NOT the LPIPS-VGG of transeditor_amd.lpips: another network, another input scaling site (the same
constants), and the eps inside the root instead of beside it.

Weights come from local files: a torchvision alexnet state dict (keys features.{0,3,6,8,10}.{weight,bias}; classifier.* is ignored;
the default path is the torch hub cache file) and the reference's own metrics/lpips_weights.ckpt (keys
lpips_weights.{0..4}.main.1.weight, each [1,C,1,1]).  Nothing is downloaded and torchvision is not imported.  The five widths are
read from the shapes, and a head whose width differs from its tap's is refused.

Layers: te_alex_stem_fwd_f32 ((x - mu) / sigma, conv1 11 x 11 stride 4 pad 2, ReLU in one pass), te_pool3_f32 (max, stride 2),
te_conv2d_f32 with its ReLU for conv2 ... conv5 (a pool in front of conv3 as well; the last pool of `features` feeds nothing and is
not run), te_lpips_unit_f32 in place on each tap once the next layer has read it, then five te_lpips_allpairs_fwd_f32 launches and
one te_lpips_allpairs_dist_f32.  Only the five taps stay alive.  D is symmetric bit for bit with an exactly zero diagonal, and
D[i,j] does not depend on the group that images i and j are scored in.  Eval only: there is no backward pass.
Measured times and shares: profiles/README.md, 'LPIPS diversity'.

AlexLPIPSLoss is the OTHER AlexNet LPIPS of the reference, the lpips_lambda term of encoder training (pSp/criteria/lpips/lpips.py:29-35
LPIPS('alex') as pSp/training/coach_new.py:285-320 calc_loss calls it), with its backward pass:

    lpips_loss = AlexLPIPSLoss('alexnet-owt-7be5be79.pth', 'alex.pth')      # torchvision alexnet weights, the richzhang v0.1 alex heads
    loss = lpips_loss(inversed, real)                               # 0-dim: sum_l sum_b mean_p sum_c w_l[c] (fx - fy)^2 / B
    loss.backward()                                                 # the gradient reaches `inversed` and nothing else

The same trunk, but each tap is normalised as f / (sqrt(sum_c f^2) + 1e-10), eps beside the root (pSp/criteria/lpips/utils.py:6-8): the
heads are te_lpips_normalize_f32 / te_lpips_head_fwd_f32 / te_lpips_dist_f32 of csrc/lpips.hip, and backwards te_lpips_head_bwd_f32,
te_conv2d_dgrad_f32 and the two adjoints of csrc/lpips_alex_bwd.hip (te_pool3s2_max_bwd_f32, te_alex_stem_dgrad_f32).  Times:
profiles/README.md, 'LPIPS loss'.
"""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .frozen_net import check_images, no_gpu, resolve, weight_bias

CONVS = (0, 3, 6, 8, 10)                                              # the Conv2d children of alexnet().features
GEOMETRY = ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))   # (kernel, stride, padding)
POOL_BEFORE = (1, 2)                                                  # MaxPool2d(3, 2) in front of these convolutions
MIN_SIDE = 7                                                          # 7 + 2 * 2 = 11: conv1 gives one pixel
ALEXNET_FILE = 'alexnet-owt-7be5be79.pth'
_NO_GPU = no_gpu('AlexLPIPS')
_HINT = 'not a torchvision alexnet state dict: features.{0,3,6,8,10}.{weight,bias}'
_LIN_HINT = "not the reference's metrics/lpips_weights.ckpt: lpips_weights.{0..4}.main.1.weight"


def default_alexnet_path():
    return os.path.join(torch.hub.get_dir(), 'checkpoints', ALEXNET_FILE)


def parse_convs(sd, path='state_dict', who='AlexLPIPS'):
    """the convolution half of parse_state_dicts: [(w, b)] * 5 from a torchvision alexnet state dict"""
    convs, ci = [], 3
    for i, (k, _, _) in zip(CONVS, GEOMETRY):
        w, b = weight_bias(sd, f'features.{i}.weight', f'features.{i}.bias', (None, ci, k, k), who, path, _HINT)
        convs.append((w, b))
        ci = w.shape[0]
    return convs


def parse_state_dicts(sd, lin, path='state_dict', lin_path='lin_state_dict'):
    """-> dict(convs [(w, b)] * 5, heads [w [C]] * 5, widths); a ValueError naming the key that is missing, has the wrong shape, or
    whose width differs from its tap's"""
    convs, heads = parse_convs(sd, path), []
    for l, (w, _) in enumerate(convs):
        key = f'lpips_weights.{l}.main.1.weight'
        h = weight_bias(lin, key, None, (1, None, 1, 1), 'AlexLPIPS', lin_path, _LIN_HINT)
        if h.shape[1] != w.shape[0]:
            raise ValueError(f'AlexLPIPS: {key} has {h.shape[1]} channels, but its tap features.{CONVS[l]} has {w.shape[0]}')
        heads.append(h.detach().float().reshape(-1).contiguous())
    return dict(convs=convs, heads=heads, widths=tuple(w.shape[0] for w, _ in convs))


class AlexLPIPS(torch.nn.Module):
    def __init__(self, alexnet_path=None, lin_path=None, state_dict=None, lin_state_dict=None):
        super().__init__()
        if state_dict is None and alexnet_path is None:
            alexnet_path = default_alexnet_path()
        state_dict, alexnet_path = resolve(alexnet_path, state_dict, 'AlexLPIPS', 'torchvision alexnet weight', arg='alexnet_path',
                                           note='; nothing is downloaded: pass alexnet_path or state_dict')
        lin_state_dict, lin_path = resolve(lin_path, lin_state_dict, 'AlexLPIPS', 'AlexNet LPIPS head (metrics/lpips_weights.ckpt)',
                                           arg='lin_path')
        net = parse_state_dicts(state_dict, lin_state_dict, alexnet_path, lin_path)
        self.widths = net['widths']
        for l, ((w, b), h) in enumerate(zip(net['convs'], net['heads'])):
            self.register_buffer(f'w{l}', w)
            self.register_buffer(f'b{l}', b)
            self.register_buffer(f'lin{l}', h)
        self.eval()
        if torch.cuda.is_available():
            self.to('cuda')

    def _taps(self, images):
        """[N,3,H,W] -> the five normalised taps.  A tap is normalised in place once the next layer has read it, so nothing but the
        taps (and one pooled tensor at a time) is alive."""
        check_images(images, 'AlexLPIPS', '[N,3,H,W]')
        if images.shape[2] < MIN_SIDE or images.shape[3] < MIN_SIDE:
            raise ValueError(f'AlexLPIPS: H and W must be at least {MIN_SIDE}, got {images.shape[2]}x{images.shape[3]}')
        if not images.is_cuda:
            raise RuntimeError(_NO_GPU)
        taps = [_lib.alex_stem_fwd(images.detach().float(), self.w0, self.b0)]
        for l in range(1, 5):
            a = taps[-1]
            k, s, p = GEOMETRY[l]
            if l in POOL_BEFORE:
                if a.shape[2] < 3 or a.shape[3] < 3:
                    raise ValueError(f'AlexLPIPS: {images.shape[2]}x{images.shape[3]} images leave a {a.shape[2]}x{a.shape[3]} plane in front '
                                     f'of the max pool of features.{CONVS[l] - 1}, which needs 3x3')
                a = _lib.pool3(a, _lib.POOL3_MAX_S2)
            nxt = _lib.conv2d(a, getattr(self, f'w{l}'), getattr(self, f'b{l}'), s, (p, p), act=1)
            del a
            _lib.lpips_unit(taps[-1], out=taps[-1])
            taps.append(nxt)
        _lib.lpips_unit(taps[-1], out=taps[-1])
        return taps

    @torch.no_grad()
    def pairwise(self, images):
        """[N,3,H,W] in [-1, 1] -> D [N,N] fp32 on the device: D[i,j] = LPIPS(images[i], images[j]); symmetric, zero diagonal"""
        taps = self._taps(images)
        partials = [_lib.lpips_allpairs_fwd(t, getattr(self, f'lin{l}')) for l, t in enumerate(taps)]
        return _lib.lpips_allpairs_dist(partials, [(t.shape[1], t.shape[2] * t.shape[3]) for t in taps], images.shape[0])

    @torch.no_grad()
    def group_mean(self, images):
        """-> 0-d tensor: the mean of the N (N - 1) / 2 values with i < j (evaluate_query.py:82-91)"""
        if images.ndim == 4 and images.shape[0] < 2:
            raise ValueError(f'AlexLPIPS: a group needs at least 2 images, got {images.shape[0]}')
        D = self.pairwise(images)
        i, j = torch.triu_indices(D.shape[0], D.shape[0], 1, device=D.device)
        return D[i, j].mean()

    @torch.no_grad()
    def forward(self, x, y):
        """LPIPS.forward(x, y) for [B,3,H,W] or [3,H,W] inputs -> 0-d tensor: the mean over the batch of d(x[b], y[b]) (the
        reference's torch.mean runs over the batch and the plane together)"""
        if x.shape != y.shape or x.ndim not in (3, 4):
            raise ValueError(f'AlexLPIPS: x and y must be [B,3,H,W] or [3,H,W] of one shape, got {tuple(x.shape)}, {tuple(y.shape)}')
        if x.ndim == 3:
            x, y = x[None], y[None]
        B = x.shape[0]
        D = self.pairwise(torch.cat([x, y]))
        b = torch.arange(B, device=D.device)
        return D[b, b + B].mean()


# ------------------------------------------------------------------------------------------------------------ the loss form
MIN_LOSS_SIDE = 31                                                    # 31 -> 7 -> 3 -> 1: both pools see a 3 x 3 plane
_LOSS = 'AlexLPIPSLoss'
_LOSS_LIN_HINT = 'not an LPIPS v0.1 alex head file: lin{0..4}.model.1.weight, or {0..4}.1.weight as pSp renames them'


def parse_loss_heads(lin, widths, path='lin_state_dict'):
    """[w [C]] * 5 from a richzhang alex.pth state dict (lin{l}.model.1.weight [1,C,1,1]; pSp/criteria/lpips/utils.py:22-28 renames the
    keys to {l}.1.weight, which is accepted too); a ValueError naming the key that is missing, misshapen or of another width than its tap"""
    heads = []
    for l, c in enumerate(widths):
        key = next((k for k in (f'lin{l}.model.1.weight', f'{l}.1.weight') if k in lin), f'lin{l}.model.1.weight')
        h = weight_bias(lin, key, None, (1, None, 1, 1), _LOSS, path, _LOSS_LIN_HINT)
        if h.shape[1] != c:
            raise ValueError(f'{_LOSS}: {key} has {h.shape[1]} channels, but its tap features.{CONVS[l]} has {c}')
        heads.append(h.detach().float().reshape(-1).contiguous())
    return heads


def _pooled(n):
    return (n - 3) // 2 + 1


class _Loss(Function):
    """sum_b LPIPS(x[b], y[b]) / B; backward -> the gradient w.r.t. x only (y is a constant), once"""

    @staticmethod
    def forward(ctx, x, net, y):
        taps = net._trunk(x)
        hats = [_lib.lpips_normalize(t) for t in net._trunk(y)]
        partials = [_lib.lpips_head_fwd(t, h, net._lin(l)) for l, (t, h) in enumerate(zip(taps, hats))]
        d = _lib.lpips_dist(partials, [t.shape[2] * t.shape[3] for t in taps])
        ctx.net, ctx.taps, ctx.hats, ctx.shape = net, taps, hats, tuple(x.shape)
        return d.sum() / x.shape[0]                                             # lpips.py:35

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        net, taps, hats = ctx.net, ctx.taps, ctx.hats
        if taps is None:
            raise RuntimeError(f'{_LOSS}: backward was called a second time; the taps of the forward pass are kept for one backward pass')
        ctx.taps = ctx.hats = None
        B = ctx.shape[0]
        gd = (gout / B).reshape(1).expand(B).contiguous()                       # d loss / d d[b]
        g = None                                                                # the gradient arriving at tap l from the layer above
        for l in range(4, 0, -1):
            gpre = _lib.lpips_head_bwd(gd, taps[l], hats[l], net._lin(l), gin=g, relu_mask=True)
            k, s, p = GEOMETRY[l]
            below = taps[l - 1]
            shape = tuple(below.shape) if l not in POOL_BEFORE else (*below.shape[:2], _pooled(below.shape[2]), _pooled(below.shape[3]))
            g = _lib.conv2d_dgrad(gpre, net._wt(l), shape, (k, k), s, (p, p))
            if l in POOL_BEFORE:
                g = _lib.pool3s2_max_bwd(g, below)
            taps[l] = hats[l] = gpre = None
        gpre = _lib.lpips_head_bwd(gd, taps[0], hats[0], net._lin(0), gin=g, relu_mask=True)
        return _lib.alex_stem_dgrad(gpre, net._wt(0), ctx.shape), None, None


class AlexLPIPSLoss(torch.nn.Module):
    def __init__(self, alexnet_path=None, lin_path=None, state_dict=None, lin_state_dict=None):
        super().__init__()
        if state_dict is None and alexnet_path is None:
            alexnet_path = default_alexnet_path()
        state_dict, alexnet_path = resolve(alexnet_path, state_dict, _LOSS, 'torchvision alexnet weight', arg='alexnet_path',
                                           note='; nothing is downloaded: pass alexnet_path or state_dict')
        lin_name = 'lin_state_dict' if lin_state_dict is not None else None     # (resolve names every dict 'state_dict')
        lin_state_dict, lin_path = resolve(lin_path, lin_state_dict, _LOSS, 'LPIPS v0.1 alex head (alex.pth)', arg='lin_path')
        lin_path = lin_name or lin_path
        convs = parse_convs(state_dict, alexnet_path, _LOSS)
        self.widths = tuple(w.shape[0] for w, _ in convs)
        heads = parse_loss_heads(lin_state_dict, self.widths, lin_path)
        for l, ((w, b), h) in enumerate(zip(convs, heads)):
            k, s, p = GEOMETRY[l]
            self.register_buffer(f'w{l}', w)
            self.register_buffer(f'b{l}', b)
            self.register_buffer(f'lin{l}', h)
            # the weights as the data gradients read them, made once: the network is frozen
            self.register_buffer(f'wt{l}', _lib.alex_stem_dgrad_weight(w) if l == 0 else _lib.dgrad_weight(w, s, (p, p)), persistent=False)
        self.eval()
        if torch.cuda.is_available():
            self.to('cuda')

    def _lin(self, l):
        return getattr(self, f'lin{l}')

    def _wt(self, l):
        return getattr(self, f'wt{l}')

    def _trunk(self, images):
        """[B,3,H,W] -> the five raw taps (the ReLU outputs of conv1 ... conv5); all five stay alive for the backward pass"""
        taps = [_lib.alex_stem_fwd(images, self.w0, self.b0)]
        for l in range(1, 5):
            a = taps[-1]
            k, s, p = GEOMETRY[l]
            if l in POOL_BEFORE:
                a = _lib.pool3(a, _lib.POOL3_MAX_S2)
            taps.append(_lib.conv2d(a, getattr(self, f'w{l}'), getattr(self, f'b{l}'), s, (p, p), act=1))
        return taps

    @staticmethod
    def _check(x, y):
        check_images(x, _LOSS)
        if tuple(x.shape) != tuple(y.shape):
            raise ValueError(f'{_LOSS}: x and y must have one shape, got {tuple(x.shape)}, {tuple(y.shape)}')
        H, W = x.shape[2:]
        h, w = (H - 7) // 4 + 1, (W - 7) // 4 + 1                              # conv1; conv2 keeps the plane
        for l in POOL_BEFORE:
            if h < 3 or w < 3:
                raise ValueError(f'{_LOSS}: {H}x{W} images leave a {max(h, 0)}x{max(w, 0)} plane in front of the max pool of features.{CONVS[l] - 1}, '
                                 f'which needs 3x3: H and W must be at least {MIN_LOSS_SIDE}')
            h, w = _pooled(h), _pooled(w)

    def forward(self, x, y):
        """LPIPS.forward(x, y) of pSp/criteria/lpips/lpips.py for [B,3,H,W] images in [-1, 1] -> 0-dim tensor; differentiable once with
        respect to x.  A window such as img[:, :, 35:223, 32:220] is copied to a contiguous tensor here, by torch, whose slicing
        carries the gradient back to img."""
        self._check(x, y)
        if not (x.is_cuda and y.is_cuda):
            raise RuntimeError(_NO_GPU)
        return _Loss.apply(x.float().contiguous(), self, y.detach().float().contiguous())

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
"""
import os

import torch

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


def parse_state_dicts(sd, lin, path='state_dict', lin_path='lin_state_dict'):
    """-> dict(convs [(w, b)] * 5, heads [w [C]] * 5, widths); a ValueError naming the key that is missing, has the wrong shape, or
    whose width differs from its tap's"""
    convs, heads, ci = [], [], 3
    for i, (k, _, _) in zip(CONVS, GEOMETRY):
        w, b = weight_bias(sd, f'features.{i}.weight', f'features.{i}.bias', (None, ci, k, k), 'AlexLPIPS', path, _HINT)
        convs.append((w, b))
        ci = w.shape[0]
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

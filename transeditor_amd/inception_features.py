"""Inception-v3 pool3 features on the gfx950 kernels: the feature extractor of the reference's FID (metrics/inception.py InceptionV3 with
use_fid_inception=True and output_blocks=[3], as metrics/calc_inception.py:55 and metrics/fid_query.py:86 build it with
normalize_input=False: the 2048-d output of the final average pool of the TensorFlow-FID network).

    net = InceptionV3Features('pt_inception-2015-12-05-6726825d.pth')    # the pytorch-fid weight file, from a local path
    f = net(images)                                                      # [B,3,H,W] in [-1, 1] -> [B,2048]
    evaluate_fid(G, net, 'inception_ffhq.pkl')                           # an instance is a feature_fn of transeditor_amd.fid

Weights come from a local state dict with torchvision's keys (<layer>.conv.weight, <layer>.bn.{weight,bias,running_mean,running_var};
fc.* and num_batches_tracked are ignored).  Nothing is downloaded and torchvision is not imported.  As in the reference the image is
resized to 299 x 299 (bilinear, align_corners=False) and goes into Conv2d_1a_3x3 as it is.

Every layer is conv (no bias) + BatchNorm(eps 0.001, eval) + ReLU.  The batch norm is folded into the convolution when the weights
are loaded, in fp64 on the host and rounded once: g = gamma / sqrt(var + eps), w' = w g, b' = beta - mean g.  All 94 convolutions run
on te_conv2d_f32 with bias and ReLU in its epilogue; every branch of a Mixed block writes into its channel slice of the block's one
output tensor (there is no torch.cat); the pools are te_pool3_f32, the resize te_resize_bilinear_f32 and the final global average
te_adaptive_avgpool_f32.  The FID network's patches are kept: the average pools of the A, C and first E block do not count the
padding, and the last block (Mixed_7c) pools with a 3 x 3 MAX.  Eval only: no backward pass.  The convolution sums each output as one
fp32 chain whose order depends on the layer alone, so an image's features are bitwise the same whatever batch it is in.

Measured throughput and shares: profiles/README.md, 'Inception-v3 pool3 features'.
"""
import os

import torch

from . import _lib
from .frozen_net import check_images, no_gpu, resolve, weight_bias

WEIGHTS_FILE = 'pt_inception-2015-12-05-6726825d.pth'
BN_EPS = 0.001
FEATURE_DIM = 2048
MIN_SIZE = 75                    # the smallest input that still reaches Mixed_7a's stride-2 layers with 3 x 3 pixels
_NO_GPU = no_gpu('InceptionV3Features')
_HINT = "not an Inception-v3 state dict with torchvision's keys"


def default_inception_path():
    """where torch's hub cache would hold the pytorch-fid Inception weights (never fetched from here)"""
    return os.path.join(torch.hub.get_dir(), 'checkpoints', WEIGHTS_FILE)


def _c(name, ci, co, k=1, stride=1, pad=0):
    k = (k, k) if isinstance(k, int) else k
    pad = (pad, pad) if isinstance(pad, int) else pad
    return name, ci, co, k, stride, pad


def _block_a(n, ci, pf):
    return [_c(f'{n}.branch1x1', ci, 64), _c(f'{n}.branch5x5_1', ci, 48), _c(f'{n}.branch5x5_2', 48, 64, 5, pad=2),
            _c(f'{n}.branch3x3dbl_1', ci, 64), _c(f'{n}.branch3x3dbl_2', 64, 96, 3, pad=1), _c(f'{n}.branch3x3dbl_3', 96, 96, 3, pad=1),
            _c(f'{n}.branch_pool', ci, pf)]


def _block_b(n, ci):
    return [_c(f'{n}.branch3x3', ci, 384, 3, 2), _c(f'{n}.branch3x3dbl_1', ci, 64), _c(f'{n}.branch3x3dbl_2', 64, 96, 3, pad=1),
            _c(f'{n}.branch3x3dbl_3', 96, 96, 3, 2)]


def _block_c(n, ci, c7):
    row, col = dict(k=(1, 7), pad=(0, 3)), dict(k=(7, 1), pad=(3, 0))
    return [_c(f'{n}.branch1x1', ci, 192),
            _c(f'{n}.branch7x7_1', ci, c7), _c(f'{n}.branch7x7_2', c7, c7, **row), _c(f'{n}.branch7x7_3', c7, 192, **col),
            _c(f'{n}.branch7x7dbl_1', ci, c7), _c(f'{n}.branch7x7dbl_2', c7, c7, **col), _c(f'{n}.branch7x7dbl_3', c7, c7, **row),
            _c(f'{n}.branch7x7dbl_4', c7, c7, **col), _c(f'{n}.branch7x7dbl_5', c7, 192, **row),
            _c(f'{n}.branch_pool', ci, 192)]


def _block_d(n, ci):
    return [_c(f'{n}.branch3x3_1', ci, 192), _c(f'{n}.branch3x3_2', 192, 320, 3, 2),
            _c(f'{n}.branch7x7x3_1', ci, 192), _c(f'{n}.branch7x7x3_2', 192, 192, (1, 7), pad=(0, 3)),
            _c(f'{n}.branch7x7x3_3', 192, 192, (7, 1), pad=(3, 0)), _c(f'{n}.branch7x7x3_4', 192, 192, 3, 2)]


def _block_e(n, ci):
    row, col = dict(k=(1, 3), pad=(0, 1)), dict(k=(3, 1), pad=(1, 0))
    return [_c(f'{n}.branch1x1', ci, 320),
            _c(f'{n}.branch3x3_1', ci, 384), _c(f'{n}.branch3x3_2a', 384, 384, **row), _c(f'{n}.branch3x3_2b', 384, 384, **col),
            _c(f'{n}.branch3x3dbl_1', ci, 448), _c(f'{n}.branch3x3dbl_2', 448, 384, 3, pad=1),
            _c(f'{n}.branch3x3dbl_3a', 384, 384, **row), _c(f'{n}.branch3x3dbl_3b', 384, 384, **col),
            _c(f'{n}.branch_pool', ci, 192)]


# (name, Ci, Co, (kh, kw), stride, (py, px)) of all 94 convolutions, in the order forward() runs them
LAYERS = tuple(
    [_c('Conv2d_1a_3x3', 3, 32, 3, 2), _c('Conv2d_2a_3x3', 32, 32, 3), _c('Conv2d_2b_3x3', 32, 64, 3, pad=1),
     _c('Conv2d_3b_1x1', 64, 80), _c('Conv2d_4a_3x3', 80, 192, 3)]
    + _block_a('Mixed_5b', 192, 32) + _block_a('Mixed_5c', 256, 64) + _block_a('Mixed_5d', 288, 64)
    + _block_b('Mixed_6a', 288)
    + _block_c('Mixed_6b', 768, 128) + _block_c('Mixed_6c', 768, 160) + _block_c('Mixed_6d', 768, 160) + _block_c('Mixed_6e', 768, 192)
    + _block_d('Mixed_7a', 768)
    + _block_e('Mixed_7b', 1280) + _block_e('Mixed_7c', 2048))
_BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS, dtype=torch.float32):
    """conv (no bias) followed by an eval-mode batch norm -> (w', b') fp32: fp64 arithmetic on the host, one rounding (dtype=
    torch.float64: the values before it)"""
    g = gamma.detach().double().cpu() / torch.sqrt(var.detach().double().cpu() + eps)
    wf = w.detach().double().cpu() * g.view(-1, 1, 1, 1)
    bf = beta.detach().double().cpu() - mean.detach().double().cpu() * g
    return wf.to(dtype).contiguous(), bf.to(dtype).contiguous()


def inception_convs(sd, path):
    """{layer: (w' [Co,Ci,kh,kw], b' [Co])} for all of LAYERS from a state dict with torchvision's keys; `path` names it in messages.
    Every shape is checked; keys that are not in LAYERS (fc.*, num_batches_tracked, AuxLogits) are ignored."""
    def get(key, shape):
        return weight_bias(sd, key, None, shape, 'InceptionV3Features', path, _HINT)
    return {name: fold_bn(get(f'{name}.conv.weight', (co, ci, *k)), *(get(f'{name}.bn.{b}', (co,)) for b in _BN_KEYS))
            for name, ci, co, k, _, _ in LAYERS}


class InceptionV3Features(torch.nn.Module):
    def __init__(self, weights_path=None, state_dict=None, resize_input=True):
        super().__init__()
        if state_dict is None and weights_path is None:
            weights_path = default_inception_path()
        state_dict, path = resolve(weights_path, state_dict, 'InceptionV3Features', 'Inception-v3 weight', arg='weights_path', named=False,
                                   note=f' (the pytorch-fid file {WEIGHTS_FILE}; it is never downloaded from here)')
        self.resize_input = bool(resize_input)
        self._spec = {}
        for i, (name, _, _, _, stride, pad) in enumerate(LAYERS):
            self._spec[name] = (i, stride, pad)
        for name, (w, b) in inception_convs(state_dict, path).items():
            i = self._spec[name][0]
            self.register_buffer(f'w{i}', w)
            self.register_buffer(f'b{i}', b)
        self.eval()
        if torch.cuda.is_available():
            self.to('cuda')

    # ---------------------------------------------------------------------------------------------------------------- layers
    def _conv(self, name, x, out=None, c0=0):
        i, stride, pad = self._spec[name]
        return _lib.conv2d(x, getattr(self, f'w{i}'), getattr(self, f'b{i}'), stride, pad, act=1, out=out, c0=c0)

    def _out(self, x, channels, reduce=False):
        H, W = x.shape[2:]
        if reduce:
            H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        return torch.empty(x.shape[0], channels, H, W, device=x.device, dtype=torch.float32)

    def _mixed_a(self, n, x, pf):
        out = self._out(x, 224 + pf)
        self._conv(f'{n}.branch1x1', x, out, 0)
        self._conv(f'{n}.branch5x5_2', self._conv(f'{n}.branch5x5_1', x), out, 64)
        t = self._conv(f'{n}.branch3x3dbl_2', self._conv(f'{n}.branch3x3dbl_1', x))
        self._conv(f'{n}.branch3x3dbl_3', t, out, 128)
        self._conv(f'{n}.branch_pool', _lib.pool3(x, _lib.POOL3_AVG_S1), out, 224)
        return out

    def _mixed_b(self, n, x):
        out = self._out(x, 384 + 96 + x.shape[1], reduce=True)
        self._conv(f'{n}.branch3x3', x, out, 0)
        t = self._conv(f'{n}.branch3x3dbl_2', self._conv(f'{n}.branch3x3dbl_1', x))
        self._conv(f'{n}.branch3x3dbl_3', t, out, 384)
        _lib.pool3(x, _lib.POOL3_MAX_S2, out, 480)
        return out

    def _mixed_c(self, n, x):
        out = self._out(x, 768)
        self._conv(f'{n}.branch1x1', x, out, 0)
        t = self._conv(f'{n}.branch7x7_2', self._conv(f'{n}.branch7x7_1', x))
        self._conv(f'{n}.branch7x7_3', t, out, 192)
        t = self._conv(f'{n}.branch7x7dbl_1', x)
        for j in (2, 3, 4):
            t = self._conv(f'{n}.branch7x7dbl_{j}', t)
        self._conv(f'{n}.branch7x7dbl_5', t, out, 384)
        self._conv(f'{n}.branch_pool', _lib.pool3(x, _lib.POOL3_AVG_S1), out, 576)
        return out

    def _mixed_d(self, n, x):
        out = self._out(x, 320 + 192 + x.shape[1], reduce=True)
        self._conv(f'{n}.branch3x3_2', self._conv(f'{n}.branch3x3_1', x), out, 0)
        t = self._conv(f'{n}.branch7x7x3_1', x)
        for j in (2, 3):
            t = self._conv(f'{n}.branch7x7x3_{j}', t)
        self._conv(f'{n}.branch7x7x3_4', t, out, 320)
        _lib.pool3(x, _lib.POOL3_MAX_S2, out, 512)
        return out

    def _mixed_e(self, n, x, pool):
        out = self._out(x, 2048)
        self._conv(f'{n}.branch1x1', x, out, 0)
        t = self._conv(f'{n}.branch3x3_1', x)
        self._conv(f'{n}.branch3x3_2a', t, out, 320)
        self._conv(f'{n}.branch3x3_2b', t, out, 704)
        t = self._conv(f'{n}.branch3x3dbl_2', self._conv(f'{n}.branch3x3dbl_1', x))
        self._conv(f'{n}.branch3x3dbl_3a', t, out, 1088)
        self._conv(f'{n}.branch3x3dbl_3b', t, out, 1472)
        self._conv(f'{n}.branch_pool', _lib.pool3(x, pool), out, 1856)
        return out

    @torch.no_grad()
    def forward(self, images):
        """[B,3,H,W] in [-1, 1] -> [B,2048] fp32 on the device.  resize_input=True: any H, W, resized to 299 x 299; False: any
        H, W >= 75.  An activation is dropped once its readers have run (no reference to it is left)."""
        check_images(images, 'InceptionV3Features')
        if not self.resize_input and (images.shape[2] < MIN_SIZE or images.shape[3] < MIN_SIZE):
            raise ValueError(f'InceptionV3Features: without resize_input H and W must be at least {MIN_SIZE}, got '
                             f'{images.shape[2]}x{images.shape[3]}')
        if not images.is_cuda:
            raise RuntimeError(_NO_GPU)
        a = images.detach().float().contiguous()
        if self.resize_input:
            a = _lib.resize_bilinear(a, 299, 299)
        for name in ('Conv2d_1a_3x3', 'Conv2d_2a_3x3', 'Conv2d_2b_3x3'):
            a = self._conv(name, a)
        a = _lib.pool3(a, _lib.POOL3_MAX_S2)
        a = self._conv('Conv2d_4a_3x3', self._conv('Conv2d_3b_1x1', a))
        a = _lib.pool3(a, _lib.POOL3_MAX_S2)
        a = self._mixed_a('Mixed_5b', a, 32)
        a = self._mixed_a('Mixed_5c', a, 64)
        a = self._mixed_a('Mixed_5d', a, 64)
        a = self._mixed_b('Mixed_6a', a)
        for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
            a = self._mixed_c(n, a)
        a = self._mixed_d('Mixed_7a', a)
        a = self._mixed_e('Mixed_7b', a, _lib.POOL3_AVG_S1)
        a = self._mixed_e('Mixed_7c', a, _lib.POOL3_MAX_S1)               # the FID network's quirk: a max pool in the last block
        return _lib.adaptive_avgpool(a, 1, 1).view(a.shape[0], FEATURE_DIM)

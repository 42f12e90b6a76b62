"""Plain-torch restatement of the FID's feature extractor (metrics/inception.py: the TensorFlow-FID Inception-v3 up to its final average
pool; no reference code is read at run time and torchvision is not imported), written from the architecture table:

    every "conv" = Conv2d(bias=False) -> BatchNorm2d(eps=0.001) in eval mode -> ReLU, UNFOLDED, as the reference computes it
    Conv2d_1a 3->32 k3 s2, 2a 32->32 k3, 2b 32->64 k3 p1, maxpool 3 s2, 3b 64->80 k1, 4a 80->192 k3, maxpool 3 s2,
    Mixed_5b/5c/5d (A), Mixed_6a (B), Mixed_6b/6c/6d/6e (C), Mixed_7a (D), Mixed_7b/7c (E), global average -> [B,2048]

indexed by torchvision's state dict keys, in whatever dtype it is asked for, and a synthetic state dict filled from a seed.  The FID
patches: the average pools of A, C and Mixed_7b do not count the padding, Mixed_7c pools with a 3 x 3 max.  Everything runs on the CPU
(torch's fp64 convolution is sure to exist there).
"""
import torch
import torch.nn.functional as F

EPS = 0.001


def _a(n, ci, pf):
    return {f'{n}.branch1x1': (ci, 64, 1, 1), f'{n}.branch5x5_1': (ci, 48, 1, 1), f'{n}.branch5x5_2': (48, 64, 5, 5),
            f'{n}.branch3x3dbl_1': (ci, 64, 1, 1), f'{n}.branch3x3dbl_2': (64, 96, 3, 3), f'{n}.branch3x3dbl_3': (96, 96, 3, 3),
            f'{n}.branch_pool': (ci, pf, 1, 1)}


def _b(n, ci):
    return {f'{n}.branch3x3': (ci, 384, 3, 3), f'{n}.branch3x3dbl_1': (ci, 64, 1, 1), f'{n}.branch3x3dbl_2': (64, 96, 3, 3),
            f'{n}.branch3x3dbl_3': (96, 96, 3, 3)}


def _c(n, ci, c7):
    return {f'{n}.branch1x1': (ci, 192, 1, 1),
            f'{n}.branch7x7_1': (ci, c7, 1, 1), f'{n}.branch7x7_2': (c7, c7, 1, 7), f'{n}.branch7x7_3': (c7, 192, 7, 1),
            f'{n}.branch7x7dbl_1': (ci, c7, 1, 1), f'{n}.branch7x7dbl_2': (c7, c7, 7, 1), f'{n}.branch7x7dbl_3': (c7, c7, 1, 7),
            f'{n}.branch7x7dbl_4': (c7, c7, 7, 1), f'{n}.branch7x7dbl_5': (c7, 192, 1, 7),
            f'{n}.branch_pool': (ci, 192, 1, 1)}


def _d(n, ci):
    return {f'{n}.branch3x3_1': (ci, 192, 1, 1), f'{n}.branch3x3_2': (192, 320, 3, 3),
            f'{n}.branch7x7x3_1': (ci, 192, 1, 1), f'{n}.branch7x7x3_2': (192, 192, 1, 7), f'{n}.branch7x7x3_3': (192, 192, 7, 1),
            f'{n}.branch7x7x3_4': (192, 192, 3, 3)}


def _e(n, ci):
    return {f'{n}.branch1x1': (ci, 320, 1, 1),
            f'{n}.branch3x3_1': (ci, 384, 1, 1), f'{n}.branch3x3_2a': (384, 384, 1, 3), f'{n}.branch3x3_2b': (384, 384, 3, 1),
            f'{n}.branch3x3dbl_1': (ci, 448, 1, 1), f'{n}.branch3x3dbl_2': (448, 384, 3, 3),
            f'{n}.branch3x3dbl_3a': (384, 384, 1, 3), f'{n}.branch3x3dbl_3b': (384, 384, 3, 1),
            f'{n}.branch_pool': (ci, 192, 1, 1)}


# layer -> (Ci, Co, kh, kw)
SHAPES = {'Conv2d_1a_3x3': (3, 32, 3, 3), 'Conv2d_2a_3x3': (32, 32, 3, 3), 'Conv2d_2b_3x3': (32, 64, 3, 3),
          'Conv2d_3b_1x1': (64, 80, 1, 1), 'Conv2d_4a_3x3': (80, 192, 3, 3),
          **_a('Mixed_5b', 192, 32), **_a('Mixed_5c', 256, 64), **_a('Mixed_5d', 288, 64), **_b('Mixed_6a', 288),
          **_c('Mixed_6b', 768, 128), **_c('Mixed_6c', 768, 160), **_c('Mixed_6d', 768, 160), **_c('Mixed_6e', 768, 192),
          **_d('Mixed_7a', 768), **_e('Mixed_7b', 1280), **_e('Mixed_7c', 2048)}


def state_dict(seed=0):
    """torchvision's keys, on the CPU: He-scaled normal conv weights, BN gamma and running_var uniform in [0.5, 1.5], small beta and
    running_mean (activations keep their size through the 47 layers of the deepest path), plus the keys a real file carries and the
    extractor ignores (fc.*, num_batches_tracked)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (ci, co, kh, kw) in SHAPES.items():
        sd[f'{name}.conv.weight'] = torch.randn(co, ci, kh, kw, generator=g) * (2.0 / (ci * kh * kw)) ** 0.5
        sd[f'{name}.bn.weight'] = torch.rand(co, generator=g) + 0.5
        sd[f'{name}.bn.bias'] = torch.randn(co, generator=g) * 0.05
        sd[f'{name}.bn.running_mean'] = torch.randn(co, generator=g) * 0.05
        sd[f'{name}.bn.running_var'] = torch.rand(co, generator=g) + 0.5
        sd[f'{name}.bn.num_batches_tracked'] = torch.tensor(0)
    sd['fc.weight'] = torch.zeros(1008, 2048)
    sd['fc.bias'] = torch.zeros(1008)
    return sd


class _Net:
    def __init__(self, sd, dtype):
        self.sd, self.dtype = sd, dtype

    def conv(self, name, x, stride=1, padding=0):
        p = lambda k: self.sd[f'{name}.{k}'].detach().cpu().to(self.dtype)
        y = F.conv2d(x, p('conv.weight'), None, stride=stride, padding=padding)
        y = F.batch_norm(y, p('bn.running_mean'), p('bn.running_var'), p('bn.weight'), p('bn.bias'), training=False, eps=EPS)
        return F.relu(y)

    def block_a(self, n, x):
        b1 = self.conv(f'{n}.branch1x1', x)
        b5 = self.conv(f'{n}.branch5x5_2', self.conv(f'{n}.branch5x5_1', x), padding=2)
        b3 = self.conv(f'{n}.branch3x3dbl_1', x)
        b3 = self.conv(f'{n}.branch3x3dbl_3', self.conv(f'{n}.branch3x3dbl_2', b3, padding=1), padding=1)
        bp = self.conv(f'{n}.branch_pool', F.avg_pool2d(x, 3, 1, 1, count_include_pad=False))
        return torch.cat([b1, b5, b3, bp], 1)

    def block_b(self, n, x):
        b3 = self.conv(f'{n}.branch3x3', x, stride=2)
        bd = self.conv(f'{n}.branch3x3dbl_2', self.conv(f'{n}.branch3x3dbl_1', x), padding=1)
        bd = self.conv(f'{n}.branch3x3dbl_3', bd, stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)

    def block_c(self, n, x):
        row, col = (0, 3), (3, 0)
        b1 = self.conv(f'{n}.branch1x1', x)
        b7 = self.conv(f'{n}.branch7x7_1', x)
        b7 = self.conv(f'{n}.branch7x7_3', self.conv(f'{n}.branch7x7_2', b7, padding=row), padding=col)
        bd = self.conv(f'{n}.branch7x7dbl_1', x)
        for j, pad in ((2, col), (3, row), (4, col), (5, row)):
            bd = self.conv(f'{n}.branch7x7dbl_{j}', bd, padding=pad)
        bp = self.conv(f'{n}.branch_pool', F.avg_pool2d(x, 3, 1, 1, count_include_pad=False))
        return torch.cat([b1, b7, bd, bp], 1)

    def block_d(self, n, x):
        b3 = self.conv(f'{n}.branch3x3_2', self.conv(f'{n}.branch3x3_1', x), stride=2)
        b7 = self.conv(f'{n}.branch7x7x3_1', x)
        b7 = self.conv(f'{n}.branch7x7x3_3', self.conv(f'{n}.branch7x7x3_2', b7, padding=(0, 3)), padding=(3, 0))
        b7 = self.conv(f'{n}.branch7x7x3_4', b7, stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)

    def block_e(self, n, x, max_pool):
        b1 = self.conv(f'{n}.branch1x1', x)
        b3 = self.conv(f'{n}.branch3x3_1', x)
        b3 = torch.cat([self.conv(f'{n}.branch3x3_2a', b3, padding=(0, 1)), self.conv(f'{n}.branch3x3_2b', b3, padding=(1, 0))], 1)
        bd = self.conv(f'{n}.branch3x3dbl_2', self.conv(f'{n}.branch3x3dbl_1', x), padding=1)
        bd = torch.cat([self.conv(f'{n}.branch3x3dbl_3a', bd, padding=(0, 1)), self.conv(f'{n}.branch3x3dbl_3b', bd, padding=(1, 0))], 1)
        pooled = F.max_pool2d(x, 3, 1, 1) if max_pool else F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)
        return torch.cat([b1, b3, bd, self.conv(f'{n}.branch_pool', pooled)], 1)

    def trunk(self, h):
        h = self.conv('Conv2d_1a_3x3', h, stride=2)
        h = self.conv('Conv2d_2b_3x3', self.conv('Conv2d_2a_3x3', h), padding=1)
        h = F.max_pool2d(h, 3, 2)
        h = self.conv('Conv2d_4a_3x3', self.conv('Conv2d_3b_1x1', h))
        h = F.max_pool2d(h, 3, 2)
        for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
            h = self.block_a(n, h)
        h = self.block_b('Mixed_6a', h)
        for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
            h = self.block_c(n, h)
        h = self.block_d('Mixed_7a', h)
        h = self.block_e('Mixed_7b', h, max_pool=False)
        return self.block_e('Mixed_7c', h, max_pool=True)


@torch.no_grad()
def mixed_7c(x, sd, dtype, resize_input=True):
    """the network up to the output of Mixed_7c on the CPU in `dtype`: [B,3,H,W] -> [B,2048,h,w]"""
    h = x.detach().cpu().to(dtype)
    if resize_input:
        h = F.interpolate(h, size=(299, 299), mode='bilinear', align_corners=False)
    return _Net(sd, dtype).trunk(h)


@torch.no_grad()
def pool3(x, sd, dtype, resize_input=True):
    """the whole extractor in `dtype` -> [B,2048] on the CPU"""
    return F.adaptive_avg_pool2d(mixed_7c(x, sd, dtype, resize_input), 1).flatten(1)

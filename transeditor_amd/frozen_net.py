"""What the frozen, forward-only evaluation networks share (lpips.PerceptualLoss, vgg_features.VGG16Features, dex.DEXScorer,
celeba_attr.CelebAAttributeScorer, inception_features.InceptionV3Features), each piece written once:

    load / resolve   : a local weight file -> state dict; "path or state_dict, not both"
    weight_bias      : one layer's (weight, bias) from a state dict, shapes checked, a ValueError naming the key otherwise
    check_images / no_gpu : the input checks every forward starts with, in the caller's own words
    FrozenConvs      : a module whose 3x3 convolutions are the frozen buffers w{i} / b{i}: the packed-weight cache and the launch
    VGGTrunk         : FrozenConvs + conv1_2 ... conv5_3 of a vgg16 with their ReLU passes and max-pools

Nothing is downloaded and every message names the class that the user called (`who`).
"""
import os

import torch

from . import _lib
from .op import modconv

POOL_AFTER = (1, 3, 6, 9)        # 2x2 max-pool after these convolutions of vgg16 (features[4, 9, 16, 23])


def load(path, what, who, note='', named=True):
    """the state dict in the file `path`; `what` names the kind of file, `note` is appended to the not-found message"""
    if path is None or not os.path.isfile(path):
        raise FileNotFoundError(f'{who}: {what} file not found: {path}{note}')
    sd = torch.load(path, map_location='cpu')
    if not isinstance(sd, dict):
        raise ValueError(f'{who}: {f"{what} file " if named else ""}{path} does not hold a state dict')
    return sd


def resolve(path, state_dict, who, what, arg='path', **load_args):
    """a constructor's (path, state_dict) pair -> (state dict, its name in messages); `arg` is the path argument's name"""
    if state_dict is None:
        return load(path, what, who, **load_args), path
    if path is not None:
        raise ValueError(f'{who}: give {arg} or state_dict, not both')
    if not isinstance(state_dict, dict):
        raise ValueError(f'{who}: state_dict must be a dict, got {type(state_dict).__name__}')
    return state_dict, 'state_dict'


def weight_bias(sd, kw, kb, shape, who, path, hint, want=None):
    """(weight, bias) of one layer as contiguous fp32.  `shape` is the weight's expected shape with None where the state dict decides;
    the bias must be [shape[0]].  `hint` (the layout, for the missing-key message) and `want` (the expected shapes, when they are not
    plain tuples) are the caller's words.  kb=None: the tensor `kw` alone, as it is stored."""
    keys = (kw,) if kb is None else (kw, kb)
    if any(k not in sd for k in keys):
        raise ValueError(f'{who}: {path} has no {" / ".join(keys)} ({hint})')
    w = sd[kw]
    ok = w.ndim == len(shape) and all(s is None or s == d for s, d in zip(shape, w.shape))
    if kb is None:
        if not ok:
            raise ValueError(f'{who}: {kw} is {tuple(w.shape)}, expected {want or tuple(shape)}')
        return w
    b = sd[kb]
    if not ok or b.ndim != 1 or b.shape[0] != w.shape[0]:
        raise ValueError(f'{who}: {kw} is {tuple(w.shape)} / bias {tuple(b.shape)}, expected {want or f"{tuple(shape)} / {(shape[0],)}"}')
    return w.detach().float().contiguous(), b.detach().float().contiguous()


def no_gpu(who):
    return f'{who} needs a GPU (the network runs on the gfx950 kernels only; there is no CPU path)'


def check_images(images, who, dims='[B,3,H,W]', square=False, pairs=False):
    """[B,3,H,W] (`pairs`: an even B; `square`: H == W), else a ValueError in `who`'s name"""
    if images.ndim != 4 or images.shape[1] != 3 or pairs and images.shape[0] % 2:
        raise ValueError(f'{who}: expected {dims} images, got {tuple(images.shape)}')
    if square and images.shape[3] != images.shape[2]:
        raise ValueError(f'{who}: the images must be square, got {images.shape[2]}x{images.shape[3]}')


def _relu_(y):
    """in-place ReLU as te_bias_act_f32 (act 3 = leaky ReLU, alpha 0, scale 1)"""
    _lib._launch('te_bias_act_f32', _lib._ptr(y), _lib._ptr(y), None, None, 3, 0, 0.0, 1.0, y.numel(), 1, 1)
    return y


class FrozenConvs:
    """mixin of a torch.nn.Module whose 3x3 convolutions run on the project's convolution (op/modconv.py planner) from the frozen
    buffers w{i} / b{i}"""

    def _freeze(self, convs, others=(), device='cuda', evaluate=True):
        """the end of a constructor: convs [(w, b)] -> w{i} / b{i}, others [(name, tensor)], eval mode, onto the GPU if there is one"""
        for i, (w, b) in enumerate(convs):
            self.register_buffer(f'w{i}', w)
            self.register_buffer(f'b{i}', b)
        for name, t in others:
            self.register_buffer(name, t)
        self._packs = {}
        if evaluate:
            self.eval()
        if device is not None and torch.cuda.is_available():
            self.to(device)

    def _w(self, i):
        return getattr(self, f'w{i}')

    def _packed(self, i, pack_kind):
        """packed layout of conv i (the network is frozen: kept as long as the buffer's version and address are unchanged)"""
        w = self._w(i)
        key = (i, pack_kind)
        ent = self._packs.get(key)
        if ent is None or ent[0] != (w._version, w.data_ptr()):
            ent = self._packs[key] = ((w._version, w.data_ptr()), _lib.conv_pack(w, pack_kind))
        return ent[1]

    def _conv(self, i, x, act=0):
        """conv i + bias + the epilogue's activation `act`"""
        w = self._w(i)
        B, _, H, W = x.shape
        pk, ck = modconv.fwd_kinds('3x3', B, w, H, W)
        return _lib.conv(x, self._packed(i, pk), ck, w.shape[0], H, W, bias=getattr(self, f'b{i}'), act=act)


class VGGTrunk(FrozenConvs):
    """conv1_2 ... conv5_3 of a frozen vgg16: shared by PerceptualLoss, VGG16Features and DEXScorer"""

    def _conv_fwd(self, i, x):
        return _relu_(self._conv(i, x))

    def _walk(self, stem, tap=None):
        """relu1_1 = stem() -> relu5_3 through conv1_2 ... conv5_3 and the four max-pools between them; tap(i, ReLU output of conv i)
        is called for i = 0 ... 12 as each appears.  The walk itself keeps no activation once the next layer has read it (which is
        why it makes relu1_1 itself: a caller's argument would live as long as the call)."""
        a = stem()
        for i in range(13):
            if i:
                if (i - 1) in POOL_AFTER:
                    a = _lib.maxpool2_fwd(a)
                a = self._conv_fwd(i, a)
            if tap is not None:
                tap(i, a)
        return a

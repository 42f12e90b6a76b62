"""Noise regulariser and noise normalisation of the projector (projector_optimization.py:21-49) over a whole list of noise maps,
one kernel launch per direction (csrc/noisereg.hip):

    loss = noise_regularize(noises)      # differentiable with respect to every map
    noise_normalize_(noises)             # in place: (n - mean) / std (unbiased), per map
"""
import torch
from torch.autograd import Function

from .. import _lib


class _NoiseRegularize(Function):
    @staticmethod
    def forward(ctx, *maps):
        maps = [m.contiguous() for m in maps]
        loss, ws = _lib.noise_reg_fwd(maps)
        ctx.save_for_backward(ws, *maps)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        ws, *maps = ctx.saved_tensors
        return tuple(_lib.noise_reg_bwd(g, ws, maps))


def noise_regularize(noises):
    """sum over maps and scales of mean(n * roll(n, 1, 3))^2 + mean(n * roll(n, 1, 2))^2 (a 0-dim tensor)"""
    return _NoiseRegularize.apply(*noises)


@torch.no_grad()
def noise_normalize_(noises):
    """noise.data.add_(-mean).div_(std) for every map, one launch"""
    for n in noises:
        if not n.is_contiguous():
            raise RuntimeError('te_hip: noise_normalize_ works in place on contiguous maps')
    _lib.noise_normalize_(list(noises))
    torch.autograd.graph.increment_version(list(noises))      # written through raw pointers

"""The identity loss of encoder training on the gfx950 kernels (the reference's pSp/criteria/id_loss.py:8-45 IDLoss, one of the three
losses of pSp/training/coach_new.py): how far is the reconstruction's ArcFace embedding from the target's?

    id_loss = IDLoss('model_ir_se50.pth')                           # the reference's own weight file
    loss, sim_improvement, id_logs = id_loss(y_hat, y, x)           # id_loss.py:23-45: images [B,3,S,S] in [-1, 1]
    loss.backward()                                                 # the gradient reaches y_hat and nothing else

    loss            = mean_i (1 - <e(y_hat_i), e(y_i)>)             a 0-dim tensor on the device
    sim_improvement = mean_i (<e(y_hat_i), e(y_i)> - <e(y_i), e(x_i)>)        a float
    id_logs[i]      = {'diff_target': <e(y_hat_i), e(y_i)>, 'diff_input': <e(y_hat_i), e(x_i)>, 'diff_views': <e(y_i), e(x_i)>}

e is arcface.ArcFaceID: y_hat runs through embed_grad (the hand-written backward pass of csrc/irse_bwd.hip), y and x through embed
(no_grad; the reference detaches y's features, and x's only enter the logs).  The paired dot products are te_rows_dot_f32; the
backward of <a_i, b_i> w.r.t. a_i is b_i times the incoming scalar.  The network is frozen: IDLoss has no trainable parameter.  The
constructor's arguments are ArcFaceID's.  Times and deviations: profiles/README.md, 'Identity loss'.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .arcface import BOX, POOL, ArcFaceID


class _RowsDot(Function):
    """d[i] = <a[i], b[i]> (te_rows_dot_f32); backward -> the gradient w.r.t. a only: gd[i] * b[i]"""

    @staticmethod
    def forward(ctx, a, b):
        ctx.b = b
        return _lib.rows_dot(a.contiguous(), b)

    @staticmethod
    @once_differentiable
    def backward(ctx, gd):
        return gd.view(-1, 1) * ctx.b, None


class IDLoss(torch.nn.Module):
    def __init__(self, path=None, state_dict=None, box=BOX, pool=POOL, units=None):
        super().__init__()
        self.facenet = ArcFaceID(path, state_dict=state_dict, box=box, pool=pool, units=units)

    def forward(self, y_hat, y, x):
        if not (tuple(y_hat.shape) == tuple(y.shape) == tuple(x.shape)):
            raise ValueError(f'IDLoss: y_hat, y and x must have one shape, got {tuple(y_hat.shape)}, {tuple(y.shape)}, {tuple(x.shape)}')
        x_feats = self.facenet.embed(x)
        y_feats = self.facenet.embed(y)
        y_hat_feats = self.facenet.embed_grad(y_hat)
        diff_target = _RowsDot.apply(y_hat_feats, y_feats)
        loss = (1 - diff_target).sum() / x.shape[0]                            # id_loss.py:40, :45
        with torch.no_grad():
            dots = torch.stack([diff_target.detach(), _lib.rows_dot(y_hat_feats.detach().contiguous(), x_feats),
                                _lib.rows_dot(y_feats, x_feats)]).double().cpu().tolist()       # one copy to the host for the logs
        id_logs = [{'diff_target': t, 'diff_input': i, 'diff_views': v} for t, i, v in zip(*dots)]
        sim_improvement = sum(d['diff_target'] - d['diff_views'] for d in id_logs) / x.shape[0]
        return loss, sim_improvement, id_logs

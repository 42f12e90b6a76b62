"""Plain-torch restatement of the identity loss (pSp/criteria/id_loss.py:23-45 IDLoss.forward on tests/arcface_restated.py's network) with
a gradient, for torch autograd in whatever dtype it is asked for, and the restated contracts of the backward kernels (te_hip.h, M9b).
Everything runs on the CPU; no reference code is read at run time."""
import torch
import torch.nn.functional as F

import arcface_restated as R

# what tools/id_loss_golden.py records in tests/golden/id_loss_ref.npz: the weights and y_hat are arcface_restated.GOLDEN's
GOLDEN = dict(R.GOLDEN, y_seed=202, x_seed=303)


def embed(x, sd, dtype, units=R.UNITS50, box=R.BOX, pool=R.POOL, gates=None, pres=None):
    """arcface_restated.embed without the detach in front of the crop: differentiable w.r.t. x.  pres: a list that receives every
    PReLU's input"""
    P = R._params(sd, dtype)
    y0, y1, x0, x1 = box
    h = R._bn(F.conv2d(F.adaptive_avg_pool2d(x.to(dtype)[:, :, y0:y1, x0:x1], (pool, pool)), P['input_layer.0.weight'], None, 1, 1), P, 'input_layer.1')
    if pres is not None:
        pres.append(h.detach().flatten())
    h = F.prelu(h, P['input_layer.2.weight'])
    for n, (_, _, stride) in enumerate(units):
        p = f'body.{n}'
        if pres is not None:
            pres.append(F.conv2d(R._bn(h, P, f'{p}.res_layer.0'), P[f'{p}.res_layer.1.weight'], None, 1, 1).detach().flatten())
        h = R._finish(h, R._res(h, P, p, stride), P, p, stride, gates)
    h = R._bn(h, P, 'output_layer.0').flatten(1)
    h = R._bn(F.linear(h, P['output_layer.3.weight'], P['output_layer.3.bias']), P, 'output_layer.4')
    return h / torch.norm(h, 2, 1, True)


def id_loss(y_hat, y, x, sd, dtype, units=R.UNITS50, box=R.BOX, pool=R.POOL, gates=None, pres=None):
    """id_loss.py:23-45 -> (loss, sim_improvement, id_logs, d loss / d y_hat); y_hat, y, x on the CPU"""
    y_hat = y_hat.detach().to(dtype).requires_grad_(True)
    with torch.no_grad():
        ey, ex = (embed(t, sd, dtype, units, box, pool) for t in (y, x))
    eh = embed(y_hat, sd, dtype, units, box, pool, gates, pres)
    target, inp, views = (eh * ey).sum(1), (eh * ex).sum(1), (ey * ex).sum(1)
    loss = (1 - target).mean()
    grad, = torch.autograd.grad(loss, y_hat)
    logs = [{'diff_target': float(t), 'diff_input': float(i), 'diff_views': float(v)} for t, i, v in zip(target.detach(), inp.detach(), views)]
    return loss.detach(), float((target.detach() - views).mean()), logs, grad


# ------------------------------------------------------------------------------------------------------------ restated contracts
def dgrad_acc(g, w, x_hw, stride, pad):
    """acc of te_conv2d_dgrad_f32 from the forward's OWN weight w [Co,Ci,kh,kw]: torch's transposed convolution, in g's dtype"""
    (H, W), (kh, kw) = x_hw, w.shape[2:]
    op = (H - ((g.shape[2] - 1) * stride - 2 * pad[0] + kh), W - ((g.shape[3] - 1) * stride - 2 * pad[1] + kw))
    return F.conv_transpose2d(g, w.to(g.dtype), None, stride, pad, op)


def dgrad_acc_from_layout(g, wt, x_shape, kernel, stride, pad):
    """acc of te_conv2d_dgrad_f32 from the PREPARED weight, as te_hip.h words it: per output phase (ry, rx) a dense stride-1 correlation
    of g with the block [Ci, Co, ny, nx], row y = s yy + r reading g rows yy - pad' + j, pad' = n - 1 - (r + p - k0) / s"""
    B, Ci, H, W = x_shape
    Co = g.shape[1]
    acc = torch.zeros(B, Ci, H, W, dtype=g.dtype)
    at = 0

    def axis(r, k, p):
        k0 = (r + p) % stride
        n = (k - k0 + stride - 1) // stride if k0 < k else 0
        return n, n - 1 - (r + p - k0) // stride
    for ry in range(stride):
        for rx in range(stride):
            (ny, py), (nx, px) = axis(ry, kernel[0], pad[0]), axis(rx, kernel[1], pad[1])
            Hp, Wp = len(range(ry, H, stride)), len(range(rx, W, stride))
            blk = wt[at:at + Ci * Co * ny * nx].view(Ci, Co, ny, nx).to(g.dtype)
            at += blk.numel()
            if ny == 0 or nx == 0 or Hp == 0 or Wp == 0:
                continue
            assert py >= 0 and px >= 0                                          # (true of every layer of the network)
            gp = F.pad(g, (px, Wp + nx, py, Hp + ny))                           # zeros wherever the phase looks past g
            acc[:, :, ry::stride, rx::stride] = F.conv2d(gp, blk)[:, :, :Hp, :Wp]
    assert at == wt.numel()
    return acc


def dgrad_epilogue(acc, pre=None, slope=None, in_scale=None, add=None, add_stride=1):
    if pre is not None:
        return torch.where(pre.to(acc.dtype) > 0, acc, acc * slope.to(acc.dtype).view(1, -1, 1, 1))
    if in_scale is not None:
        acc = acc * in_scale.to(acc.dtype).view(1, -1, 1, 1)
    if add is not None:
        acc = acc.clone()
        acc[:, :, ::add_stride, ::add_stride] += add.to(acc.dtype)
    return acc


def se_bwd(gout, r, gate, pooled, w1, w2):
    """te_se_bwd_f32 restated in gout's dtype"""
    dt = gout.dtype
    r, gate, pooled, w1, w2 = (t.to(dt) for t in (r, gate, pooled, w1, w2))
    ggate = (gout * r).sum((2, 3))
    gh = ((ggate * gate * (1 - gate)) @ w2) * (pooled @ w1.t() > 0)
    gmean = (gh @ w1) / (gout.shape[2] * gout.shape[3])
    return gout * gate[:, :, None, None] + gmean[:, :, None, None]


def stem_bwd(g, w, pre, slope, img_shape, box, pool):
    """te_id_stem_bwd_f32 restated from the stem's own weight w [Co,3,3,3], in g's dtype: PReLU', the transposed convolution, then the
    adjoint of the crop and AdaptiveAvgPool2d (torch autograd of the pool: it is linear)"""
    dt = g.dtype
    gp = dgrad_acc(dgrad_epilogue(g, pre, slope), w, (pool, pool), 1, (1, 1))
    img = torch.zeros(img_shape, dtype=dt, requires_grad=True)
    y0, y1, x0, x1 = box
    return torch.autograd.grad(F.adaptive_avg_pool2d(img[:, :, y0:y1, x0:x1], (pool, pool)), img, gp)[0]


def rows_unit_bwd(ge, e, a):
    dt = ge.dtype
    e, a = e.to(dt), a.to(dt)
    return (ge - e * (e * ge).sum(1, keepdim=True)) / a.norm(dim=1, keepdim=True)

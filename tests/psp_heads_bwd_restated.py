"""The backward pass of the pSp encoder's head stage, restated for the tests of transeditor_amd.psp_heads_train: plain torch on the CPU.

The truth is tests/psp_encoder_restated.py's graph (F.conv2d / F.interpolate / F.linear, EqualLinear's scale applied as the reference
applies it) from the features c1, c2, c3 on, under torch autograd, in whatever dtype it is asked for.  `stage` is that graph with one
switch, the project's pinning convention (tests/pinning.py): with `masks` given every leaky ReLU becomes x * where(mask, 1, slope), so
that the library's own branch decisions can be pinned and what remains between two backward passes is arithmetic; without, it is
F.leaky_relu and the masks it took (pre-activation > 0) are recorded.  A helper, not a test.
"""
import math

import torch
import torch.nn.functional as F

import arcface_restated as R
import psp_encoder_restated as P

LRELU = P.LRELU


def head_prefixes(sd):
    Ns, Np = P._heads(sd, 'styles'), P._heads(sd, 'spatials')
    return [f'styles.{j}' for j in range(Ns)] + [f'spatials.{j}' for j in range(Np)]


def trained_keys(sd):
    """every key of the head stage: what TrainableHeads trains"""
    keys = []
    for prefix in head_prefixes(sd):
        for k in range(P._depth(sd, prefix)):
            keys += [f'{prefix}.convs.{2 * k}.weight', f'{prefix}.convs.{2 * k}.bias']
        keys += [f'{prefix}.linear.weight', f'{prefix}.linear.bias']
    return keys + ['latlayer1.weight', 'latlayer1.bias', 'latlayer2.weight', 'latlayer2.bias', 'adjust_style.weight', 'adjust_style.bias']


def _act(x, key, masks, taken):
    if masks is None:
        taken[key] = x.detach() > 0
        return F.leaky_relu(x, LRELU)
    m = masks[key]
    assert m.shape == x.shape and m.dtype == torch.bool, key
    one = torch.ones((), dtype=x.dtype)
    return x * torch.where(m, one, one * LRELU)


def stage(c1, c2, c3, Pm, masks=None):
    """the head stage on the parameters Pm {reference key: tensor} -> (z_out [B,D,T], p_out [B,D,Np], the masks taken {(prefix, k): bool
    [B,D,h,w]} (those given, where given))"""
    d0 = P._depth(Pm, 'spatials.0')
    Ns = P._heads(Pm, 'styles')
    taken = {}
    feat = {d0: c3}
    depths = {prefix: P._depth(Pm, prefix) for prefix in head_prefixes(Pm)}
    if any(d > d0 for d in depths.values()):
        feat[d0 + 1] = P.upsample_add(c3, F.conv2d(c2, Pm['latlayer1.weight'], Pm['latlayer1.bias']))
    if any(d > d0 + 1 for d in depths.values()):
        feat[d0 + 2] = P.upsample_add(feat[d0 + 1], F.conv2d(c1, Pm['latlayer2.weight'], Pm['latlayer2.bias']))
    lat = []
    for prefix, d in depths.items():
        x = feat[d]
        D = Pm[f'{prefix}.linear.weight'].shape[0]
        for k in range(d):
            x = _act(F.conv2d(x, Pm[f'{prefix}.convs.{2 * k}.weight'], Pm[f'{prefix}.convs.{2 * k}.bias'], 2, 1), (prefix, k), masks, taken)
        lat.append(F.linear(x.reshape(-1, D), Pm[f'{prefix}.linear.weight'] * (1 / math.sqrt(D)), Pm[f'{prefix}.linear.bias']))
    z_lat, p_lat = torch.stack(lat[:Ns], 1), torch.stack(lat[Ns:], 1)
    z_out = F.linear(z_lat.permute(0, 2, 1), Pm['adjust_style.weight'] * (1 / math.sqrt(Ns)), Pm['adjust_style.bias'])
    return z_out, p_lat.permute(0, 2, 1), (taken if masks is None else masks)


def gradients(c, sd, gz, gp, dtype, masks=None):
    """autograd through `stage` in `dtype`: c = (c1, c2, c3), cotangents gz, gp -> dict(z, p, masks, grads {reference key or 'c1' / 'c2' /
    'c3': gradient})"""
    keys = trained_keys(sd)
    Pm = {k: sd[k].detach().cpu().to(dtype).clone().requires_grad_(True) for k in keys}
    cs = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in c]
    z, p, taken = stage(*cs, Pm, masks)
    leaves = [Pm[k] for k in keys] + cs
    got = torch.autograd.grad([z, p], leaves, [gz.cpu().to(dtype), gp.cpu().to(dtype)])
    grads = dict(zip(keys + ['c1', 'c2', 'c3'], got))
    return dict(z=z.detach(), p=p.detach(), masks=taken, grads=grads)


def features(x, sd, dtype, units, taps):
    """the backbone's features (c1, c2, c3) in `dtype`"""
    return P.features(x, R._params(sd, dtype), units, taps)


def library_masks(bufs, program, launch_heads, D):
    """the branch decisions the library took, from its kept level buffers: head g of the launch that wrote channels [c0 * D, ...) of
    bufs[dst] -> {(prefix, k): bool [B,D,h,w] on the CPU}"""
    out = {}
    for (_, _, dst, _, c0, _), heads in zip(program, launch_heads):
        for g, (kind, i, k) in enumerate(heads):
            out[f'{kind}.{i}', k] = (bufs[dst][:, (c0 + g) * D:(c0 + g + 1) * D] > 0).cpu()
    return out


def ranger_first_step(p, g, lr, beta1=0.95):
    """Ranger's first step on one tensor in p's dtype (tests/ranger_restated.py's run at step 1: unrectified, no lookahead yet, no weight
    decay): the gradient centralised over every dim but the first where it has more than one"""
    g = g.to(p.dtype)
    if g.dim() > 1:
        rows = g.reshape(g.shape[0], -1)
        g = (rows - rows.mean(dim=1, keepdim=True)).reshape(g.shape)
    exp_avg = (1 - beta1) * g
    return p + (-(1.0 / (1 - beta1)) * lr) * exp_avg

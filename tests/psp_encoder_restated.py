"""Plain-torch restatement of the dual-space pSp encoder (pSp/models/encoders/psp_encoders_new.py:11-32 GradualStyleBlock and :35-140
GradualStyleEncoder.forward, with the units of helpers.py:76-120; no reference code is read at run time):

    conv 3x3 pad 1 (no bias) -> batch norm -> PReLU -> the units (arcface_restated), c1 / c2 / c3 tapped after units taps[0..2]
    p2 = bilinear(c3 -> c2's size, align_corners=True) + conv1x1(c2);   p1 = bilinear(p2 -> c1's size) + conv1x1(c1)
    head = [conv 3x3 stride 2 pad 1 -> LeakyReLU(0.01)] * depth -> view(-1, D) -> linear(w / sqrt(D), b)
    z_out = linear over the head axis of stack(styles)(w / sqrt(Ns), b) -> [B, D, T];   p_out = stack(spatials) -> [B, D, Np]

indexed by the reference's state dict keys, with the batch norms NOT folded, in whatever dtype it is asked for; a synthetic state dict
for any small geometry filled from a seed.  A head sits on the feature its depth names: the spatials' depth d on c3, d + 1 on p2, d + 2 on
p1 (the reference's coarse_ind / middle_ind say the same for its own geometry).  Everything runs on the CPU.
"""
import math

import torch
import torch.nn.functional as F

import arcface_restated as R

UNITS50 = R.UNITS50
TAPS = (6, 20, 23)
STYLES = (3, 4, 7)               # coarse, middle, fine (coarse_ind = 3, middle_ind = 7, style_count = 14)
LRELU = 0.01

# what tools/psp_encoder_golden.py records in tests/golden/psp_encoder_ref.npz
GOLDEN = dict(seed=2, image_seed=103, B=1, S=256)
# the small geometry of the end-to-end GPU tests
SMALL = dict(units=((8, 16, 2), (16, 32, 2), (32, 64, 2)), taps=(0, 1, 2), D=64, styles=(2, 1, 2), spatials=4, tokens=4, depth=2, S=32)


def _heads(P, kind):
    n = 0
    while f'{kind}.{n}.convs.0.weight' in P:
        n += 1
    return n


def _depth(P, prefix):
    d = 0
    while f'{prefix}.convs.{2 * d}.weight' in P:
        d += 1
    return d


def features(x, P, units, taps):
    """-> (c1, c2, c3) in P's dtype"""
    dtype = P['input_layer.0.weight'].dtype
    h = F.prelu(R._bn(F.conv2d(x.detach().cpu().to(dtype), P['input_layer.0.weight'], None, 1, 1), P, 'input_layer.1'), P['input_layer.2.weight'])
    c = []
    for n, (_, _, stride) in enumerate(units):
        h = R._finish(h, R._res(h, P, f'body.{n}', stride), P, f'body.{n}', stride)
        if n in taps:
            c.append(h)
        if n == taps[2]:
            break
    return c


def upsample_add(x, y):
    return F.interpolate(x, size=y.shape[2:], mode='bilinear', align_corners=True) + y


def head(x, P, prefix):
    D = P[f'{prefix}.linear.weight'].shape[0]
    for k in range(_depth(P, prefix)):
        x = F.leaky_relu(F.conv2d(x, P[f'{prefix}.convs.{2 * k}.weight'], P[f'{prefix}.convs.{2 * k}.bias'], 2, 1), LRELU)
    return F.linear(x.reshape(-1, D), P[f'{prefix}.linear.weight'] * (1 / math.sqrt(D)), P[f'{prefix}.linear.bias'])


def encode(x, sd, dtype, units=UNITS50, taps=TAPS, want_latents=False):
    """(z_out [B,D,T], p_out [B,D,Np]) in `dtype`; want_latents: -> also the stacked head outputs [B, Ns + Np, D]"""
    P = R._params(sd, dtype)
    c1, c2, c3 = features(x, P, units, taps)
    d0 = _depth(P, 'spatials.0')
    Ns, Np = _heads(P, 'styles'), _heads(P, 'spatials')
    depths = [_depth(P, f'styles.{j}') for j in range(Ns)]
    feat = {d0: c3}
    if any(d > d0 for d in depths):
        feat[d0 + 1] = upsample_add(c3, F.conv2d(c2, P['latlayer1.weight'], P['latlayer1.bias']))
    if any(d > d0 + 1 for d in depths):
        feat[d0 + 2] = upsample_add(feat[d0 + 1], F.conv2d(c1, P['latlayer2.weight'], P['latlayer2.bias']))
    z_lat = torch.stack([head(feat[depths[j]], P, f'styles.{j}') for j in range(Ns)], 1)
    p_lat = torch.stack([head(c3, P, f'spatials.{j}') for j in range(Np)], 1)
    z_out = F.linear(z_lat.permute(0, 2, 1), P['adjust_style.weight'] * (1 / math.sqrt(Ns)), P['adjust_style.bias'])
    out = (z_out, p_lat.permute(0, 2, 1))
    return (*out, torch.cat([z_lat, p_lat], 1)) if want_latents else out


def state_dict(seed, units=UNITS50, taps=TAPS, images=None, D=512, styles=STYLES, spatials=16, tokens=16, depth=4, se=True, fc2_scale=None,
               reduction=16, want_scales=False):
    """GradualStyleEncoder's key names, on the CPU.  input_layer and body are arcface_restated.state_dict's (batch norm statistics away
    from the identity, PReLU slopes partly negative, the SE fc2 calibrated on `images` in fp64 or scaled by the recorded `fc2_scale`):
    the stem sees the full image, so the calibration walks it with the whole image as the box.  The heads are drawn from a second
    generator (seed + 7919): convolutions He-scaled (gain 2, so that the codes do not collapse through up to `depth + 2` leaky
    layers), their biases 0.1 * randn, EqualLinear weights randn (the layer scales them itself) with biases 0.1 * randn."""
    S = None if images is None else images.shape[2]
    body = R.state_dict(seed, units=list(units), images=images, box=None if S is None else (0, S, 0, S), pool=S or R.POOL, se=se, dim=1,
                        fc2_scale=fc2_scale, reduction=reduction, want_scales=True)
    sd = {k: v for k, v in body[0].items() if not k.startswith('output_layer')}
    g = torch.Generator().manual_seed(seed + 7919)
    c1c, c2c, Cf = (units[t][1] for t in taps)

    def conv(k, co, ci, ks):
        sd[f'{k}.weight'] = torch.randn(co, ci, ks, ks, generator=g) * (2.0 / (ci * ks * ks)) ** 0.5
        sd[f'{k}.bias'] = torch.randn(co, generator=g) * 0.1

    def linear(k, co, ci):
        sd[f'{k}.weight'] = torch.randn(co, ci, generator=g)
        sd[f'{k}.bias'] = torch.randn(co, generator=g) * 0.1

    def block(prefix, d):
        for k in range(d):
            conv(f'{prefix}.convs.{2 * k}', D, Cf if k == 0 else D, 3)
        linear(f'{prefix}.linear', D, D)
    j = 0
    for k, n in enumerate(styles):
        for _ in range(n):
            block(f'styles.{j}', depth + k)
            j += 1
    for i in range(spatials):
        block(f'spatials.{i}', depth)
    conv('latlayer1', Cf, c2c, 1)
    conv('latlayer2', Cf, c1c, 1)
    linear('adjust_style', tokens, sum(styles))
    return (sd, body[1]) if want_scales else sd


def checkpoint(sd, plus=True, averages=True, seed=5):
    """the layout pSp/training/coach_new.py:358-371 writes: encoder.* (and a decoder.* key) under state_dict, opts, the averages"""
    D, T = sd['styles.0.linear.weight'].shape[0], sd['adjust_style.weight'].shape[0]
    Np = _heads(sd, 'spatials')
    g = torch.Generator().manual_seed(seed)
    ck = {'state_dict': {**{f'encoder.{k}': v for k, v in sd.items()}, 'decoder.style.0.weight': torch.zeros(2, 2)},
          'opts': {'from_plus_space': plus, 'start_from_latent_avg': averages, 'encoder_type': 'GradualStyleEncoder', 'output_size': 256}}
    if averages:
        names = ('z_plus_latent_avg', 'p_plus_latent_avg') if plus else ('z_latent_avg', 'p_latent_avg')
        ck[names[0]] = torch.randn(1, D, T, generator=g)
        ck[names[1]] = torch.randn(1, D, Np, generator=g)
    return ck


def small_state_dict(seed, images=None, se=True, **kw):
    G = SMALL
    return state_dict(seed, units=G['units'], taps=G['taps'], images=images, D=G['D'], styles=G['styles'], spatials=G['spatials'],
                      tokens=G['tokens'], depth=G['depth'], se=se, reduction=4, **kw)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())

"""Plain-torch restatement of the ArcFace identity network of edit evaluation (pSp/criteria/id_loss.py:17-21 extract_feats and
pSp/models/encoders/model_irse.py:45-49 Backbone.forward with helpers.py:16-120; no reference code is read at run time):

    x[:, :, 35:223, 32:220] -> AdaptiveAvgPool2d((112, 112)) -> conv 3x3 pad 1 (no bias) -> batch norm -> PReLU
    -> per unit:  shortcut = x[:, :, ::s, ::s]  (in == depth)  or  batch norm(conv 1x1 stride s)
                  res = batch norm -> conv 3x3 pad 1 -> PReLU -> conv 3x3 stride s pad 1 -> batch norm
                        [-> * sigmoid(fc2(relu(fc1(mean over the plane))))]           (mode 'ir_se')
                  res + shortcut
    -> batch norm -> flatten -> Linear -> BatchNorm1d -> x / ||x||_2

indexed by the reference's state dict keys, with the batch norms NOT folded (F.batch_norm, eps 1e-5, eval), in whatever dtype it is
asked for; a synthetic state dict filled from a seed; test images.  Everything runs on the CPU.

A state dict does not hold the strides, so the restatement takes the unit list [(in, depth, stride)] as an argument; UNITS50 is
get_blocks(50).
"""
import math

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')
BOX = (35, 223, 32, 220)
POOL = 112
UNITS50 = [u for cin, depth, n in ((64, 64, 3), (64, 128, 4), (128, 256, 14), (256, 512, 3)) for u in [(cin, depth, 2)] + [(depth, depth, 1)] * (n - 1)]
GATE_SPREAD = 2.5                # the standard deviation the calibrated SE logits have

# what tools/arcface_golden.py records in tests/golden/arcface_ref.npz
GOLDEN = dict(seed=1, image_seed=101, B=2, S=256)


def images(seed, B, S):
    """tanh of bilinearly upsampled 4 x 4 noise * 1.2 + 0.3 * randn: smooth structure that differs per image (the adaptive average
    would flatten plain noise), inside (-1, 1)"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, 3, 4, 4, generator=g)
    return torch.tanh(F.interpolate(low, size=(S, S), mode='bilinear', align_corners=False) * 1.2 + 0.3 * torch.randn(B, 3, S, S, generator=g))


def out_side(pool, units):
    h = pool
    for _, _, s in units:
        h = (h - 1) // s + 1
    return h


def extract(x, box=BOX, pool=POOL, dtype=torch.float32):
    """id_loss.py:18-19: the crop and the adaptive average, in `dtype`"""
    y0, y1, x0, x1 = box
    return F.adaptive_avg_pool2d(x.detach().cpu().to(dtype)[:, :, y0:y1, x0:x1], (pool, pool))


def _bn(t, P, k):
    return F.batch_norm(t, P[f'{k}.running_mean'], P[f'{k}.running_var'], P.get(f'{k}.weight'), P.get(f'{k}.bias'), False, 0.0, BN_EPS)


def _stem(x, P, box, pool, dtype):
    return F.prelu(_bn(F.conv2d(extract(x, box, pool, dtype), P['input_layer.0.weight'], None, 1, 1), P, 'input_layer.1'), P['input_layer.2.weight'])


def _res(h, P, p, stride):
    """res_layer.0 ... res_layer.4: everything of the residual branch before the squeeze-and-excitation"""
    r = F.prelu(F.conv2d(_bn(h, P, f'{p}.res_layer.0'), P[f'{p}.res_layer.1.weight'], None, 1, 1), P[f'{p}.res_layer.2.weight'])
    return _bn(F.conv2d(r, P[f'{p}.res_layer.3.weight'], None, stride, 1), P, f'{p}.res_layer.4')


def _hidden(r, P, p):
    return F.relu(F.conv2d(r.mean((2, 3), keepdim=True), P[f'{p}.res_layer.5.fc1.weight']))


def _finish(h, r, P, p, stride, gates=None):
    if f'{p}.res_layer.5.fc1.weight' in P:
        g = torch.sigmoid(F.conv2d(_hidden(r, P, p), P[f'{p}.res_layer.5.fc2.weight']))
        if gates is not None:
            gates.append(g.flatten())
        r = r * g
    if f'{p}.shortcut_layer.0.weight' in P:
        sc = _bn(F.conv2d(h, P[f'{p}.shortcut_layer.0.weight'], None, stride, 0), P, f'{p}.shortcut_layer.1')
    else:
        sc = h[:, :, ::stride, ::stride]                                       # MaxPool2d(1, stride)
    return r + sc


def _params(sd, dtype):
    return {k: v.cpu().to(dtype) for k, v in sd.items() if v.is_floating_point()}


def embed(x, sd, dtype, units=UNITS50, box=BOX, pool=POOL, gates=None):
    """[B,D] unit rows in `dtype`; gates: a list that receives every unit's SE gates"""
    P = _params(sd, dtype)
    h = _stem(x, P, box, pool, dtype)
    for n, (_, _, stride) in enumerate(units):
        h = _finish(h, _res(h, P, f'body.{n}', stride), P, f'body.{n}', stride, gates)
    h = _bn(h, P, 'output_layer.0').flatten(1)
    h = _bn(F.linear(h, P['output_layer.3.weight'], P['output_layer.3.bias']), P, 'output_layer.4')
    return h / torch.norm(h, 2, 1, True)                                       # helpers.py:16-19


def state_dict(seed, units=UNITS50, images=None, box=BOX, pool=POOL, se=True, dim=512, affine=True, fc2_scale=None, reduction=16,
               want_scales=False):
    """Backbone's key names from torch.Generator().manual_seed(seed), on the CPU: normal convolutions of gain 1 (He-scaled for the
    stem), batch norms with gamma and running_var uniform in [0.5, 1.5] and beta and running_mean 0.3 * randn (so that folding the
    leading batch norm's shift into a bias would move border outputs by a few tenths), PReLU slopes 0.25 + 0.3 * randn per channel
    (a fifth of them negative), one num_batches_tracked per batch norm, SE with depth // reduction hidden units (at least 2).
    A drawn fc2 leaves every gate near 0.5, where a wrong gate would hardly show.  So, given the test `images`, each unit's fc2 is
    CALIBRATED on them in fp64 as the network is walked: scaled so that the unit's logits have a standard deviation of GATE_SPREAD,
    the factor rounded to a quarter power of two (so that the last bits of the fp64 walk do not enter the weights).  `fc2_scale`
    (one factor per unit) applies recorded factors instead of walking; want_scales: -> (state dict, the factors)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(k, co, ci, ks, gain=1.0):
        sd[f'{k}.weight'] = torch.randn(co, ci, ks, ks, generator=g) * (gain / (ci * ks * ks)) ** 0.5

    def bn(k, c, with_affine=True):
        if with_affine:
            sd[f'{k}.weight'] = torch.rand(c, generator=g) + 0.5
            sd[f'{k}.bias'] = torch.randn(c, generator=g) * 0.3
        sd[f'{k}.running_mean'] = torch.randn(c, generator=g) * 0.3
        sd[f'{k}.running_var'] = torch.rand(c, generator=g) + 0.5
        sd[f'{k}.num_batches_tracked'] = torch.tensor(0, dtype=torch.long)

    def prelu(k, c):
        sd[f'{k}.weight'] = 0.25 + 0.3 * torch.randn(c, generator=g)
    c0 = units[0][0]
    conv('input_layer.0', c0, 3, 3, gain=2.0)
    bn('input_layer.1', c0)
    prelu('input_layer.2', c0)
    for n, (cin, depth, stride) in enumerate(units):
        p = f'body.{n}'
        if cin != depth:
            conv(f'{p}.shortcut_layer.0', depth, cin, 1)
            bn(f'{p}.shortcut_layer.1', depth)
        bn(f'{p}.res_layer.0', cin)
        conv(f'{p}.res_layer.1', depth, cin, 3)
        prelu(f'{p}.res_layer.2', depth)
        conv(f'{p}.res_layer.3', depth, depth, 3)
        bn(f'{p}.res_layer.4', depth)
        if se:
            r = max(depth // reduction, 2)
            sd[f'{p}.res_layer.5.fc1.weight'] = torch.randn(r, depth, 1, 1, generator=g) * (2.0 / depth) ** 0.5
            sd[f'{p}.res_layer.5.fc2.weight'] = torch.randn(depth, r, 1, 1, generator=g) * (1.0 / r) ** 0.5
    cl, h = units[-1][1], out_side(pool, units)
    bn('output_layer.0', cl)
    sd['output_layer.3.weight'] = torch.randn(dim, cl * h * h, generator=g) * (1.0 / (cl * h * h)) ** 0.5
    sd['output_layer.3.bias'] = torch.randn(dim, generator=g) * 0.1
    bn('output_layer.4', dim, with_affine=affine)
    scales = []
    if se and fc2_scale is not None:
        scales = [float(s) for s in fc2_scale]
        for n, s in enumerate(scales):
            sd[f'body.{n}.res_layer.5.fc2.weight'] = sd[f'body.{n}.res_layer.5.fc2.weight'] * s
    elif se and images is not None:
        P = _params(sd, torch.float64)
        hh = _stem(images, P, box, pool, torch.float64)
        for n, (_, _, stride) in enumerate(units):
            p = f'body.{n}'
            r = _res(hh, P, p, stride)
            lg = F.conv2d(_hidden(r, P, p), P[f'{p}.res_layer.5.fc2.weight'])
            assert float(lg.std()) > 0, f'{p}: every hidden unit of the drawn SE is dead on these images; use a smaller reduction'
            s = 2.0 ** (round(4 * math.log2(GATE_SPREAD / float(lg.std()))) / 4)
            scales.append(s)
            sd[f'{p}.res_layer.5.fc2.weight'] = sd[f'{p}.res_layer.5.fc2.weight'] * s
            P[f'{p}.res_layer.5.fc2.weight'] = sd[f'{p}.res_layer.5.fc2.weight'].double()
            hh = _finish(hh, r, P, p, stride)
    return (sd, scales) if want_scales else sd

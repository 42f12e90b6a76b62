"""Plain-torch restatement of the DEX age / gender scorer of attribute editing (our_interfaceGAN/ffhq_utils/dex/models.py:27-69, api.py:42-65,
called from edit_all_noinversion_ffhq.py:113-131; no reference code is read at run time):

    RGB [-1, 1] -> BGR -> clamp, +1, /2, *255, round -> centre crop -> 13 x (conv3x3 + ReLU) with five 2x2 max-pools -> flatten
    -> Linear, ReLU, Linear, ReLU -> Linear -> softmax -> sum_c (c + 1) p_c (age) or p_0 (gender)

indexed by the reference's state dict keys, in whatever dtype it is asked for (the preprocessing always runs in torch's own fp32, as the
reference runs it), and a synthetic state dict filled from a seed.  Everything runs on the CPU.

The geometry is read from the shapes, as transeditor_amd.dex reads it: fc1 has 512 * pool^2 inputs and the crop is 32 * pool pixels.
The real files have pool 7 (a 224 px crop), hidden widths 4096 and 101 or 2 classes; the tests also use smaller networks.
"""
import math

import torch
import torch.nn.functional as F

CHANNELS = (64, 128, 256, 512, 512)          # per block
CONVS = (2, 2, 3, 3, 3)


def conv_keys():
    """[(key prefix, Ci, Co)] * 13 in network order"""
    out, ci = [], 3
    for blk, (co, n) in enumerate(zip(CHANNELS, CONVS)):
        for j in range(1, n + 1):
            out.append((f'conv.{blk}.conv{j}', ci, co))
            ci = co
    return out


# what tools/dex_golden.py records in tests/golden/dex_ref.npz: the first seed (images: seed + 100) whose fp64 outputs meet the tests'
# non-degeneracy conditions for 101 and for 2 classes
GOLDEN = dict(seed=1, image_seed=101, B=2, S=256)


def state_dict(seed, pool=7, hidden=(4096, 4096), classes=101):
    """The reference's key names from torch.Generator().manual_seed(seed), on the CPU: He-scaled normal weights, biases 0.05 * randn;
    conv1_1's weight divided by 128 (its input is 0 ... 255, not [-1, 1]); cls with gain 1 (std sqrt(1 / K)), so that the logits
    spread by about one and the softmax neither saturates nor flattens.  cls is drawn last: a tuple of class counts gives one state
    dict per count, each what the single count would give, all sharing the tensors before cls."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, ci, co in conv_keys():
        sd[f'{key}.weight'] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        sd[f'{key}.bias'] = torch.randn(co, generator=g) * 0.05
    sd['conv.0.conv1.weight'] /= 128
    k = 512 * pool * pool
    for name, j in zip(('fc1.0', 'fc2.0'), hidden):
        sd[f'{name}.weight'] = torch.randn(j, k, generator=g) * (2.0 / k) ** 0.5
        sd[f'{name}.bias'] = torch.randn(j, generator=g) * 0.05
        k = j
    state, out = g.get_state(), []
    for c in (classes if isinstance(classes, tuple) else (classes,)):
        g.set_state(state)
        one = dict(sd)
        one['cls.weight'] = torch.randn(c, k, generator=g) * (1.0 / k) ** 0.5
        one['cls.bias'] = torch.randn(c, generator=g) * 0.05
        out.append(one)
    return out if isinstance(classes, tuple) else out[0]


def images(seed, B, S):
    """0.6 * randn: about a tenth of the pixels lie outside [-1, 1], so the clamp is live"""
    return 0.6 * torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(seed))


def crop_of(sd):
    return 32 * math.isqrt(sd['fc1.0.weight'].shape[1] // 512)


def preprocess(x, crop):
    """edit_all_noinversion_ffhq.py:113-116 and the centre crop of api.py:62, in torch's fp32: [B,3,H,W] RGB -> [B,3,crop,crop] BGR"""
    x = x.detach().cpu().float()
    v = torch.stack([x[:, 2], x[:, 1], x[:, 0]], 1).clamp(-1, 1).add(1).div(2).mul(255).round()
    y0, x0 = (x.shape[2] - crop) // 2, (x.shape[3] - crop) // 2
    return v[:, :, y0:y0 + crop, x0:x0 + crop]


def stem(x, w, b, crop, dtype):
    """conv1_1 + ReLU of the preprocessed crop"""
    return F.relu(F.conv2d(preprocess(x, crop).to(dtype), w.cpu().to(dtype), b.cpu().to(dtype), padding=1))


def logits(x, sd, dtype, preprocessed=False):
    h = (x.detach().cpu().float() if preprocessed else preprocess(x, crop_of(sd))).to(dtype)
    at = 0
    for n in CONVS:
        for _ in range(n):
            key = conv_keys()[at][0]
            h = F.relu(F.conv2d(h, sd[f'{key}.weight'].cpu().to(dtype), sd[f'{key}.bias'].cpu().to(dtype), padding=1))
            at += 1
        h = F.max_pool2d(h, 2, 2)
    h = h.flatten(1)
    for name in ('fc1.0', 'fc2.0'):
        h = F.relu(F.linear(h, sd[f'{name}.weight'].cpu().to(dtype), sd[f'{name}.bias'].cpu().to(dtype)))
    return F.linear(h, sd['cls.weight'].cpu().to(dtype), sd['cls.bias'].cpu().to(dtype))


def probabilities(x, sd, dtype, preprocessed=False):
    """[B,C] in `dtype`"""
    return F.softmax(logits(x, sd, dtype, preprocessed), dim=1)


def age_weights(C, dtype=torch.float64):
    return torch.arange(1, C + 1, dtype=dtype)


def score_of(p, attribute):
    """api.py:42-44, :56-58 (age: the weights are 1 ... C) and :64 (gender: the first class)"""
    return (p * age_weights(p.shape[1], p.dtype)).sum(1) if attribute == 'age' else p[:, 0]


def score_bar(bar, p64, attribute):
    """per row: |d score| <= |weights|_2 |dp|_2 (Cauchy-Schwarz) with |dp|_2 <= bar |p64|_2, the probability bar"""
    wn = float(age_weights(p64.shape[1]).norm()) if attribute == 'age' else 1.0
    return bar * wn * p64.double().norm(dim=1)

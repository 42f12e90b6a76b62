"""Plain-torch restatement of the CelebA-HQ attribute classifier of attribute editing (our_interfaceGAN/celebahq_utils/dex/networks/
classifiers/attribute_classifier.py: D with fixed_size=True, use_mbstd=False; attribute_utils.py:8-32; called from
edit_all_noinversion_celebahq.py:175-182; no reference code is read at run time):

    RGB [-1, 1] -> BGR -> clamp, +1, /2, *255, round -> f x f box mean down to R x R
    -> fromrgb_lod0: conv 1x1 * sqrt(2 / 3) + b, lrelu
    -> for r = R, R / 2, ..., 8:  conv0 3x3 * sqrt(2 / (9 Ci)) + b, lrelu;  conv1 3x3 * scale + b, 2x2 average pool, lrelu
    -> 4x4: conv 3x3 * scale + b, lrelu; flatten; dense0 * sqrt(2 / K) + b, lrelu; dense1 * sqrt(1 / K) + b = the logit l
    -> softmax([l, -l])[:, 1] = 1 / (1 + exp(2 l))

(lrelu = leaky ReLU 0.2) indexed by the reference's state dict keys, in whatever dtype it is asked for (the preprocessing always runs in
torch's own fp32, as the reference runs it), and the seeded weights and images the tests and tools/celeba_attr_golden.py share.
Everything runs on the CPU.

The channel counts follow the reference's rule nf(stage) = min(fmap_base / 2^stage, fmap_max): the stem and the block at 2^k pixels
have nf(k - 1) channels, the block's conv1 leaves nf(k - 2).
"""
import functools
import math

import torch
import torch.nn.functional as F

SLOPE = 0.2


def nf(stage, fmap_base=8192, fmap_max=512):
    return min(int(fmap_base / 2.0 ** stage), fmap_max)


def layers(R, fmap_base=8192, fmap_max=512):
    """[(key prefix, weight shape, fan-in, gain)] in network order; key + '.weight' / key's wscale.b are the state dict's names"""
    k = int(math.log2(R))
    assert R == 2 ** k and R >= 8
    n = functools.partial(nf, fmap_base=fmap_base, fmap_max=fmap_max)
    out = [('fromrgb_lod0.conv', (n(k - 1), 3, 1, 1), 3, 2.0)]
    for res in range(k, 2, -1):
        r = 2 ** res
        out.append((f'{r}x{r}.conv0', (n(res - 1), n(res - 1), 3, 3), 9 * n(res - 1), 2.0))
        out.append((f'{r}x{r}.conv1', (n(res - 2), n(res - 1), 3, 3), 9 * n(res - 1), 2.0))
    out.append(('4x4.conv', (n(1), n(1), 3, 3), 9 * n(1), 2.0))
    out.append(('4x4.dense0', (n(0), n(1) * 16), n(1) * 16, 2.0))
    out.append(('4x4.dense1', (1, n(0)), n(0), 1.0))
    return out


def weight_key(prefix):
    return f'{prefix}.linear.weight' if 'dense' in prefix else f'{prefix}.conv.weight'


def bias_key(prefix):
    return f'{prefix}.wscale.b'


def resolution_of(sd):
    return max(int(k.split('x')[0]) for k in sd if k.endswith('.conv0.conv.weight'))


def state_dict(seed, R, fmap_base=8192, fmap_max=512):
    """The reference's key names from torch.Generator().manual_seed(seed), on the CPU: every weight and bias ~ N(0, 1), the scale of the
    trained files (the equalised learning rate keeps the constant scale outside the parameter).  dense1's weight is divided by 255: the
    network's input is byte levels, so this leaves the logit of order one and the score unsaturated."""
    g = torch.Generator().manual_seed(seed)
    sd = {'lod_in': torch.tensor(0.0, dtype=torch.float64)}
    for prefix, shape, _, _ in layers(R, fmap_base, fmap_max):
        sd[weight_key(prefix)] = torch.randn(*shape, generator=g)
        sd[bias_key(prefix)] = torch.randn(shape[0], generator=g)
    sd['4x4.dense1.linear.weight'] /= 255
    return sd


def images(seed, B, S):
    """bilinearly upsampled 4 x 4 noise * 1.2 + 0.3 * randn: smooth structure that differs per image, about 30 % of the pixels outside
    [-1, 1]"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, 3, 4, 4, generator=g)
    return F.interpolate(low, size=(S, S), mode='bilinear', align_corners=False) * 1.2 + 0.3 * torch.randn(B, 3, S, S, generator=g)


def preprocess(x):
    """edit_all_noinversion_celebahq.py:175-177 in torch's fp32: [B,3,S,S] RGB -> BGR byte levels"""
    x = x.detach().cpu().float()
    return torch.stack([x[:, 2], x[:, 1], x[:, 0]], 1).clamp(-1, 1).add(1).div(2).mul(255).round()


def box_mean(v, R):
    """attribute_utils.py:8-19 for any resolution: the mean over f x f blocks, f = S / R"""
    S = v.shape[2]
    f = S // R
    assert f * R == S and v.shape[3] == S
    return v if f == 1 else v.view(v.shape[0], v.shape[1], R, f, R, f).mean(dim=[3, 5])


def lrelu(x):
    return F.leaky_relu(x, SLOPE)


def _wb(sd, prefix, dtype):
    return sd[weight_key(prefix)].cpu().to(dtype), sd[bias_key(prefix)].cpu().to(dtype)


def scale_of(w, gain):
    """gain / sqrt(fan-in) with gain^2 = 2, or 1 for dense1"""
    return math.sqrt(gain / w[0].numel())


def stem(x, w, b, R, dtype, preprocessed=False):
    """fromrgb_lod0 on the box mean of the byte levels; w [C0,3] is ALREADY scaled (what te_attr_stem_fwd_f32 takes)"""
    v = x.detach().cpu().float() if preprocessed else preprocess(x)
    m = box_mean(v.to(dtype), R)
    return lrelu(F.conv2d(m, w.cpu().to(dtype).view(-1, 3, 1, 1), b.cpu().to(dtype)))


def logits(x, sd, dtype, preprocessed=False):
    """[B] in `dtype`"""
    R = resolution_of(sd)
    v = x.detach().cpu().float() if preprocessed else preprocess(x)
    h = box_mean(v.to(dtype), R)
    w, b = _wb(sd, 'fromrgb_lod0.conv', dtype)
    h = lrelu(F.conv2d(h, w) * scale_of(w, 2.0) + b.view(1, -1, 1, 1))
    r = R
    while r >= 8:
        w, b = _wb(sd, f'{r}x{r}.conv0', dtype)
        h = lrelu(F.conv2d(h, w, padding=1) * scale_of(w, 2.0) + b.view(1, -1, 1, 1))
        w, b = _wb(sd, f'{r}x{r}.conv1', dtype)
        h = lrelu(F.avg_pool2d(F.conv2d(h, w, padding=1) * scale_of(w, 2.0) + b.view(1, -1, 1, 1), 2, 2))
        r //= 2
    w, b = _wb(sd, '4x4.conv', dtype)
    h = lrelu(F.conv2d(h, w, padding=1) * scale_of(w, 2.0) + b.view(1, -1, 1, 1)).flatten(1)
    w, b = _wb(sd, '4x4.dense0', dtype)
    h = lrelu(F.linear(h, w) * scale_of(w, 2.0) + b)
    w, b = _wb(sd, '4x4.dense1', dtype)
    return (F.linear(h, w) * scale_of(w, 1.0) + b)[:, 0]


def score_of(l):
    """attribute_utils.py:28-32: softmax([l, -l])[:, 1], which DECREASES in l"""
    return F.softmax(torch.stack([l, -l], 1), dim=1)[:, 1]


# ---------------------------------------------------------------------------------------------------------- the shared cases
# Seed 0 (images: 100) is the first for which the fp64 restatement meets `conditions`, in every case.
# The W == 16 form of the split-bf16 Winograd kernel needs an even batch AND at least 128 blocks (te_conv_wino6_supported: B / 2 * 2
# tiles x M / 64 channel blocks); with 128 channels that is a batch of 64, which only the small r16w6 network makes cheap in fp64.
CASES = {
    'r16': dict(R=16, fmap_base=128, fmap_max=32, B=3, S=16, seed=0, image_seed=100),          # channels 16 / 32: the plain route
    'r64b2': dict(R=64, fmap_base=4096, fmap_max=128, B=2, S=64, seed=0, image_seed=100),      # 128 channels; wino6 at 64 and 32 px
    'r64b3': dict(R=64, fmap_base=4096, fmap_max=128, B=3, S=64, seed=0, image_seed=100),      # the odd batch
    'r64s128': dict(R=64, fmap_base=4096, fmap_max=128, B=2, S=128, seed=0, image_seed=100),   # f = 2 into the same network
    'r16w6': dict(R=16, fmap_base=4096, fmap_max=128, B=64, S=16, seed=0, image_seed=100),     # 128 channels: the W == 16 wino6 form
}
# what tools/celeba_attr_golden.py records in tests/golden/celeba_attr_ref.npz
GOLDEN = {
    'small': dict(R=32, fmap_base=256, fmap_max=64, B=4, S=32, seed=0, image_seed=100),        # channels 16 / 32 / 64
    'true': dict(R=256, fmap_base=8192, fmap_max=512, B=2, S=256, seed=0, image_seed=100),     # the real files' geometry: 64 ... 512
}


def case_state_dict(c):
    return state_dict(c['seed'], c['R'], c['fmap_base'], c['fmap_max'])


def case_images(c):
    return images(c['image_seed'], c['B'], c['S'])


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(fp64 logits, fp32 logits) of the restatement for CASES[name]: computed once per process, never modified"""
    c = CASES[name]
    sd, x = case_state_dict(c), case_images(c)
    return logits(x, sd, torch.float64), logits(x, sd, torch.float32)


def conditions(l64, x):
    """what the fp64 restatement itself must meet for a case to test anything: no score saturates, the images are told apart, the clamp
    is live on both sides.  -> dict of the figures; raises AssertionError"""
    s = score_of(l64.double())
    v = preprocess(x)
    low, high = float((v == 0).float().mean()), float((v == 255).float().mean())
    spread = float(l64.max() - l64.min())
    assert 0.05 < float(s.min()) and float(s.max()) < 0.95, f'saturated scores {s.tolist()}'
    assert spread >= 0.1, f'logit spread {spread}'
    assert low > 0.02 and high > 0.02, f'clamped fractions {low} / {high}'
    return dict(score_min=float(s.min()), score_max=float(s.max()), spread=spread, clamped_low=low, clamped_high=high)

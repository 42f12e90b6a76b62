"""Plain-torch restatement of the PRDC feature extractor (metrics/calc_prdc.py:101-104: torchvision vgg16 with classifier[:-1] in eval
mode; no reference code is read at run time):

    vgg16.features (13 x conv3x3 + ReLU, five 2x2 max-pools) -> adaptive_avg_pool2d(7) -> flatten -> Linear, ReLU, Linear, ReLU

indexed by torchvision's state dict keys, in whatever dtype it is asked for, and a synthetic full state dict filled from a seed.  The
convolutions run on the CPU (torch's fp64 convolution is sure to exist there); the classifier runs where its weights live: they are
411 MB, so they are generated on the device and never written to disk.
"""
import torch
import torch.nn.functional as F

VGG_CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_BEFORE = (2, 4, 7, 10)                  # a max-pool in front of these convolutions; the fifth follows the last one
FC = ((0, 4096, 512 * 7 * 7), (3, 4096, 4096))


def conv_state_dict(seed=0):
    """features.* only, on the CPU: He-scaled normal weights and small biases (activations keep their size through 13 layers)"""
    g = torch.Generator().manual_seed(seed)
    sd, ci = {}, 3
    for idx, co in zip(VGG_CONV_INDEX, VGG_CHANNELS):
        sd[f'features.{idx}.weight'] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        sd[f'features.{idx}.bias'] = torch.randn(co, generator=g) * 0.05
        ci = co
    return sd


def full_state_dict(seed=0, device='cuda'):
    """conv_state_dict plus classifier.{0,3,6}: fan-in-scaled normal weights, small biases, made on `device`"""
    sd = conv_state_dict(seed)
    g = torch.Generator(device=device).manual_seed(seed + 1)
    for idx, j, k in FC:
        sd[f'classifier.{idx}.weight'] = torch.randn(j, k, generator=g, device=device) * (2.0 / k) ** 0.5
        sd[f'classifier.{idx}.bias'] = torch.randn(j, generator=g, device=device) * 0.05
    sd['classifier.6.weight'] = torch.zeros(10, 4096, device=device)          # the logits layer: never read
    sd['classifier.6.bias'] = torch.zeros(10, device=device)
    return sd


def pool5(x, sd, dtype):
    """vgg16.features on the CPU in `dtype`: [B,3,H,W] -> [B,512,H/32,W/32]"""
    h = x.detach().cpu().to(dtype)
    for j, idx in enumerate(VGG_CONV_INDEX):
        if j in POOL_BEFORE:
            h = F.max_pool2d(h, 2, 2)
        h = F.relu(F.conv2d(h, sd[f'features.{idx}.weight'].cpu().to(dtype), sd[f'features.{idx}.bias'].cpu().to(dtype), padding=1))
    return F.max_pool2d(h, 2, 2)


def fc7(x, sd, dtype):
    """the whole extractor in `dtype` -> [B,4096] on the classifier weights' device"""
    w0 = sd['classifier.0.weight']
    h = F.adaptive_avg_pool2d(pool5(x, sd, dtype), 7).flatten(1).to(w0.device)
    for idx, _, _ in FC:
        h = F.relu(F.linear(h, sd[f'classifier.{idx}.weight'].to(dtype), sd[f'classifier.{idx}.bias'].to(dtype)))
    return h

"""Plain-torch restatement of the pose scorer of attribute editing (our_interfaceGAN/ffhq_utils/dex/models.py:73-89 ClassifyModel, api.py:61-65,
called from edit_all_noinversion_ffhq.py:113-131; no reference code is read at run time):

    RGB [-1, 1] -> BGR -> clamp, +1, /2, *255, round -> centre crop -> conv 7x7 stride 2 pad 3 (no bias) -> batch norm -> ReLU
    -> max pool 3x3 stride 2 pad 1 -> eight basic blocks (conv3x3, bn, ReLU, conv3x3, bn, + the input or its 1x1 stride-2 conv + bn, ReLU)
    -> mean over the plane -> Linear -> softmax -> p_0

indexed by the reference's state dict keys, with the batch norms NOT folded (F.batch_norm, eps 1e-5, eval), in whatever dtype it is
asked for (the preprocessing always runs in torch's own fp32, as the reference runs it); a synthetic state dict filled from a seed;
and the same network in module form with torchvision's child order and names (`resnet18`), the placeholder tools/pose_golden.py hands
the reference's models.py.  Everything runs on the CPU.

The four widths are read from the shapes, as transeditor_amd.pose reads them; the real file has (64, 128, 256, 512), 2 classes and a
224 px crop, the tests also use smaller networks.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from dex_restated import images, preprocess, score_bar  # noqa: F401  (the scorers share the test images and the preprocessing)

WIDTHS = (64, 128, 256, 512)
BN_EPS = 1e-5
BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')

# what tools/pose_golden.py records in tests/golden/pose_ref.npz (images: seed + 100)
GOLDEN = dict(seed=1, image_seed=101, B=2, S=256, crop=224)


def blocks():
    """[(key prefix, layer index 0 ... 3, has a downsample)] * 8 in network order"""
    return [(f'backbone.{4 + li}.{blk}', li, blk == 0 and li > 0) for li in range(4) for blk in range(2)]


def conv_bn_keys():
    """[(convolution key, batch norm key, kernel size)] * 20, in the order state_dict() draws them"""
    out = [('backbone.0', 'backbone.1', 7)]
    for p, _, down in blocks():
        out += [(f'{p}.conv1', f'{p}.bn1', 3), (f'{p}.conv2', f'{p}.bn2', 3)]
        if down:
            out.append((f'{p}.downsample.0', f'{p}.downsample.1', 1))
    return out


def widths_of(sd):
    return tuple(sd[f'backbone.{4 + li}.0.conv1.weight'].shape[0] for li in range(4))


def features(x, sd, dtype, crop, preprocessed=False):
    """[B,widths[3]] in `dtype`: everything before extra_layer"""
    x = x.detach().cpu().float()
    if preprocessed:
        y0, x0 = (x.shape[2] - crop) // 2, (x.shape[3] - crop) // 2
        h = x[:, :, y0:y0 + crop, x0:x0 + crop]
    else:
        h = preprocess(x, crop)
    h = h.to(dtype)
    P = {k: v.cpu().to(dtype) for k, v in sd.items() if v.is_floating_point()}

    def bn(t, k):
        return F.batch_norm(t, P[f'{k}.running_mean'], P[f'{k}.running_var'], P[f'{k}.weight'], P[f'{k}.bias'], False, 0.0, BN_EPS)
    h = F.relu(bn(F.conv2d(h, P['backbone.0.weight'], None, 2, 3), 'backbone.1'))
    h = F.max_pool2d(h, 3, 2, 1)
    for p, _, down in blocks():
        s = 2 if down else 1
        y = F.relu(bn(F.conv2d(h, P[f'{p}.conv1.weight'], None, s, 1), f'{p}.bn1'))
        y = bn(F.conv2d(y, P[f'{p}.conv2.weight'], None, 1, 1), f'{p}.bn2')
        if down:
            h = bn(F.conv2d(h, P[f'{p}.downsample.0.weight'], None, s, 0), f'{p}.downsample.1')
        h = F.relu(y + h)
    return h.mean((2, 3))


def logits(x, sd, dtype, crop, preprocessed=False):
    return F.linear(features(x, sd, dtype, crop, preprocessed), sd['extra_layer.weight'].cpu().to(dtype), sd['extra_layer.bias'].cpu().to(dtype))


def probabilities(x, sd, dtype, crop, preprocessed=False):
    """[B,C] in `dtype`"""
    return F.softmax(logits(x, sd, dtype, crop, preprocessed), dim=1)


def state_dict(seed, widths=WIDTHS, images=None, crop=GOLDEN['crop'], classes=2):
    """ClassifyModel's key names from torch.Generator().manual_seed(seed), on the CPU: He-scaled normal convolutions (the stem's divided
    by 128: its input is 0 ... 255), gamma and running_var uniform in [0.5, 1.5], beta and running_mean 0.2 * randn, one
    num_batches_tracked per batch norm, extra_layer with gain 1.  A network drawn like this saturates the softmax (p_0 comes out
    exactly 0 or 1: the features are all positive and their common part is multiplied by a random weight sum).  So, given the test
    `images`, extra_layer is CALIBRATED on them in fp64: its weight is scaled so that the logits have unit spread over images and
    classes, and its bias is minus their mean per class.  Without images the drawn extra_layer is kept (host-side tests)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(k, co, ci, ks):
        sd[f'{k}.weight'] = torch.randn(co, ci, ks, ks, generator=g) * (2.0 / (ci * ks * ks)) ** 0.5

    def bn(k, c):
        sd[f'{k}.weight'] = torch.rand(c, generator=g) + 0.5
        sd[f'{k}.bias'] = torch.randn(c, generator=g) * 0.2
        sd[f'{k}.running_mean'] = torch.randn(c, generator=g) * 0.2
        sd[f'{k}.running_var'] = torch.rand(c, generator=g) + 0.5
        sd[f'{k}.num_batches_tracked'] = torch.tensor(0, dtype=torch.long)
    conv('backbone.0', widths[0], 3, 7)
    sd['backbone.0.weight'] /= 128.0
    bn('backbone.1', widths[0])
    ci = widths[0]
    for p, li, down in blocks():
        co = widths[li]
        conv(f'{p}.conv1', co, ci, 3)
        bn(f'{p}.bn1', co)
        conv(f'{p}.conv2', co, co, 3)
        bn(f'{p}.bn2', co)
        if down:
            conv(f'{p}.downsample.0', co, ci, 1)
            bn(f'{p}.downsample.1', co)
        ci = co
    sd['extra_layer.weight'] = torch.randn(classes, ci, generator=g) * (1.0 / ci) ** 0.5
    sd['extra_layer.bias'] = torch.randn(classes, generator=g) * 0.1
    if images is not None:
        f = features(images, sd, torch.float64, crop)
        w = sd['extra_layer.weight'].double()
        lg = f @ w.t()
        scale = 1.0 / float(lg.std())
        sd['extra_layer.weight'] = (w * scale).float()
        sd['extra_layer.bias'] = (-(lg * scale).mean(0)).float()
    return sd


# ------------------------------------------------------------------------------------------------------------ the module form
class BasicBlock(nn.Module):
    def __init__(self, ci, co, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(ci, co, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(co)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(co, co, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(co)
        self.downsample = None
        if stride != 1 or ci != co:
            self.downsample = nn.Sequential(nn.Conv2d(ci, co, 1, stride, bias=False), nn.BatchNorm2d(co))

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        out += identity
        return self.relu(out)


class ResNet18(nn.Module):
    """children in torchvision's order and under its names: conv1, bn1, relu, maxpool, layer1 ... layer4, avgpool, fc"""

    def __init__(self, widths=WIDTHS, num_classes=1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, widths[0], 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(widths[0])
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        ci = widths[0]
        for li, co in enumerate(widths):
            setattr(self, f'layer{li + 1}', nn.Sequential(BasicBlock(ci, co, 2 if li else 1), BasicBlock(co, co, 1)))
            ci = co
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(ci, num_classes)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        for li in range(4):
            x = getattr(self, f'layer{li + 1}')(x)
        return self.fc(torch.flatten(self.avgpool(x), 1))


def resnet18(**kw):
    return ResNet18(**kw)

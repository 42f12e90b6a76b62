"""Plain-torch restatements for the LPIPS / projector tests (no reference code is read at run time):

- LPIPS-VGG 'net-lin' v0.1: utils/lpips/networks_basic.py:21-87 (ScalingLayer, normalize_tensor, lin heads, spatial_average, sum of
  the five layers in order), pretrained_networks.py:98-136 (vgg16.features[0:30] in five slices, taps relu1_2 ... relu5_3);
- the noise regulariser and noise normalisation: projector_optimization.py:21-49;
- seeded random weight files in the torchvision vgg16 and LPIPS v0.1 layouts.
"""
import torch
import torch.nn.functional as F

VGG_CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
SHIFT = torch.tensor([-.030, -.088, -.188])
SCALE = torch.tensor([.458, .448, .450])


def write_weights(tmp_path, seed=0):
    """(vgg_path, lin_path): He-scaled random convolutions (so activations keep their size through 13 layers), lin >= 0"""
    g = torch.Generator().manual_seed(seed)
    sd, ci = {}, 3
    for idx, co in zip(VGG_CONV_INDEX, VGG_CHANNELS):
        sd[f'features.{idx}.weight'] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        sd[f'features.{idx}.bias'] = torch.randn(co, generator=g) * 0.05
        ci = co
    sd['classifier.0.weight'] = torch.zeros(2, 2)                       # other keys are ignored
    lin = {f'lin{l}.model.1.weight': torch.rand(1, c, 1, 1, generator=g) * 0.1 for l, c in enumerate((64, 128, 256, 512, 512))}
    vp, lp = str(tmp_path / 'vgg16.pth'), str(tmp_path / 'vgg.pth')
    torch.save(sd, vp)
    torch.save(lin, lp)
    return vp, lp


def normalize_tensor(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def vgg_taps(x, sd):
    h = (x - SHIFT.to(x).view(1, 3, 1, 1)) / SCALE.to(x).view(1, 3, 1, 1)
    taps = []
    for j, idx in enumerate(VGG_CONV_INDEX):
        if j in (2, 4, 7, 10):
            h = F.max_pool2d(h, 2, 2)
        h = F.relu(F.conv2d(h, sd[f'features.{idx}.weight'].to(x), sd[f'features.{idx}.bias'].to(x), padding=1))
        if j in (1, 3, 6, 9, 12):
            taps.append(h)
    return taps


def target_taps(target, vgg_sd):
    """the target's normalised taps (what a cached target holds)"""
    return [normalize_tensor(t) for t in vgg_taps(target, vgg_sd)]


def lpips_from_taps(pred, t_taps, vgg_sd, lin_sd):
    """networks_basic.py:59-82 with the target's normalised taps given -> [N,1,1,1]"""
    t1 = vgg_taps(pred, vgg_sd)
    val = None
    for l in range(5):
        diff = (t_taps[l] - normalize_tensor(t1[l])) ** 2
        r = F.conv2d(diff, lin_sd[f'lin{l}.model.1.weight'].to(pred)).mean([2, 3], keepdim=True)
        val = r if val is None else val + r
    return val


def lpips(pred, target, vgg_sd, lin_sd):
    """model.forward(target, pred) -> [N,1,1,1]"""
    return lpips_from_taps(pred, target_taps(target, vgg_sd), vgg_sd, lin_sd)


def noise_regularize(noises):
    loss = 0
    for noise in noises:
        size = noise.shape[2]
        while True:
            loss = (loss + (noise * torch.roll(noise, shifts=1, dims=3)).mean().pow(2)
                    + (noise * torch.roll(noise, shifts=1, dims=2)).mean().pow(2))
            if size <= 8:
                break
            noise = noise.reshape([-1, 1, size // 2, 2, size // 2, 2])
            noise = noise.mean([3, 5])
            size //= 2
    return loss


def noise_normalize(noises):
    return [(n - n.mean()) / n.std() for n in noises]


def noise_list(size, batch, seed):
    g = torch.Generator().manual_seed(seed)
    sizes = [4] + [2 ** i for i in range(3, size.bit_length()) for _ in range(2)]
    return [torch.randn(batch, 1, s, s, generator=g) for s in sizes]

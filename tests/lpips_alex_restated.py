"""Plain-torch restatement of the AlexNet LPIPS of the diversity score (metrics/lpips.py:16-17, :49-82, called pair by pair from
metrics/evaluate_query.py:82-91; no reference code is read at run time):

    (x - mu) / sigma -> conv 11x11 stride 4 pad 2, ReLU*, max pool 3x3 stride 2 -> conv 5x5 pad 2, ReLU*, max pool 3x3 stride 2
    -> conv 3x3 pad 1, ReLU* -> conv 3x3 pad 1, ReLU* -> conv 3x3 pad 1, ReLU*                 (* a tap; the last pool feeds nothing)
    tap -> f * rsqrt(sum_c f^2 + 1e-10);   d(a, b) = sum_l mean_p sum_c w_l[c] (fa - fb)^2

indexed by torchvision's alexnet state dict keys (features.{0,3,6,8,10}.*) and the reference's head keys
(lpips_weights.{l}.main.1.weight), in whatever dtype it is asked for; seeded synthetic weights and images; and the same network in
module form with torchvision's child order and names (`alexnet`), the placeholder tools/lpips_alex_golden.py hands the reference's
lpips.py.  Everything runs on the CPU.  The widths are read from the shapes; the real network has (64, 192, 384, 256, 256).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

WIDTHS = (64, 192, 384, 256, 256)
CONVS = (0, 3, 6, 8, 10)
GEOMETRY = ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))   # (kernel, stride, padding)
POOL_BEFORE = (1, 2)
MU = (-0.03, -0.088, -0.188)
SIGMA = (0.458, 0.448, 0.450)
EPS = 1e-10

# what tools/lpips_alex_golden.py records in tests/golden/lpips_alex_ref.npz
GOLDEN = dict(seed=1, image_seed=101, N=6, S=64)


def images(seed, N, S, W=None):
    """tanh(randn): generator-like images inside (-1, 1)"""
    return torch.tanh(torch.randn(N, 3, S, W or S, generator=torch.Generator().manual_seed(seed)))


def state_dict(seed, widths=WIDTHS):
    """torchvision alexnet's `features` keys from torch.Generator().manual_seed(seed): He-scaled normal weights, biases 0.1 * randn"""
    g = torch.Generator().manual_seed(seed)
    sd, ci = {}, 3
    for i, (k, _, _), co in zip(CONVS, GEOMETRY, widths):
        sd[f'features.{i}.weight'] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd[f'features.{i}.bias'] = torch.randn(co, generator=g) * 0.1
        ci = co
    return sd


def lin_state_dict(seed, widths=WIDTHS, signed=False):
    """heads in the layout of metrics/lpips_weights.ckpt: uniform in [0, 0.1) (the real file is non-negative); signed: in
    [-0.025, 0.075), a quarter of the weights negative"""
    g = torch.Generator().manual_seed(seed)
    return {f'lpips_weights.{l}.main.1.weight': (torch.rand(1, c, 1, 1, generator=g) - (0.25 if signed else 0.0)) * 0.1 for l, c in enumerate(widths)}


def scale(x, dtype):
    """(x - mu) / sigma; the constants are the reference's fp32 tensors (lpips.py:58-59) in every dtype"""
    x = x.detach().cpu().to(dtype)
    return (x - torch.tensor(MU, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)) / torch.tensor(SIGMA, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)


def taps(x, sd, dtype):
    """the five ReLU outputs, not normalised"""
    h, out = scale(x, dtype), []
    for l, (i, (_, s, p)) in enumerate(zip(CONVS, GEOMETRY)):
        if l in POOL_BEFORE:
            h = F.max_pool2d(h, 3, 2)
        h = F.relu(F.conv2d(h, sd[f'features.{i}.weight'].cpu().to(dtype), sd[f'features.{i}.bias'].cpu().to(dtype), s, p))
        out.append(h)
    return out


def unit(f):
    """metrics/lpips.py:16-17"""
    return f * torch.rsqrt(torch.sum(f ** 2, dim=1, keepdim=True) + EPS)


def head_pairwise(fh, w):
    """one layer: D [N,N] for normalised taps fh [N,C,...] and w [C], the difference before the square"""
    N = fh.shape[0]
    fh = fh.reshape(N, fh.shape[1], -1)
    D = torch.zeros(N, N, dtype=fh.dtype)
    for i in range(N - 1):
        d = (fh[i:i + 1] - fh[i + 1:]) ** 2                             # [N - 1 - i,C,HW]: the pairs (i, j > i)
        D[i, i + 1:] = (d * w.to(fh.dtype).view(1, -1, 1)).sum(1).mean(1)
    return D + D.t()


def heads_of(lin, dtype=torch.float32):
    return [lin[f'lpips_weights.{l}.main.1.weight'].cpu().to(dtype).reshape(-1) for l in range(5)]


def pairwise(x, sd, lin, dtype):
    """D [N,N] in `dtype`, layers added in order"""
    D = None
    for f, w in zip(taps(x, sd, dtype), heads_of(lin, dtype)):
        m = head_pairwise(unit(f), w)
        D = m if D is None else D + m
    return D


def triu(D):
    i, j = torch.triu_indices(D.shape[0], D.shape[0], 1)
    return D[i, j]


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------------------ the module form
class AlexNet(nn.Module):
    """children in torchvision's order and under its names: features (13 layers), avgpool, classifier"""

    def __init__(self, widths=WIDTHS, num_classes=1000):
        super().__init__()
        layers, ci = [], 3
        for l, ((k, s, p), co) in enumerate(zip(GEOMETRY, widths)):
            layers += [nn.Conv2d(ci, co, k, s, p), nn.ReLU(inplace=True)]
            if l in (0, 1, 4):
                layers.append(nn.MaxPool2d(3, 2))
            ci = co
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d((6, 6))
        self.classifier = nn.Sequential(nn.Dropout(), nn.Linear(ci * 36, 4096), nn.ReLU(inplace=True), nn.Dropout(), nn.Linear(4096, 4096),
                                        nn.ReLU(inplace=True), nn.Linear(4096, num_classes))

    def forward(self, x):
        return self.classifier(torch.flatten(self.avgpool(self.features(x)), 1))


def alexnet(pretrained=False, **kw):
    return AlexNet(**kw)

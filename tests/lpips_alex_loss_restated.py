"""Plain-torch restatement of the AlexNet LPIPS of encoder training (pSp/criteria/lpips/lpips.py:29-35 LPIPS('alex').forward with
networks.py:49-62 and utils.py:6-8; no reference code is read at run time), differentiable by torch autograd in whatever dtype it is
asked for:

    taps as tests/lpips_alex_restated.py;   tap -> f / (sqrt(sum_c f^2) + 1e-10)          (eps BESIDE the root)
    loss(x, y) = sum_l sum_b mean_p sum_c w_l[c] (fx - fy)^2 / B

and the contracts of the two backward entry points of csrc/lpips_alex_bwd.hip as te_hip.h words them.  Everything runs on the CPU.
"""
import torch
import torch.nn.functional as F

import lpips_alex_restated as R

EPS = 1e-10
# what tools/lpips_alex_loss_golden.py records in tests/golden/lpips_alex_loss_ref.npz
GOLDEN = dict(seed=1, x_seed=101, y_seed=202, B=3, S=64)


def scale(x, dtype):
    """R.scale with the graph kept"""
    x = x.to(dtype)
    return (x - torch.tensor(R.MU, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)) / torch.tensor(R.SIGMA, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)


def taps(x, sd, dtype):
    """the five ReLU outputs, not normalised, with the graph kept"""
    h, out = scale(x, dtype), []
    for l, (i, (_, s, p)) in enumerate(zip(R.CONVS, R.GEOMETRY)):
        if l in R.POOL_BEFORE:
            h = F.max_pool2d(h, 3, 2)
        h = F.relu(F.conv2d(h, sd[f'features.{i}.weight'].cpu().to(dtype), sd[f'features.{i}.bias'].cpu().to(dtype), s, p))
        out.append(h)
    return out


def normalize(f):
    """pSp/criteria/lpips/utils.py:6-8"""
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + EPS)


def heads_of(lin, dtype=torch.float32):
    """[w [C]] * 5 from lin{l}.model.1.weight"""
    return [lin[f'lin{l}.model.1.weight'].cpu().to(dtype).reshape(-1) for l in range(5)]


def lin_state_dict(seed, widths=R.WIDTHS):
    """heads in the layout of the richzhang alex.pth: uniform in [0, 0.1) (the real file is non-negative)"""
    g = torch.Generator().manual_seed(seed)
    return {f'lin{l}.model.1.weight': torch.rand(1, c, 1, 1, generator=g) * 0.1 for l, c in enumerate(widths)}


def loss(x, y, sd, lin, dtype):
    """LPIPS.forward(x, y) -> 0-dim, the layers added in order"""
    val = None
    for fx, fy, w in zip(taps(x, sd, dtype), taps(y.detach(), sd, dtype), heads_of(lin, dtype)):
        d = (normalize(fx) - normalize(fy)) ** 2
        m = (d * w.view(1, -1, 1, 1)).sum(1).mean((1, 2)).sum()
        val = m if val is None else val + m
    return val / x.shape[0]


def value_and_grad(x, y, sd, lin, dtype):
    """(the loss, its gradient w.r.t. x) in `dtype` on the CPU"""
    xin = x.detach().cpu().to(dtype).requires_grad_(True)
    v = loss(xin, y.detach().cpu(), sd, lin, dtype)
    g, = torch.autograd.grad(v, xin)
    return v.detach(), g


def zero_pixels(x, sd):
    """per tap: the pixels that are zero on every channel (where te_lpips_head_bwd_f32's documented NaN deviation would show)"""
    return [int(((t ** 2).sum(1) == 0).sum()) for t in taps(x.detach(), sd, torch.float64)]


# ------------------------------------------------------------------------------------------------------------ restated contracts
def pool3s2_max_bwd(g, x):
    """te_pool3s2_max_bwd_f32: torch's own max_pool2d backward on the CPU (its tie rule is the contract's)"""
    xin = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():                                                   # (callers may sit inside a Function's backward)
        return torch.autograd.grad(F.max_pool2d(xin, 3, 2), xin, g.to(x.dtype))[0]


def stem_weight_from_layout(wt, Co):
    """w [Co,3,11,11] read back from alex_stem_dgrad_weight's layout as te_hip.h words it: wt[ry][o, jy, kx, c] = w[o, c, k0(ry) + 4 jy, kx]"""
    w, at = torch.full((Co, 3, 11, 11), float('nan'), dtype=wt.dtype), 0
    for ry in range(4):
        k0 = (ry + 2) % 4
        ny = len(range(k0, 11, 4))
        blk = wt[at:at + Co * ny * 33].view(Co, ny, 11, 3)
        at += blk.numel()
        w[:, :, k0::4, :] = blk.permute(0, 3, 1, 2)
    assert at == wt.numel() and not bool(w.isnan().any())                       # every tap lands in exactly one row phase
    return w


def stem_dgrad(g, w, img_hw, dtype=torch.float64):
    """te_alex_stem_dgrad_f32 from the forward's OWN weight: conv_transpose2d(g, w, stride 4, padding 2) extended to [H, W], / sigma"""
    H, W = img_hw
    op = (H - (4 * g.shape[2] + 3), W - (4 * g.shape[3] + 3))                   # (Ho - 1) * 4 - 4 + 11 = 4 Ho + 3; 0 ... 3 rows more
    acc = F.conv_transpose2d(g.to(dtype), w.to(dtype), None, 4, 2, op)
    return acc / torch.tensor(R.SIGMA, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)


def head_bwd(gd, f, t_hat, w, gin=None, relu_mask=True):
    """te_lpips_head_bwd_f32 as te_hip.h states it, in f's dtype"""
    HW = f.shape[2] * f.shape[3]
    r = torch.sqrt((f ** 2).sum(1, keepdim=True))
    u = 2 * w.to(f.dtype).view(1, -1, 1, 1) * (f / (r + EPS) - t_hat.to(f.dtype)) * gd.to(f.dtype).view(-1, 1, 1, 1) / HW
    second = f * (f * u).sum(1, keepdim=True) / (r * (r + EPS) ** 2)
    gf = u / (r + EPS) - torch.where(r > 0, second, torch.zeros_like(second))
    if gin is not None:
        gf = gf + gin.to(f.dtype)
    return torch.where(f > 0, gf, torch.zeros_like(gf)) if relu_mask else gf

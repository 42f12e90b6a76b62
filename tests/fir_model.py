"""A plain-torch fp32 model of the FIR kernels (csrc/upfirdn2d.hip) for tests/test_fir_forms_cpu.py: it fills the buffers of a
fir_forms.Run the way a launch does, so that the instruments of tests/fir_forms.py can be proven without a GPU - they pass on the model and
fail on the model with one planted defect.

tiled(): the structure of blur44_kernel and fir_tile_kernel<1,1,4,4,AG> - a loop over the tiles of the query's plan, a zero-filled staged
window per tile, the activation-gradient prologue with its ownership rule, the 4 x 4 filter with the flipped taps, the ext column and row
of the last tiles, the epilogues, per-tile sums and stores at flat addresses (a store past a row's end lands where the kernel's would).
contract(): the arithmetic contract in the header of csrc/upfirdn2d.hip (mid, i0, j0 per axis) for every other kernel - a second
restatement next to the zero-insert / pad / slice one of tests/fir_restated.py.

DEFECTS, one at a time: 'double_own' (in image row 0 the first element right of the first tile border is owned by both neighbours),
'drop_halo' (the last tile of the plane does not own its rows of the image's last column), 'swap_pads' (pad_x0 and pad_y0 exchanged), 'flip_x' (taps flipped on the y axis
only), 'transpose' (tap matrix transposed), 'shift' (the right-edge group shifted one column too few), 'ext_flag' (the ext column taken
from the ext row's flag).
"""
import numpy as np
import torch

import fir_forms as ff
from fp64_check import GUARD

DEFECTS = ('double_own', 'drop_halo', 'swap_pads', 'flip_x', 'transpose', 'shift', 'ext_flag')


def _window(x, y0, x0, h, w):
    """x[:, y0:y0 + h, x0:x0 + w] with zeros outside the image"""
    P, H, W = x.shape
    out = x.new_zeros(P, h, w)
    ys, ye, xs, xe = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
    if ys < ye and xs < xe:
        out[:, ys - y0:ye - y0, xs - x0:xe - x0] = x[:, ys:ye, xs:xe]
    return out


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def tiled(e, f, ops, run, defect=None):
    assert defect in (None,) + DEFECTS and f['kernel'] in ('blur44', 'tile_ag')
    mode = ff.MODE_OF[e.op]
    th, tw, nx, ny = f['tile_h'], f['tile_w'], f['tiles_x'], f['tiles_y']
    px0, px1, py0, py1 = e.pad
    if defect == 'swap_pads':
        px0, py0 = py0, px0
    k = ops.k
    kf = {None: torch.flip(k, [0, 1]), 'flip_x': torch.flip(k, [0]), 'transpose': torch.flip(k.t(), [0, 1])}.get(defect, torch.flip(k, [0, 1]))
    x, P = ops.x, e.planes
    if defect == 'shift' and e.W % 4:
        g0 = e.W - e.W % 4                                   # the group that straddles the right edge, one column off
        x = x.clone()
        x[..., g0:] = ops.x[..., g0 - 1:e.W - 1]
    oh, ow = ff.out_hw(e)
    yflat = run.ybuf[GUARD:]
    epi = bool(e.bias or e.act)
    alpha, scale = _f32(ops.alpha), _f32(ops.scale)
    pos, neg = scale, alpha * scale
    planes = torch.arange(P)
    for by in range(ny):
        for bx in range(nx):
            last_x, last_y = bx == nx - 1, by == ny - 1
            ex, ey = f['ext_x'], f['ext_y']
            if defect == 'ext_flag':
                ex = ey
            oy0, ox0 = by * th, bx * tw
            rows = list(range(oy0, min(oy0 + th + (1 if ey and last_y else 0), oh)))
            cols = list(range(ox0, min(ox0 + tw, ow))) + ([ox0 + tw] if ex and last_x else [])
            nr, nc = len(rows), cols[-1] - ox0 + 1
            iy0, ix0 = oy0 - py0, ox0 - px0
            win = _window(x, iy0, ix0, max(nr, th) + 3, max(nc, tw) + 3)
            if mode == 1:
                rwin = _window(ops.ref, iy0, ix0, max(nr, th) + 3, max(nc, tw) + 3)
                win = win * torch.where(rwin > 0, pos, neg)
                own = win[:, :None if last_y else th, :None if last_x else tw].sum(dim=(1, 2))
                if defect == 'double_own' and not last_x and by == 0:
                    own = own + win[:, py0, tw]                  # image row 0, the first column of the right neighbour
                if defect == 'drop_halo' and last_x and last_y:
                    own = own - win[:, :None if last_y else th, e.W - 1 - ix0].sum(dim=1)
                run.part[:, by * nx + bx] = own
            v = torch.zeros(P, nr, nc)
            for a in range(4):
                for c in range(4):
                    v += win[:, a:a + nr, c:c + nc] * kf[a, c]
            if mode == 0 and epi:
                if e.bias:
                    v = v + ops.b[planes % e.bias][:, None, None]
                if e.act:
                    v = torch.where(v > 0, v, v * alpha)
                v = v * scale
            sel = [c - ox0 for c in cols]
            v = v[:, :, sel]
            if mode == 2:
                ci = torch.tensor(cols)
                rf = torch.zeros(P, nr, len(cols))
                ok = ci < ow
                rf[:, :, ok] = ops.ref[:, rows][:, :, ci[ok]]
                v = v * torch.where(rf > 0, pos, neg)
                run.part[:, by * nx + bx] = v.sum(dim=(1, 2))
            idx = (planes[:, None, None] * oh + torch.tensor(rows)[None, :, None]) * ow + torch.tensor(cols)[None, None, :]
            yflat[idx] = v


def contract(e, ops, run):
    """every other kernel: out[o] = sum_t in[i0 + t] kflip[j0 + t up] per axis, then the epilogue; fp32 accumulation for float and half"""
    dt = getattr(torch, e.dtype)
    acc = torch.float64 if dt == torch.float64 else torch.float32
    x, k = ops.x.to(acc), ops.k.to(acc)
    if e.minor > 1:
        x = x.permute(0, 3, 1, 2)
    (ux, uy), (dx, dy) = e.up, e.down
    px0, _, py0, _ = e.pad
    kh, kw = k.shape
    H, W = e.H, e.W
    oh, ow = ff.out_hw(e)

    def axis(n_out, down, up, pad0):
        mid = torch.arange(n_out) * down + up - 1 - pad0
        i0 = torch.div(mid, up, rounding_mode='floor')
        return i0, (i0 + 1) * up - mid - 1
    iy0, jy0 = axis(oh, dy, uy, py0)
    ix0, jx0 = axis(ow, dx, ux, px0)
    out = x.new_zeros(x.shape[:-2] + (oh, ow))
    for ty in range(-(-kh // uy)):
        iy, jy = iy0 + ty, jy0 + ty * uy
        vy = (iy >= 0) & (iy < H) & (jy < kh)
        for tx in range(-(-kw // ux)):
            ix, jx = ix0 + tx, jx0 + tx * ux
            vx = (ix >= 0) & (ix < W) & (jx < kw)
            w = k[(kh - 1 - jy).clamp(0, kh - 1)][:, (kw - 1 - jx).clamp(0, kw - 1)] * (vy[:, None] & vx[None, :])
            out = out + x[..., iy.clamp(0, H - 1), :][..., ix.clamp(0, W - 1)] * w
    if e.bias or e.act:
        alpha, scale = _f32(ops.alpha), _f32(ops.scale)
        if e.bias:
            out = out + ops.b[torch.arange(e.planes) % e.bias][:, None, None]
        if e.act:
            out = torch.where(out > 0, out, out * alpha)
        out = out * scale
    if e.minor > 1:
        out = out.permute(0, 2, 3, 1)
    run.y.copy_(out.to(dt))


def launch(e, f, ops, defect=None):
    """a fir_forms.Run filled by the model of the entry's launch"""
    run = ff.buffers(e, f, 'cpu')
    if f['kernel'] in ('blur44', 'tile_ag'):
        tiled(e, f, ops, run, defect)
    else:
        assert defect is None
        contract(e, ops, run)
    assert int(np.prod(run.y.shape)) == int(np.prod(ff.y_shape(e)))
    return run

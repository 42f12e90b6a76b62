"""Encoder head training on the gfx950 kernels: the backward pass of everything that sits on the backbone of the dual-space pSp encoder
(psp_encoder.DualSpaceEncoder), and one iteration of the reference's pSp/training/coach_new.py:128-135 with the backbone frozen.

    enc = DualSpaceEncoder('psp.pt')                                   # the backbone stays as it is
    heads = TrainableHeads(enc)                                        # the two laterals, the 30 heads, adjust_style: 333.7 M of 364.7 M
    decode = generator_decoder(generator, enc.from_plus_space)         # psp_new.py:111-116; the generator's parameters are frozen
    crit = EncoderLoss(id_loss=..., lpips_loss=..., w_norm_lambda=...) # encoder_loss.py
    opt = encoder_optimizer(heads.parameters())                        # optim.Ranger, the reference's default
    loss, loss_dict, id_logs = heads_step(enc, heads, decode, crit, opt, images)
    torch.save(heads.checkpoint(torch.load('psp.pt')), 'tuned.pt')     # loads into DualSpaceEncoder and into the reference's pSp

    python -m transeditor_amd.psp_heads_train --ckpt psp.pt --g_ckpt G.pt --images X.pt --steps N --out tuned.pt [--lr 1e-4] [--batch 8]
                                              [--id_ckpt model_ir_se50.pth --alexnet alexnet.pth --lpips_alex_lin alex.pth]

TrainableHeads owns, as fp32 nn.Parameters on the device: the packed head weights h{n}_w and biases h{n}_b of the encoder's launch
program, the STORED (unscaled) EqualLinear weights lin_w / lin_b and adjust_w / adjust_b, and the laterals lat1_* / lat2_*.  A packed
weight is held as [G*D, Ci, 3, 3] and lin_w as [n*D, D], the heads one behind the other: optim.Ranger centralises a gradient over
every dim but the first, and these shapes give it the rows the reference's per-layer [D, Ci, 3, 3] and [D, D] parameters have.  The
forward is one hand-written autograd.Function (as arcface.ArcFaceID.embed_grad is): (c1, c2, c3, *params) -> (z_code, p_code) without
the latent averages.  It runs DualSpaceEncoder's launch program unchanged (the codes are bitwise encode()'s on the same weights) and
keeps the level buffers it allocates anyway; the leaky ReLU's branch is read from a kept OUTPUT's sign (the slope is positive).  The
backward walks the program in reverse, per launch te_conv2d_heads_wgrad_f32 and then the data gradient: te_conv2d_heads_dgrad_f32 for
heads on their own activations, te_conv2d_dgrad_f32 on the weight viewed as one [G*D, Ci, 3, 3] convolution for heads that share a
feature, its `add` accumulating the feature's several consumers; then the two upsample adjoints and the laterals.  It returns the
gradients of all parameters and of c1, c2, c3 (the seam to a backbone backward pass).  EqualLinear's scales are folded on the way in
and multiplied onto the gradients on the way out.  Once differentiable: a double backward raises.  Bit-reproducible from run to run.

Out of scope here: the backbone's backward pass (its IR-SE units need batch norm in training mode), the fake-guide step
(coach_new.py:137-151), train_decoder (psp_training_options.py:73 defaults it to False; the generator is frozen), the validation loop
and logging.  The reference's face_pool is the identity for a 256 px generator and is skipped there; a generator of another size is
refused with resize=True, not pooled without a gradient.  Measured deviations and times: profiles/README.md, 'Encoder head training'.
"""
import argparse
import json
import math
import sys

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .psp_encoder import LRELU, DualSpaceEncoder, split_checkpoint
from .frozen_net import check_images, no_gpu

WHO = 'TrainableHeads'
_NO_GPU = no_gpu(WHO)


def head_keys(launch_heads, n_styles, n_spatials, lat1=True, lat2=True):
    """the reference's key names of everything TrainableHeads trains, in no particular order"""
    keys = [f'{kind}.{i}.convs.{2 * k}.{t}' for heads in launch_heads for kind, i, k in heads for t in ('weight', 'bias')]
    keys += [f'{kind}.{i}.linear.{t}' for kind, n in (('styles', n_styles), ('spatials', n_spatials)) for i in range(n) for t in ('weight', 'bias')]
    keys += [f'{name}.{t}' for name, on in (('latlayer1', lat1), ('latlayer2', lat2)) if on for t in ('weight', 'bias')]
    return keys + ['adjust_style.weight', 'adjust_style.bias']


def unpack(named, launch_heads, D, n_styles, n_spatials):
    """tensors laid out as TrainableHeads' parameters (values or gradients) {parameter name: tensor} -> {reference key: tensor}: head g
    of launch n is rows [g*D, (g+1)*D) of h{n}_w and of h{n}_b, head j of the latents' order (styles, then spatials) rows [j*D, (j+1)*D)
    of lin_w and lin_b"""
    out = {}
    for n, heads in enumerate(launch_heads):
        for g, (kind, i, k) in enumerate(heads):
            out[f'{kind}.{i}.convs.{2 * k}.weight'] = named[f'h{n}_w'][g * D:(g + 1) * D]
            out[f'{kind}.{i}.convs.{2 * k}.bias'] = named[f'h{n}_b'][g * D:(g + 1) * D]
    order = [('styles', i) for i in range(n_styles)] + [('spatials', i) for i in range(n_spatials)]
    for j, (kind, i) in enumerate(order):
        out[f'{kind}.{i}.linear.weight'] = named['lin_w'][j * D:(j + 1) * D]
        out[f'{kind}.{i}.linear.bias'] = named['lin_b'][j * D:(j + 1) * D]
    out['adjust_style.weight'], out['adjust_style.bias'] = named['adjust_w'], named['adjust_b']
    for name, key in (('lat1', 'latlayer1'), ('lat2', 'latlayer2')):
        if f'{name}_w' in named:
            out[f'{key}.weight'], out[f'{key}.bias'] = named[f'{name}_w'], named[f'{name}_b']
    return out


def fold(w, scale):
    """EqualLinear's weight as the kernels take it: w * scale formed in fp64, rounded once (psp_encoder.parse_state_dict does the same)"""
    return (w.detach().double() * scale).to(w.dtype)


class _Heads(Function):
    """(c1, c2, c3, *parameters) -> (z_code, p_code) of DualSpaceEncoder's head stage, bit for bit; backward -> the gradients of the
    features and of every parameter"""

    @staticmethod
    def forward(ctx, mod, c1, c2, c3, *params):
        P = dict(zip(mod.names, params))
        D, Ns, Np = mod.dim, mod.n_styles, mod.n_spatials
        B, n = c3.shape[0], Ns + Np
        bufs = {'c3': c3}
        if mod.has_lat1:
            bufs['p2'] = _lib.upsample_add(c3, _lib.conv2d(c2, P['lat1_w'], P['lat1_b'], 1, (0, 0), act=0))
        if mod.has_lat2:
            bufs['p1'] = _lib.upsample_add(bufs['p2'], _lib.conv2d(c1, P['lat2_w'], P['lat2_b'], 1, (0, 0), act=0))
        for i, src, dst, shared, c0, G in mod.program:
            x = bufs[src]
            if dst not in bufs:
                side = (x.shape[2] - 1) // 2 + 1
                bufs[dst] = torch.empty(B, mod.sizes.get(dst, n) * D, side, side, device=x.device, dtype=x.dtype)
            w = P[f'h{i}_w']
            _lib.conv2d_heads(x, w.view(G, D, *w.shape[1:]), P[f'h{i}_b'], 2, (1, 1), shared, LRELU, bufs[dst], c0 * D)
        lin_w = fold(P['lin_w'], mod.lin_scale).view(n, D, D, 1, 1)
        A = fold(P['adjust_w'], mod.adjust_scale)
        lat = _lib.conv2d_heads(bufs['r0'], lin_w, P['lin_b'], 1, (0, 0), False, 1.0).view(B, n, D)
        z, p = _lib.psp_codes(lat, A, P['adjust_b'], Np, None, None)
        ctx.mod, ctx.kept = mod, (P, bufs, c1, c2, lin_w, A, lat)
        return z, p

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, gp):
        mod = ctx.mod
        if ctx.kept is None:
            raise RuntimeError(f'{WHO}: backward through the head stage a second time: its kept activations were freed by the first')
        P, bufs, c1, c2, lin_w, A, lat = ctx.kept
        ctx.kept = None
        need_c1, need_c2, need_c3 = ctx.needs_input_grad[1:4]
        D, Ns, Np = mod.dim, mod.n_styles, mod.n_spatials
        B, n = lat.shape[0], Ns + Np
        grads = {}
        glat, gA, gbz = _lib.psp_codes_bwd(gz.contiguous(), gp.contiguous(), lat, A)
        grads['adjust_w'], grads['adjust_b'] = gA.mul_(mod.adjust_scale), gbz
        # the EqualLinears: 1 x 1 on the 1 x 1 plane; the data gradient enters the last leaky layer, whose output is r0
        r0, g = bufs['r0'], glat.view(B, n * D, 1, 1)
        gw, grads['lin_b'] = _lib.conv2d_heads_wgrad(g, r0, (n, D, D, 1, 1), 1, (0, 0), False)
        grads['lin_w'] = gw.view(n * D, D).mul_(mod.lin_scale)
        G = {'r0': _lib.conv2d_heads_dgrad(g, _lib.heads_dgrad_weight(lin_w, 1, (0, 0)), r0.shape, n, (1, 1), 1, (0, 0), act=r0, slope=LRELU)}
        feat = {}                                            # the gradients of c3 / p2 / p1, accumulated over their consumers
        wanted = {'c3': need_c3, 'p2': True, 'p1': True}
        for i, src, dst, shared, c0, Gn in reversed(mod.program):
            w, x, gd = P[f'h{i}_w'], bufs[src], G[dst]
            Ci = w.shape[1]
            gw, grads[f'h{i}_b'] = _lib.conv2d_heads_wgrad(gd, x, (Gn, D, Ci, 3, 3), 2, (1, 1), shared, c0 * D)
            grads[f'h{i}_w'] = gw.view(Gn * D, Ci, 3, 3)
            if not shared:
                G[src] = _lib.conv2d_heads_dgrad(gd, _lib.heads_dgrad_weight(w.detach().view(Gn, D, Ci, 3, 3), 2, (1, 1)), x.shape, Gn, (3, 3), 2,
                                                 (1, 1), act=x, slope=LRELU, c0=c0 * D)
            elif wanted[src]:                                # the sum over the heads: one convolution with Gn * D output channels
                gs = gd[:, c0 * D:(c0 + Gn) * D].contiguous()
                feat[src] = _lib.conv2d_dgrad(gs, _lib.dgrad_weight(w.detach(), 2, (1, 1)), tuple(x.shape), (3, 3), 2, (1, 1), add=feat.get(src))
        gc = {}
        for name, up, lat_name, c, need in (('p1', 'p2', 'lat2', c1, need_c1), ('p2', 'c3', 'lat1', c2, need_c2)):
            if name not in bufs:
                continue
            lw, gl = P[f'{lat_name}_w'], feat[name]          # p = upsample(the level above) + lateral(c): the lateral's gradient is gl itself
            gw, grads[f'{lat_name}_b'] = _lib.conv2d_heads_wgrad(gl, c, (1, *lw.shape), 1, (0, 0), True)
            grads[f'{lat_name}_w'] = gw.view(lw.shape)
            if need:
                gc[name] = _lib.conv2d_dgrad(gl, _lib.dgrad_weight(lw.detach(), 1, (0, 0)), tuple(c.shape), (1, 1), 1, (0, 0))
            if wanted[up]:
                feat[up] = _lib.upsample_add_bwd(gl, tuple(bufs[up].shape), add=feat.get(up))
        return (None, gc.get('p1'), gc.get('p2'), feat.get('c3') if need_c3 else None, *(grads[k] for k in mod.names))


class TrainableHeads(torch.nn.Module):
    def __init__(self, source=None, state_dict=None, taps=None, units=None):
        """source: a DualSpaceEncoder, or the path of the checkpoint one is built from; or state_dict=, as DualSpaceEncoder takes it"""
        super().__init__()
        if isinstance(source, DualSpaceEncoder):
            if state_dict is not None:
                raise ValueError(f'{WHO}: give an encoder, a path or state_dict, not two of them')
            enc = source
        else:
            kw = {} if taps is None else dict(taps=taps)
            enc = DualSpaceEncoder(source, state_dict=state_dict, units=units, **kw)
        g = enc.geometry
        self.dim, self.n_styles, self.n_spatials, self.tokens = g['D'], g['Ns'], g['Np'], g['T']
        self.sizes, self.program, self.launch_heads = dict(g['sizes']), list(enc.program), list(enc.launch_heads)
        self.lin_scale, self.adjust_scale = 1.0 / math.sqrt(self.dim), 1.0 / math.sqrt(self.n_styles)
        self.has_lat1, self.has_lat2 = enc.lat1_w is not None, enc.lat2_w is not None
        dev = enc.lin_b.device
        n = self.n_styles + self.n_spatials

        def own(t):
            return torch.nn.Parameter(t.detach().to(dev, torch.float32).clone(memory_format=torch.contiguous_format))
        self.names = []
        for i, _, _, _, _, G in self.program:
            w = getattr(enc, f'h{i}_w')
            self._own(f'h{i}_w', own(w.view(G * self.dim, *w.shape[2:])))
            self._own(f'h{i}_b', own(getattr(enc, f'h{i}_b')))
        self._own('lin_w', own(enc.stored['lin_w'].view(n * self.dim, self.dim)))
        self._own('lin_b', own(enc.lin_b))
        self._own('adjust_w', own(enc.stored['A']))
        self._own('adjust_b', own(enc.adjust_b))
        for name, on in (('lat1', self.has_lat1), ('lat2', self.has_lat2)):
            if on:
                self._own(f'{name}_w', own(getattr(enc, f'{name}_w')))
                self._own(f'{name}_b', own(getattr(enc, f'{name}_b')))

    def _own(self, name, p):
        self.register_parameter(name, p)
        self.names.append(name)

    def forward(self, c1, c2, c3):
        """the backbone's features -> (z_code [B,D,T], p_code [B,D,Np]) WITHOUT the latent averages, with a graph to the parameters and to
        the features that require a gradient"""
        if not c3.is_cuda:
            raise RuntimeError(_NO_GPU)
        return _Heads.apply(self, c1, c2, c3, *(getattr(self, k) for k in self.names))

    def reference_keys(self):
        return head_keys(self.launch_heads, self.n_styles, self.n_spatials, self.has_lat1, self.has_lat2)

    def named_by_reference_key(self, grads=False):
        """{reference key: the parameter's slice (or its gradient's)} for every trained tensor"""
        named = {k: (getattr(self, k).grad if grads else getattr(self, k).detach()) for k in self.names}
        return unpack(named, self.launch_heads, self.dim, self.n_styles, self.n_spatials)

    def export_state_dict(self, source_sd):
        """the source ENCODER state dict (or a checkpoint holding one) with every head key replaced by the trained values under the
        reference's key names: loads into DualSpaceEncoder(state_dict=...) and into the reference's load_state_dict(strict=True)"""
        enc = split_checkpoint(source_sd)[0] if 'state_dict' in source_sd else source_sd
        out = dict(enc)
        for key, t in self.named_by_reference_key().items():
            if key not in enc or tuple(enc[key].shape) != tuple(t.shape):
                raise ValueError(f'{WHO}: the source state dict has no {key} of shape {tuple(t.shape)}: not the encoder these heads were built from')
            out[key] = t.cpu().clone()
        return out

    def checkpoint(self, source):
        """the layout coach_new.py:355-371 writes: `source` (the checkpoint the encoder came from, or a bare encoder state dict) with its
        encoder.* entries replaced by export_state_dict's; opts and the latent averages are the source's"""
        sd = self.export_state_dict(source)
        if 'state_dict' not in source:
            return {'state_dict': {f'encoder.{k}': v for k, v in sd.items()}, 'opts': {}}
        out = dict(source)
        out['state_dict'] = dict(source['state_dict'])
        out['state_dict'].update({f'encoder.{k}': v for k, v in sd.items()})
        return out


def generator_decoder(generator, from_plus_space, resize=True):
    """the callable (z_code, p_code) -> images of psp_new.py:111-116 over a frozen generator (its parameters' requires_grad is turned off:
    train_decoder is False).  resize: the reference's face_pool, AdaptiveAvgPool2d((256, 256)): the identity for a 256 px generator, where it
    is skipped; any other size is refused (resize=False renders at the generator's own size, as pSp.forward(resize=False) does)."""
    size = getattr(generator, 'size', None)
    if resize and size != 256:
        raise ValueError(f'generator_decoder: face_pool is the identity for a 256 px generator only; this one is {size} px (resize=False renders '
                         'at its own size)')
    for p in generator.parameters():
        p.requires_grad_(False)
    kw = dict(use_spatial_mapping=False, use_style_mapping=False) if from_plus_space else {}

    def decode(z_code, p_code):
        return generator(z_code, p_code, return_latents=False, **kw)[0]
    return decode


def heads_step(encoder, heads, decode, loss, optimizer, images):
    """one iteration of coach_new.py:128-135 with the backbone frozen -> (loss, loss_dict, id_logs).  encoder: the DualSpaceEncoder the
    heads were built from (its backbone runs under no_grad, its latent averages are added to the codes); decode: a differentiable
    callable (z_code, p_code) -> images; loss: encoder_loss.EncoderLoss."""
    check_images(images, WHO, '[B,3,S,S]', square=True)
    encoder._side(images.shape[2])
    if not images.is_cuda:
        raise RuntimeError(_NO_GPU)
    optimizer.zero_grad()
    with torch.no_grad():
        real = images.detach().float().contiguous()
        c1, c2, c3 = encoder.backbone(real)
    z_code, p_code = heads(c1, c2, c3)
    if encoder.z_avg is not None:                                        # psp_new.py:99-107
        z_code, p_code = z_code + encoder.z_avg, p_code + encoder.p_avg
    inversed = decode(z_code, p_code)
    total, loss_dict, id_logs = loss(real, inversed, z_code, p_code, encoder.z_avg, encoder.p_avg)
    total.backward()
    optimizer.step()
    return total.detach(), loss_dict, id_logs


# ------------------------------------------------------------------------------------------------------------------------ CLI
def build_parser():
    parser = argparse.ArgumentParser(description="fine-tune the heads of the dual-space pSp encoder on a frozen backbone "
                                                 '(pSp/training/coach_new.py:128-135)')
    parser.add_argument('--ckpt', required=True, help='the pSp checkpoint (pSp/training/coach_new.py:355-371) or a bare encoder state dict')
    parser.add_argument('--g_ckpt', required=True, help='the generator checkpoint (256 px)')
    parser.add_argument('--images', required=True, help='a torch file holding [N,3,256,256] images in [-1, 1]')
    parser.add_argument('--steps', type=int, required=True)
    parser.add_argument('--out', required=True, help='the torch file that receives the tuned checkpoint')
    parser.add_argument('--lr', type=float, default=1e-4)
    parser.add_argument('--batch', type=int, default=8)
    parser.add_argument('--id_ckpt', default=None, help='ArcFace IR-SE50 weights: without them id_lambda is 0')
    parser.add_argument('--alexnet', default=None, help="torchvision's AlexNet weights; with --lpips_alex_lin, else lpips_lambda is 0")
    parser.add_argument('--lpips_alex_lin', default=None, help="the LPIPS linear heads for AlexNet")
    parser.add_argument('--w_norm_lambda', type=float, default=0.0)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.batch < 1 or args.steps < 1:
        raise SystemExit('--batch and --steps must be positive')
    if (args.alexnet is None) != (args.lpips_alex_lin is None):
        raise SystemExit('--alexnet and --lpips_alex_lin go together')
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    from .encoder_loss import EncoderLoss
    from .optim import encoder_optimizer
    from .psp_encoder import _generator
    source = torch.load(args.ckpt, map_location='cpu')
    enc = DualSpaceEncoder(state_dict=source)
    heads = TrainableHeads(enc)
    images = torch.load(args.images, map_location='cpu')
    if not torch.is_tensor(images) or images.ndim != 4:
        raise SystemExit('--images must hold one [N,3,S,S] tensor')
    decode = generator_decoder(_generator(enc.opts, args.g_ckpt), enc.from_plus_space)
    id_loss = lpips_loss = None
    if args.id_ckpt:
        from .id_loss import IDLoss
        id_loss = IDLoss(args.id_ckpt)
    if args.alexnet:
        from .lpips_alex import AlexLPIPSLoss
        lpips_loss = AlexLPIPSLoss(args.alexnet, args.lpips_alex_lin)
    lambdas = dict(id_lambda=0.1 if id_loss is not None else 0, l2_lambda=1.0, lpips_lambda=0.8 if lpips_loss is not None else 0,
                   w_norm_lambda=args.w_norm_lambda)
    crit = EncoderLoss(id_loss=id_loss, lpips_loss=lpips_loss, start_from_latent_avg=enc.z_avg is not None, **lambdas)
    opt = encoder_optimizer(heads.parameters(), 'ranger', args.lr)
    first = last = None
    for step in range(args.steps):
        at = step * args.batch % max(images.shape[0] - args.batch + 1, 1)
        _, loss_dict, _ = heads_step(enc, heads, decode, crit, opt, images[at:at + args.batch].to('cuda'))
        first, last = loss_dict if first is None else first, loss_dict
    torch.save(heads.checkpoint(source), args.out)
    print(json.dumps({'tool': 'psp_heads_train', 'steps': args.steps, 'batch': args.batch, 'lr': args.lr, 'optimizer': 'ranger', **lambdas,
                      'dropped_terms': [k for k, v in (('id', id_loss), ('lpips', lpips_loss)) if v is None],
                      'parameters': sum(p.numel() for p in heads.parameters()), 'first': first, 'last': last}))
    return heads


if __name__ == '__main__':
    main(sys.argv[1:])

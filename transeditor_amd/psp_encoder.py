"""Encoder-based inversion on the gfx950 kernels: the reference's dual-space pSp encoder (pSp/models/encoders/psp_encoders_new.py:35-140
GradualStyleEncoder(50, 'ir_se') as pSp/models/psp_new.py:30-121 pSp applies it).  One forward pass turns a real image into (z+, p+):

    enc = DualSpaceEncoder('psp.pt')                                   # a checkpoint as pSp/training/coach_new.py:355-371 writes it
    z_code, p_code = enc.encode(images)                                # [B,3,S,S] in [-1, 1] -> two [B,512,16] tensors on the device
    recon, z_code, p_code = enc.invert(generator, images)              # pSp.forward: the codes and what the generator makes of them
    sweeps = edit.edit_sweep(generator, z_code, p_code, ...)           # the codes are what the editing functions take

    python -m transeditor_amd.psp_encoder --ckpt psp.pt --images X.pt --out codes.pt [--g_ckpt G.pt --recon recon.pt] [--batch 8]

The file is a pSp checkpoint (`state_dict` with encoder.* keys, `opts`, and z_plus_latent_avg / p_plus_latent_avg or z_latent_avg /
p_latent_avg), or a bare encoder state dict; nothing is downloaded.  The geometry is read from the shapes: the units as arcface.ArcFaceID
reads them (irse_units.py: the unit code is shared, not copied), the head width from styles.0.linear.weight, each head's depth from its
convs.{0,2,...} keys, the token counts from adjust_style.weight and the number of spatials.  The spatials and the coarse styles have the
smallest depth d and sit on c3 (the feature after unit taps[2]), the styles with d + 1 convolutions on p2 and those with d + 2 on p1
(psp_encoders_new.py:120-136); styles must come in that order.  A head of depth d needs a plane of 2^d px to reach 1 x 1, so the image
side must bring c3 to 2^d px (256 px for the real file).

Layers: input_layer is te_conv2d_prelu_f32 without the affine (its batch norm folded in), the units are irse_units.unit_forward, the two
laterals te_conv2d_f32 1x1, the two `_upsample_add` te_upsample_add_f32.  The heads run level by level, not head by head: all
convolutions that take a plane of one size are ONE te_conv2d_heads_f32 launch on weights packed at load time into [G, D, Ci, 3, 3] (two
where some heads read a shared feature and the others their own activations; both write slices of one buffer).  The number of launches
does not grow with the number of heads: ten for the real geometry (138 convolutions and 30 linears).  Planes of a few pixels take the
launch's split-K route.  The EqualLinear of every head is one more launch (1 x 1 on the 1 x 1 plane), and te_psp_codes_f32 stacks,
applies adjust_style over the head axis, permutes and adds the latent averages.  An image's codes are bitwise the same whatever batch it
is in.  Eval only here.  Of encoder training (pSp/training/coach_new.py) the loss (encoder_loss.EncoderLoss),
the optimiser (optim.Ranger / optim.encoder_optimizer, section 8k) and the backward pass of everything that sits on the backbone
(psp_heads_train.TrainableHeads, section 8l: the heads can be fine-tuned on a frozen backbone) exist; the backbone's own backward
pass, and with it full encoder training, is still out of scope.  Measured deviations and
times: profiles/README.md, 'Encoder inversion'.
"""
import argparse
import json
import math
import sys

import torch

from . import _lib
from .frozen_net import check_images, no_gpu, resolve, weight_bias
from .irse_units import check_unit_list, parse_stem, parse_units, reader, register_units, unit_forward

WHO = 'DualSpaceEncoder'
TAPS = (6, 20, 23)                                                    # psp_encoders_new.py:112-117
LRELU = 0.01                                                          # nn.LeakyReLU()'s default slope
_NO_GPU = no_gpu(WHO)
_HINT = 'not a GradualStyleEncoder state dict: input_layer.*, body.N.*, styles.N.*, spatials.N.*, latlayer1/2.*, adjust_style.*'
_AVG_KEYS = {True: ('z_plus_latent_avg', 'p_plus_latent_avg'), False: ('z_latent_avg', 'p_latent_avg')}


def split_checkpoint(sd, path='state_dict'):
    """a pSp checkpoint or a bare encoder state dict -> (encoder state dict, opts dict, z_avg, p_avg, from_plus_space).  The averages are
    those psp_new.py:99-107 adds: the pair opts.from_plus_space names, where opts.start_from_latent_avg is set; else None."""
    if 'state_dict' not in sd:
        return sd, {}, None, None, False
    inner = sd['state_dict']
    if not isinstance(inner, dict):
        raise ValueError(f'{WHO}: state_dict of {path} is not a dict')
    enc = {k[len('encoder.'):]: v for k, v in inner.items() if k.startswith('encoder.')}           # psp_new.py:23-27 get_keys
    if not enc:
        raise ValueError(f'{WHO}: state_dict of {path} has no encoder.* keys')
    opts = sd.get('opts', {})
    opts = dict(opts if isinstance(opts, dict) else vars(opts))
    plus = bool(opts.get('from_plus_space', False))
    z_avg = p_avg = None
    if opts.get('start_from_latent_avg', False):
        kz, kp = _AVG_KEYS[plus]
        for k in (kz, kp):
            if k not in sd:
                raise ValueError(f'{WHO}: {path} has no {k}, which opts.start_from_latent_avg with from_plus_space={plus} asks for')
        z_avg, p_avg = sd[kz], sd[kp]
    return enc, opts, z_avg, p_avg, plus


def _head(sd, get, prefix, Cf, D):
    """one GradualStyleBlock -> dict(convs [(w, b)], lin_w, lin_b) as stored"""
    convs = []
    while f'{prefix}.convs.{2 * len(convs)}.weight' in sd or not convs:
        k = f'{prefix}.convs.{2 * len(convs)}'
        convs.append((get(f'{k}.weight', (D, Cf if not convs else D, 3, 3)), get(f'{k}.bias', (D,))))
    return dict(convs=convs, lin_w=get(f'{prefix}.linear.weight', (D, D)), lin_b=get(f'{prefix}.linear.bias', (D,)))


def parse_state_dict(sd, path='state_dict', taps=TAPS, units=None, dtype=torch.float32):
    """an encoder state dict -> dict(stem, units, lat1, lat2 ((w, b) of the laterals), launches, lin (w [G,D,D,1,1], b), A, bz, geometry
    (D, Ns, Np, T, depth, counts (coarse, middle, fine)), keys).  `launches` is the head chain in launch order, each dict(w [G,D,Ci,3,3],
    b [G*D], src, dst, shared, c0 (in heads), heads [(kind, index, convolution)]); a buffer name is 'c3' / 'p2' / 'p1' or 'r<k>', the
    activations of side 2^k.  ValueError naming the key that is missing, misshapen or inconsistent."""
    taps = tuple(int(t) for t in taps)
    if len(taps) != 3 or not 0 <= taps[0] < taps[1] < taps[2]:
        raise ValueError(f'{WHO}: taps must be three ascending unit indices, got {taps!r}')
    get, read = reader(sd, WHO, path, _HINT)
    stem = parse_stem(get, dtype)
    parsed = parse_units(sd, get, stem[0].shape[0], check_unit_list(units, WHO), WHO, path, _HINT, dtype)
    if taps[2] >= len(parsed):
        raise ValueError(f'{WHO}: {path} has {len(parsed)} units (body.0 ... body.{len(parsed) - 1}), the taps {taps} need body.{taps[2]}')
    c1c, c2c, Cf = (parsed[t]['depth'] for t in taps)
    D = get('styles.0.linear.weight', (None, None)).shape[0]
    heads = {'styles': [], 'spatials': []}
    for kind in heads:
        while f'{kind}.{len(heads[kind])}.convs.0.weight' in sd or not heads[kind]:
            heads[kind].append(_head(sd, get, f'{kind}.{len(heads[kind])}', Cf, D))
    Ns, Np = len(heads['styles']), len(heads['spatials'])
    A = get('adjust_style.weight', (None, None))
    T = A.shape[0]
    if A.shape[1] != Ns:
        raise ValueError(f'{WHO}: adjust_style.weight is {tuple(A.shape)}: it mixes {A.shape[1]} styles, {path} has styles.0 ... styles.{Ns - 1}')
    bz = get('adjust_style.bias', (T,))
    d0 = len(heads['spatials'][0]['convs'])
    for i, h in enumerate(heads['spatials']):
        if len(h['convs']) != d0:
            raise ValueError(f'{WHO}: spatials.{i} has {len(h["convs"])} convolutions (convs.{2 * len(h["convs"]) - 2}.weight is its last), '
                             f'spatials.0 has {d0}: all of them sit on one feature')
    depths = [len(h['convs']) for h in heads['styles']]
    for i, d in enumerate(depths):
        if not d0 <= d <= d0 + 2 or (i and d < depths[i - 1]):
            raise ValueError(f'{WHO}: styles.{i} has {d} convolutions (convs.{2 * d - 2}.weight is its last): the styles must have {d0} (coarse), '
                             f'{d0 + 1} (middle) or {d0 + 2} (fine) of them, in this order')
    counts = tuple(sum(d == d0 + k for d in depths) for k in range(3))
    lat1 = lat2 = None
    if counts[1] or counts[2]:
        lat1 = weight_bias(sd, 'latlayer1.weight', 'latlayer1.bias', (Cf, c2c, 1, 1), WHO, path, _HINT)
        read.update(('latlayer1.weight', 'latlayer1.bias'))
    if counts[2]:
        lat2 = weight_bias(sd, 'latlayer2.weight', 'latlayer2.bias', (Cf, c1c, 1, 1), WHO, path, _HINT)
        read.update(('latlayer2.weight', 'latlayer2.bias'))
    lat1, lat2 = (None if t is None else tuple(v.to(dtype).contiguous() for v in t) for t in (lat1, lat2))

    # the order of the heads in every buffer is the order of `lat`: the styles (coarse, middle, fine), then the spatials
    order = [('styles', i) for i in range(Ns)] + [('spatials', i) for i in range(Np)]
    depth_of = {('styles', i): d for i, d in enumerate(depths)}
    depth_of.update({('spatials', i): d0 for i in range(Np)})
    nc, nm, nf = counts
    launches = []

    def launch(group, r, src, dst, shared, c0):
        """the convolution that brings each head of `group` to a plane of 2^r px"""
        if not group:
            return
        ws, bs, names = [], [], []
        for kind, i in group:
            k = depth_of[kind, i] - r - 1
            w, b = heads[kind][i]['convs'][k]
            ws.append(w.detach().to(dtype))
            bs.append(b.detach().to(dtype))
            names.append((kind, i, k))
        launches.append(dict(w=torch.stack(ws).contiguous(), b=torch.cat(bs).contiguous(), src=src, dst=dst, shared=shared, c0=c0, heads=names))
    coarse, middle, fine, spat = order[:nc], order[nc:nc + nm], order[nc + nm:Ns], order[Ns:]
    launch(fine, d0 + 1, 'p1', f'r{d0 + 1}', True, 0)
    launch(middle, d0, 'p2', f'r{d0}', True, 0)
    launch(fine, d0, f'r{d0 + 1}', f'r{d0}', False, nm)
    launch(coarse, d0 - 1, 'c3', f'r{d0 - 1}', True, 0)
    launch(middle + fine, d0 - 1, f'r{d0}', f'r{d0 - 1}', False, nc)
    launch(spat, d0 - 1, 'c3', f'r{d0 - 1}', True, Ns)
    for r in range(d0 - 2, -1, -1):
        launch(order, r, f'r{r + 1}', f'r{r}', False, 0)
    scale = 1.0 / math.sqrt(D)                                                                   # EqualLinear(D, D, lr_mul=1)
    lin_w = torch.stack([(heads[k][i]['lin_w'].detach().double() * scale).to(dtype) for k, i in order]).view(Ns + Np, D, D, 1, 1).contiguous()
    lin_b = torch.cat([heads[k][i]['lin_b'].detach().to(dtype) for k, i in order]).contiguous()
    stored = dict(lin_w=torch.stack([heads[k][i]['lin_w'].detach().to(dtype) for k, i in order]).contiguous(), A=A.detach().to(dtype).contiguous())
    return dict(stem=stem, units=parsed, lat1=lat1, lat2=lat2, launches=launches, lin=(lin_w, lin_b), stored=stored,
                A=(A.detach().double() * (1.0 / math.sqrt(Ns))).to(dtype).contiguous(), bz=bz.detach().to(dtype).contiguous(),
                geometry=dict(D=D, Ns=Ns, Np=Np, T=T, depth=d0, counts=counts, sizes={f'r{d0 + 1}': nf, f'r{d0}': nm + nf}), keys=read)


def _avg(t, name, D, n, path):
    """a latent average [1,D,n] (or [D,n]) -> [D,n] fp32"""
    if not torch.is_tensor(t) or tuple(t.shape) not in ((1, D, n), (D, n)):
        raise ValueError(f'{WHO}: {name} of {path} is {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}, expected (1, {D}, {n})')
    return t.detach().float().reshape(D, n).contiguous()


class DualSpaceEncoder(torch.nn.Module):
    def __init__(self, path=None, state_dict=None, taps=TAPS, units=None):
        super().__init__()
        state_dict, path = resolve(path, state_dict, WHO, 'pSp encoder checkpoint')
        enc, self.opts, z_avg, p_avg, self.from_plus_space = split_checkpoint(state_dict, path)
        net = parse_state_dict(enc, path, taps, units)
        g = net['geometry']
        self.taps, self.keys, self.geometry = tuple(int(t) for t in taps), frozenset(net['keys']), g
        self.dim, self.n_styles, self.n_spatials, self.tokens, self.depth = g['D'], g['Ns'], g['Np'], g['T'], g['depth']
        for name, t in zip(('stem_w', 'stem_b', 'stem_slope', 'lin_w', 'lin_b', 'adjust_w', 'adjust_b'), (*net['stem'], *net['lin'], net['A'], net['bz'])):
            self.register_buffer(name, t)
        register_units(self, net['units'][:self.taps[2] + 1])
        for name, t in (('lat1', net['lat1']), ('lat2', net['lat2'])):
            self.register_buffer(f'{name}_w', None if t is None else t[0])
            self.register_buffer(f'{name}_b', None if t is None else t[1])
        self.register_buffer('z_avg', None if z_avg is None else _avg(z_avg, _AVG_KEYS[self.from_plus_space][0], g['D'], g['T'], path))
        self.register_buffer('p_avg', None if p_avg is None else _avg(p_avg, _AVG_KEYS[self.from_plus_space][1], g['D'], g['Np'], path))
        self.program, self.launch_heads = [], []
        self.stored = net['stored']                                   # EqualLinear weights as the file holds them (CPU): what training starts from
        for n, l in enumerate(net['launches']):
            self.register_buffer(f'h{n}_w', l['w'])
            self.register_buffer(f'h{n}_b', l['b'])
            self.program.append((n, l['src'], l['dst'], l['shared'], l['c0'], len(l['heads'])))
            self.launch_heads.append(tuple(l['heads']))
        self.eval()
        if torch.cuda.is_available():
            self.to('cuda')

    def _side(self, S):
        """the side of c3 for an S px image, after the checks on the pyramid; ValueError where a head would not end at 1 x 1"""
        sides, h = [], S
        for i in range(self.taps[2] + 1):
            h = (h - 1) // self.units[i][2] + 1
            if i in self.taps:
                sides.append(h)
        want = [2 ** (self.depth + k) for k in (2, 1, 0)]
        nc, nm, nf = self.geometry['counts']
        used = [bool(nf), bool(nm or nf), True]
        if any(u and s != w for u, s, w in zip(used, sides, want)):
            raise ValueError(f'{WHO}: a {S} px image gives features of {sides} px after units {self.taps}; heads of {self.depth + 2}, '
                             f'{self.depth + 1} and {self.depth} convolutions need {want} px to end at 1 x 1 (an image of '
                             f'{S * want[2] // max(sides[2], 1)} px would do)')
        return sides[2]

    def heads(self, feats, splits=0):
        """the head chain: feats {'c3', 'p2', 'p1'} -> lat [B, Ns + Np, D]; splits: te_conv2d_heads_f32's (0: its rule, 1: never split),
        or a function (K, Ho * Wo) -> splits that stands in for the rule (measurements)"""
        B, D, n = feats['c3'].shape[0], self.dim, self.n_styles + self.n_spatials
        bufs = dict(feats)
        rule = splits if callable(splits) else (lambda K, HoWo: splits)
        for i, src, dst, shared, c0, G in self.program:
            x = bufs[src]
            if dst not in bufs:
                side = (x.shape[2] - 1) // 2 + 1
                bufs[dst] = torch.empty(B, self.geometry['sizes'].get(dst, n) * D, side, side, device=x.device, dtype=x.dtype)
            w = getattr(self, f'h{i}_w')
            _lib.conv2d_heads(x, w, getattr(self, f'h{i}_b'), 2, (1, 1), shared, LRELU, bufs[dst], c0 * D, rule(w[0, 0].numel(), bufs[dst].shape[2] ** 2))
        lat = _lib.conv2d_heads(bufs['r0'], self.lin_w, self.lin_b, 1, (0, 0), False, 1.0, splits=rule(D, 1))
        return lat.view(B, n, D)

    def backbone(self, images):
        """[B,3,S,S] -> [c1, c2, c3], the features after units taps[0..2]: the seam between the backbone and what sits on it"""
        a = _lib.conv2d_prelu(images, self.stem_w, self.stem_b, self.stem_slope, None, None, 1, (1, 1))
        c = []
        for i in range(self.taps[2] + 1):
            a = unit_forward(self, i, a)
            if i in self.taps:
                c.append(a)
        return c

    def features(self, images):
        """[B,3,S,S] -> {'c3', 'p2', 'p1'} (the latter two where a head reads them)"""
        c = self.backbone(images)
        feats = {'c3': c[2]}
        if self.lat1_w is not None:
            feats['p2'] = _lib.upsample_add(c[2], _lib.conv2d(c[1], self.lat1_w, self.lat1_b, 1, (0, 0), act=0))
        if self.lat2_w is not None:
            feats['p1'] = _lib.upsample_add(feats['p2'], _lib.conv2d(c[0], self.lat2_w, self.lat2_b, 1, (0, 0), act=0))
        return feats

    @torch.no_grad()
    def encode(self, images):
        """[B,3,S,S] in [-1, 1] -> (z_code [B,D,T], p_code [B,D,Np]) fp32 on the device, the latent averages added where the checkpoint
        carries them (pSp.forward(..., only_encode=True))"""
        check_images(images, WHO, '[B,3,S,S]', square=True)
        self._side(images.shape[2])
        if not images.is_cuda:
            raise RuntimeError(_NO_GPU)
        lat = self.heads(self.features(images.detach().float().contiguous()))
        return _lib.psp_codes(lat, self.adjust_w, self.adjust_b, self.n_spatials, self.z_avg, self.p_avg)

    forward = encode

    @torch.no_grad()
    def invert(self, generator, images, resize=False):
        """pSp.forward (psp_new.py:90-121): -> (the generator's images for the codes, z_code, p_code).  Plus-space codes
        (opts.from_plus_space) are rendered with use_style_mapping=False, use_spatial_mapping=False, others through the mappings;
        resize: the reference's face_pool, AdaptiveAvgPool2d((256, 256)).  `generator`: a Generator or a GeneratorSampler over it."""
        from .metrics import _as_sampler
        z_code, p_code = self.encode(images)
        kw = dict(use_style_mapping=False, use_spatial_mapping=False) if self.from_plus_space else {}
        out = _as_sampler(generator)(z_code, p_code, **kw)[0]
        if resize:
            out = _lib.adaptive_avgpool(out, 256, 256)
        return out, z_code, p_code


# ------------------------------------------------------------------------------------------------------------------------ CLI
def build_parser():
    parser = argparse.ArgumentParser(description='invert images into (z, p) codes with the dual-space pSp encoder '
                                                 '(pSp/models/psp_new.py:90-121, pSp/models/encoders/psp_encoders_new.py:35-140)')
    parser.add_argument('--ckpt', required=True, help='the pSp checkpoint (pSp/training/coach_new.py:355-371) or a bare encoder state dict')
    parser.add_argument('--images', required=True, help='a torch file holding [N,3,S,S] images in [-1, 1]')
    parser.add_argument('--out', required=True, help="the torch file that receives {'z_code', 'p_code', 'from_plus_space'}")
    parser.add_argument('--g_ckpt', default=None, help='a generator checkpoint: with --recon, the reconstructions are rendered from the codes')
    parser.add_argument('--recon', default=None, help='the torch file that receives the reconstructions [N,3,size,size] (needs --g_ckpt)')
    parser.add_argument('--batch', type=int, default=8)
    return parser


def _generator(opts, ckpt):
    """the decoder psp_new.py:41-46 builds from the checkpoint's opts, with the weights of `ckpt`"""
    from .model_spatial_query import Generator
    from .train_step import load_checkpoint_into
    size, latent = int(opts.get('size', 256)), int(opts.get('latent', 512))
    g = Generator(size, latent, latent, int(opts.get('token', 2 * (int(math.log(size, 2)) - 1))), channel_multiplier=opts.get('channel_multiplier', 2),
                  layer_noise_injection=opts.get('inject_noise', False), use_spatial_mapping=opts.get('use_spatial_mapping', True),
                  num_region=opts.get('num_region', 1), n_trans=opts.get('num_trans', 8), pixel_norm_op_dim=opts.get('pixel_norm_op_dim', 1),
                  no_trans=opts.get('no_trans', False)).to('cuda')
    load_checkpoint_into(ckpt, g, device='cuda', g_ema_only_ok=True)
    return g.eval()


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.batch < 1:
        raise SystemExit('--batch must be positive')
    if (args.g_ckpt is None) != (args.recon is None):
        raise SystemExit('--g_ckpt and --recon go together')
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    enc = DualSpaceEncoder(args.ckpt)
    images = torch.load(args.images, map_location='cpu')
    if not torch.is_tensor(images) or images.ndim != 4:
        raise SystemExit('--images must hold one [N,3,S,S] tensor')
    g = _generator(enc.opts, args.g_ckpt) if args.g_ckpt else None
    z, p, recon = [], [], []
    for at in range(0, images.shape[0], args.batch):
        x = images[at:at + args.batch].to('cuda')
        if g is None:
            zc, pc = enc.encode(x)
        else:
            im, zc, pc = enc.invert(g, x)
            recon.append(im.cpu())
        z.append(zc.cpu())
        p.append(pc.cpu())
    torch.save({'z_code': torch.cat(z), 'p_code': torch.cat(p), 'from_plus_space': enc.from_plus_space}, args.out)
    if g is not None:
        torch.save(torch.cat(recon), args.recon)
    print(json.dumps({'tool': 'psp_encoder', 'n': int(images.shape[0]), 'side': int(images.shape[2]), 'dim': enc.dim, 'tokens': enc.tokens,
                      'styles': enc.n_styles, 'spatials': enc.n_spatials, 'launches': len(enc.program) + 1,
                      'from_plus_space': enc.from_plus_space, 'latent_avg': enc.z_avg is not None}))
    return torch.cat(z), torch.cat(p)


if __name__ == '__main__':
    main(sys.argv[1:])

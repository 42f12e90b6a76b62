"""Perceptual path length (PPL) of a checkpoint in the z, p and joint latent spaces, and its LPIPS diversity score: the reference's
metrics/evaluate_query.py:135-249 and :82-133 on this project's frozen-generator sampler (transeditor_amd.inference), LPIPS-VGG
(transeditor_amd.lpips) and AlexNet LPIPS (transeditor_amd.lpips_alex).

    python -m transeditor_amd.metrics --ckpt 790000.pt --ppl --vgg16 vgg16-397923af.pth --lpips_lin vgg.pth
    python -m transeditor_amd.metrics --ckpt 790000.pt --lpips --alexnet alexnet-owt-7be5be79.pth --lpips_alex_lin lpips_weights.ckpt

Each sample is the LPIPS distance of two images whose latents are `eps` apart on the path between two random codes, divided by
eps^2.  Hot path: the generator (one captured graph per batch shape), te_crop_resize_bilinear_f32 for the crop / resize to the LPIPS
input, PerceptualLoss.pair_distance (trunk once over the interleaved batch, te_lpips_pair_head_fwd_f32 heads).  The interpolation of
the latents stays in torch with the reference's expressions (:27-43), so `t + eps` and `a + (b - a) * t` round as they do there.

Differences from the reference, all deliberate:
  - the reference appends a remainder batch even when it is empty (:147-149); an empty batch is skipped here;
  - the distances stay on the device until the run ends (no host synchronisation inside the loop);
  - the reference hard-codes 10000 samples in batches of 64 inside evaluate_ppl (:142-143) whatever the command line says; here they
    are arguments with those defaults (--ppl_n_sample, --batch);
  - FID is not run from here (--fid exits with a message): transeditor_amd.fid.  PRDC is built on given features: transeditor_amd.prdc.

The diversity score (evaluate_diversity, --lpips): per iteration three groups of 40 images are drawn and each is scored as the mean of
the AlexNet LPIPS over its 780 pairs; a figure is the mean over the iterations.  The groups, in the reference's draw order (param
before latent, :108-124):
    all     p and z vary                 ('spatial' + 'query')
    same_p  one p for the group, z varies ('spatial_same' + 'query')
    same_z  one z for the group, p varies ('spatial' + 'query_same')
The figures are named by what the group SHARES.  Inside the reference's evaluate_lpips the p-shared group is collected as `fix_z` and
the z-shared one as `fix_p`, the function returns (all, fix_z, fix_p) and its caller (:350) unpacks that as (all, fix_p, fix_z): the two
swaps cancel, so of the three numbers the reference prints after "lpips:" the first is `all`, the second `same_p`, the third `same_z`.
Hot path: the generator, AlexLPIPS.group_mean (the network once over the group, then the all-pairs head te_lpips_allpairs_fwd_f32).
"""
import argparse
import json
import math
import os
import sys
import types

import numpy as np
import torch

from .inference import GeneratorSampler
from .utils.sample import prepare_noise_new, prepare_param

SPACES = ('all', 'z', 'p')
# the diversity score's groups in draw order: (figure, prepare_param method, prepare_noise_new method)  (evaluate_query.py:108-124)
DIVERSITY_GROUPS = (('all', 'spatial', 'query'), ('same_p', 'spatial_same', 'query'), ('same_z', 'spatial', 'query_same'))


def normalize(x):                                                               # :27-28
    return x / torch.sqrt(x.pow(2).sum(-1, keepdim=True))


def slerp(a, b, t):                                                             # :31-39
    a = normalize(a)
    b = normalize(b)
    d = (a * b).sum(-1, keepdim=True)
    p = t * torch.acos(d)
    c = normalize(b - d * a)
    d = a * torch.cos(p) + c * torch.sin(p)

    return normalize(d)


def lerp(a, b, t):                                                              # :42-43
    return a + (b - a) * t


def batch_sizes(n_sample, batch):
    """:147-149 without the empty remainder"""
    if n_sample < 0 or batch <= 0:
        raise ValueError(f'batch_sizes: n_sample >= 0 and batch > 0, got {n_sample}, {batch}')
    n_batch = n_sample // batch
    resid = n_sample - n_batch * batch
    return [batch] * n_batch + ([resid] if resid else [])


def lpips_window(size, crop):
    """(y0, x0, hc, wc, h, w): the window of a size x size image that goes to LPIPS and the shape it is resampled to (:222-232).
    crop: [3c:7c, 2c:6c] with c = size // 8.  factor = window height // 256; only factor > 1 resizes (to 256 x 256), so a cropped
    256 px image reaches LPIPS as 128 x 128."""
    if crop:
        c = size // 8
        y0, x0, hc, wc = 3 * c, 2 * c, 4 * c, 4 * c
    else:
        y0, x0, hc, wc = 0, 0, size, size
    factor = hc // 256
    h, w = (256, 256) if factor > 1 else (hc, wc)
    return y0, x0, hc, wc, h, w


def lpips_input(image, crop):
    """the generator's output [B,3,S,S] -> what the reference hands to LPIPS; the window is read in place by the kernel"""
    from . import _lib
    S = image.shape[2]
    y0, x0, hc, wc, h, w = lpips_window(S, crop)
    if (y0, x0, hc, wc) == (0, 0, h, w) and image.shape[3] == S:
        return image
    if hc % h or wc % w:
        raise ValueError(f'lpips_input: a {hc}x{wc} window is not an integer multiple of {h}x{w}')
    return _lib.crop_resize_bilinear(image, y0, x0, hc, wc, h, w)


def _interpolated(inputs, use_slerp, t, eps):
    """:173-212 for one code: endpoints inputs[::2], inputs[1::2] -> the interleaved codes at t and t + eps"""
    t0, t1 = inputs[::2], inputs[1::2]
    f = slerp if use_slerp else lerp
    e0 = f(t0, t1, t)
    e1 = f(t0, t1, t + eps)
    return torch.stack([e0, e1], 1).view(*inputs.shape)


def _as_sampler(generator):
    return generator if isinstance(generator, GeneratorSampler) else GeneratorSampler(generator)


@torch.no_grad()
def ppl_distances(generator, z, p, *, space, eval_plus, use_slerp, crop, percept, eps=1e-4, t=0.0):
    """The distances [B] (already divided by eps^2) of one batch (:164-236) for the endpoint codes z, p [2B,512,16]: codes 2n and
    2n+1 are the ends of path n.  space 'z' / 'p' interpolates that code only and uses the other one as given.  `t`: a float, or the
    reference's one-element tensor.  `generator`: a Generator or a GeneratorSampler over it."""
    if space not in SPACES:
        raise ValueError(f"ppl_distances: space must be one of {SPACES}, got '{space}'")
    if z.shape[0] % 2 or z.shape[0] != p.shape[0]:
        raise ValueError(f'ppl_distances: z and p hold 2B codes each, got {tuple(z.shape)}, {tuple(p.shape)}')
    g = _as_sampler(generator)
    if eval_plus:
        z, p = g.eager(z, p, return_mapped_codes=True)
    lerp_t = t if torch.is_tensor(t) else torch.full((1,), t, device=z.device, dtype=z.dtype)
    lerped_z = _interpolated(z, use_slerp, lerp_t, eps) if space in ('all', 'z') else z
    lerped_p = _interpolated(p, use_slerp, lerp_t, eps) if space in ('all', 'p') else p
    if not eval_plus:
        image, _, _ = g(lerped_z, lerped_p)
    else:
        image, _, _ = g(lerped_z, lerped_p, use_style_mapping=False, use_spatial_mapping=False)
    return percept.pair_distance(lpips_input(image, crop)) / (eps ** 2)


def filter_mean(distances):
    """:241-249: drop what lies below the 1st percentile ('lower') or above the 99th ('higher'), mean of the rest"""
    distances = np.asarray(distances)
    try:
        lo = np.percentile(distances, 1, method='lower')
        hi = np.percentile(distances, 99, method='higher')
    except TypeError:                                                           # numpy < 1.22
        lo = np.percentile(distances, 1, interpolation='lower')
        hi = np.percentile(distances, 99, interpolation='higher')
    filtered_dist = np.extract(np.logical_and(lo <= distances, distances <= hi), distances)
    return float(filtered_dist.mean())


@torch.no_grad()
def evaluate_ppl(generator, percept, *, space='all', eval_plus=False, use_slerp=False, crop=False, n_sample=10000, batch=64,
                 sampling='end', eps=1e-4, seed=None, latent=512, para_num=16):
    """The reference's loop (:135-249) -> (ppl, distances [n_sample] as a float32 numpy array).  `seed`: draw the codes from a
    generator state of their own (the global random state is left as it was); None uses the global state as the reference does."""
    if space not in SPACES:
        raise ValueError(f"evaluate_ppl: space must be one of {SPACES}, got '{space}'")
    if sampling not in ('end', 'full'):
        raise ValueError(f"evaluate_ppl: sampling must be 'end' or 'full', got '{sampling}'")
    sizes = batch_sizes(n_sample, batch)
    if not sizes:
        raise ValueError('evaluate_ppl: n_sample must be positive')
    g = _as_sampler(generator)
    device = next(g.g.parameters()).device
    args = types.SimpleNamespace(latent=latent, para_num=para_num)
    distances = []
    with torch.random.fork_rng(devices=[device] if device.type == 'cuda' else [], enabled=seed is not None):
        if seed is not None:
            torch.manual_seed(seed)
        for b in sizes:
            if space == 'z':                                                    # fix p
                inputs_z = prepare_noise_new(b * 2, args, device, method='query')
                inputs_p = prepare_param(b * 2, args, device, method='spatial_same')
            elif space == 'p':                                                  # fix z
                inputs_z = prepare_noise_new(b * 2, args, device, method='query_same')
                inputs_p = prepare_param(b * 2, args, device, method='spatial')
            else:
                inputs_z = prepare_noise_new(b * 2, args, device, method='query')
                inputs_p = prepare_param(b * 2, args, device, method='spatial')
            lerp_t = torch.rand(1, device=device) if sampling == 'full' else torch.zeros(1, device=device)
            distances.append(ppl_distances(g, inputs_z, inputs_p, space=space, eval_plus=eval_plus, use_slerp=use_slerp, crop=crop,
                                           percept=percept, eps=eps, t=lerp_t))
    distances = torch.cat(distances).to('cpu').numpy()
    return filter_mean(distances), distances


@torch.no_grad()
def evaluate_diversity(generator, lpips, *, n_iter=1000, group=40, truncation=1.0, seed=None, latent=512, para_num=16):
    """The reference's evaluate_lpips (:94-133) -> {'all', 'same_p', 'same_z': floats, 'per_iteration': {figure: float32 numpy array
    [n_iter]}}.  `lpips`: an AlexLPIPS (anything with group_mean(images) -> 0-d tensor).  Figures are named by what the group shares;
    against the reference's print see the module docstring.  Draw order as the reference's: param before latent, the three groups in
    the order of DIVERSITY_GROUPS.  `seed` as in evaluate_ppl.  The values stay on the device until the run ends."""
    if n_iter < 1 or group < 2:
        raise ValueError(f'evaluate_diversity: n_iter >= 1 and group >= 2, got {n_iter}, {group}')
    g = _as_sampler(generator)
    device = next(g.g.parameters()).device
    args = types.SimpleNamespace(latent=latent, para_num=para_num)
    values = {name: [] for name, _, _ in DIVERSITY_GROUPS}
    with torch.random.fork_rng(devices=[device] if device.type == 'cuda' else [], enabled=seed is not None):
        if seed is not None:
            torch.manual_seed(seed)
        for _ in range(n_iter):
            for name, p_method, z_method in DIVERSITY_GROUPS:
                sample_param = prepare_param(group, args, device, method=p_method) * truncation
                latent_z = prepare_noise_new(group, args, device, method=z_method) * truncation
                img, _, _ = g(latent_z, sample_param)
                values[name].append(lpips.group_mean(img))
    stacked = {name: torch.stack(v).float() for name, v in values.items()}
    out = {name: float(v.mean()) for name, v in stacked.items()}                # (:130-132: the fp32 mean of the stacked values)
    out['per_iteration'] = {name: v.to('cpu').numpy() for name, v in stacked.items()}
    return out


# ------------------------------------------------------------------------------------------------------------------------ CLI
def build_parser(diversity=False):
    """the reference's flags with their names and defaults (:256-288; --inception is not required here: nothing reads it), plus
    --vgg16, --lpips_lin, --ppl_n_sample and --seed; diversity=True (what main() parses with) adds the diversity score's --alexnet,
    --lpips_alex_lin, --lpips_iters and --lpips_group"""
    parser = argparse.ArgumentParser(description='evaluate a checkpoint (metrics/evaluate_query.py): perceptual path length')
    parser.add_argument('--truncation', type=float, default=1)
    parser.add_argument('--truncation_mean', type=int, default=4096)
    parser.add_argument('--batch', type=int, default=64)
    parser.add_argument('--n_sample', type=int, default=50000)
    parser.add_argument('--start_num', type=int, default=0)
    parser.add_argument('--size', type=int, default=256)
    parser.add_argument('--inception', type=str, default=None)
    parser.add_argument('--ckpt', default='./checkpoint')
    parser.add_argument('--dataset', type=str, default='ffhq')
    parser.add_argument('--para_num', type=int, default=16)
    parser.add_argument('--output_dir', type=str, default='./new_generation')
    parser.add_argument('--channel_multiplier', type=int, default=2)
    parser.add_argument('--inject_noise', action='store_true', default=False)
    parser.add_argument('--num_region', type=int, default=1)
    parser.add_argument('--no_spatial_map', action='store_true', default=False)
    parser.add_argument('--num_trans', type=int, default=8)
    parser.add_argument('--no_trans', action='store_true', default=False)
    parser.add_argument('--pixel_norm_op_dim', type=int, default=1)
    parser.add_argument('--fid', action='store_true', default=False)
    parser.add_argument('--lpips', action='store_true', default=False)
    parser.add_argument('--ppl_all', action='store_true', default=False)
    parser.add_argument('--ppl', action='store_true', default=False)
    parser.add_argument('--vgg16', type=str, default=None, help='torchvision vgg16 state dict (default: the torch hub cache path)')
    parser.add_argument('--lpips_lin', type=str, default=None, help='LPIPS v0.1 vgg head weights (weights/v0.1/vgg.pth)')
    parser.add_argument('--ppl_n_sample', type=int, default=10000, help='paths per PPL figure (the reference hard-codes 10000)')
    parser.add_argument('--seed', type=int, default=None, help='draw the codes of every figure from this seed')
    if diversity:
        parser.add_argument('--alexnet', type=str, default=None, help='torchvision alexnet state dict (default: the torch hub cache path)')
        parser.add_argument('--lpips_alex_lin', type=str, default=None, help="the AlexNet LPIPS head file (the reference's metrics/lpips_weights.ckpt)")
        parser.add_argument('--lpips_iters', type=int, default=1000, help='iterations of the diversity score (the reference hard-codes 1000)')
        parser.add_argument('--lpips_group', type=int, default=40, help='images per group (the reference hard-codes 40: 780 pairs)')
    return parser


def ppl_configurations(args):
    """[(space, eval_plus, use_slerp, crop)] in the reference's order: --ppl (:353-364), then --ppl_all (:367-379)"""
    space_list = ['all', 'p', 'z']
    out = []
    if args.ppl:
        out += [(space, True, False, True) for space in space_list]
    if args.ppl_all:
        out += [(space, eval_plus, use_slerp, use_crop) for use_crop in (True, False) for use_slerp in (True, False)
                for eval_plus in (True, False) for space in space_list]
    return out


def checkpoints(ckpt, start_num):
    """:301-307: a directory holds <iteration>.pt files, those from start_num on are evaluated in sorted order"""
    if os.path.isdir(ckpt):
        files = sorted(os.path.join(ckpt, x) for x in os.listdir(ckpt))
        return [x for x in files if int(x.split('/')[-1].split('.')[0]) >= start_num]
    return [ckpt]


def main(argv=None):
    args = build_parser(diversity=True).parse_args(argv)
    if args.fid:
        raise SystemExit('transeditor_amd.metrics: --fid is not built: it needs the patched Inception-v3 network, its weights and the '
                         'dataset statistics file (--inception), none of which this library has')
    if args.lpips and args.lpips_alex_lin is None:
        raise SystemExit("transeditor_amd.metrics: --lpips_alex_lin (the AlexNet LPIPS head file, the reference's metrics/lpips_weights.ckpt) "
                         'is required; nothing is downloaded')
    configs = ppl_configurations(args)
    if not configs and not args.lpips:
        raise SystemExit('transeditor_amd.metrics: nothing to do (give --ppl, --ppl_all or --lpips)')
    if configs and args.lpips_lin is None:
        raise SystemExit('transeditor_amd.metrics: --lpips_lin (the LPIPS v0.1 vgg head file) is required; nothing is downloaded')
    if not torch.cuda.is_available():
        raise RuntimeError('transeditor_amd.metrics needs a GPU (the generator and LPIPS run on the gfx950 kernels only)')
    from .lpips import PerceptualLoss
    from .model_spatial_query import Generator
    from .train_step import load_checkpoint_into
    device = 'cuda'
    args.latent = 512
    args.token = 2 * (int(math.log(args.size, 2)) - 1)
    args.use_spatial_mapping = True                                             # :294 (whatever --no_spatial_map says)
    percept = PerceptualLoss(model='net-lin', net='vgg', use_gpu=True, vgg_path=args.vgg16, lin_path=args.lpips_lin) if configs else None
    alex = None
    if args.lpips:
        from .lpips_alex import AlexLPIPS
        alex = AlexLPIPS(args.alexnet, args.lpips_alex_lin)
    results = []
    for model_path in checkpoints(args.ckpt, args.start_num):
        g = Generator(args.size, args.latent, args.latent, args.token, channel_multiplier=args.channel_multiplier,
                      layer_noise_injection=args.inject_noise, use_spatial_mapping=args.use_spatial_mapping,
                      num_region=args.num_region, n_trans=args.num_trans, pixel_norm_op_dim=args.pixel_norm_op_dim,
                      no_trans=args.no_trans).to(device)
        load_checkpoint_into(model_path, g, device=device, g_ema_only_ok=True)
        sampler = GeneratorSampler(g)
        if alex is not None:                                                    # :348-351
            div = evaluate_diversity(sampler, alex, n_iter=args.lpips_iters, group=args.lpips_group, truncation=1.0, seed=args.seed,
                                     latent=args.latent, para_num=args.para_num)
            res = {'metric': 'lpips_diversity', 'ckpt': model_path, 'n_iter': args.lpips_iters, 'group': args.lpips_group,
                   'all': div['all'], 'same_p': div['same_p'], 'same_z': div['same_z']}
            print(json.dumps(res), flush=True)
            results.append(res)
        for space, eval_plus, use_slerp, crop in configs:
            ppl, _ = evaluate_ppl(sampler, percept, space=space, eval_plus=eval_plus, use_slerp=use_slerp, crop=crop,
                                  n_sample=args.ppl_n_sample, batch=args.batch, seed=args.seed, latent=args.latent,
                                  para_num=args.para_num)
            res = {'metric': 'ppl', 'ckpt': model_path, 'space': space, 'eval_plus': eval_plus, 'use_slerp': use_slerp, 'crop': crop,
                   'n_sample': args.ppl_n_sample, 'batch': args.batch, 'value': ppl}
            print(json.dumps(res), flush=True)
            results.append(res)
    return results


if __name__ == '__main__':
    main(sys.argv[1:])

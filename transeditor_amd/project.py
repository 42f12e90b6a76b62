"""Invert real images into the generator's dual latent space (z+, p+): the reference's projector_optimization.py:152-276, step for
step, on this project's generator, LPIPS-VGG (transeditor_amd.lpips) and noise regulariser (op/noisereg.py).

    python -m transeditor_amd.project --ckpt 790000.pt --dataset_dir images/ --vgg16 vgg16-397923af.pth --lpips_lin vgg.pth

Differences from the reference, all deliberate:
  - the latent statistics (:155-163) are drawn once per call, not once per image (only the use of the random stream differs);
    the reference's unused `param_std` is left out;
  - the loss values recorded every 10 steps stay on the device until the end (no host synchronisation inside the loop);
  - `step < 100` raises ValueError (the reference fails with an IndexError on `latent_path[-1]`);
  - the generator's parameters are frozen for the call (no weight gradients) and restored afterwards;
  - above 256 px the TARGET is mean-pooled to 256 as well (the reference pools only the generated image, :209-216, so its LPIPS and
    MSE terms would fail on mismatched shapes there).
"""
import argparse
import math
import os

import numpy as np
import torch

from .op.weight_cache import packed_weights_cache
from .op.noisereg import noise_normalize_, noise_regularize
from .optim import FusedAdam


def get_lr(t, initial_lr, rampdown=0.25, rampup=0.05):                        # :52-57
    lr_ramp = min(1, (1 - t) / rampdown)
    lr_ramp = 0.5 - 0.5 * math.cos(lr_ramp * math.pi)
    lr_ramp = lr_ramp * min(1, t / rampup)
    return initial_lr * lr_ramp


def make_image(tensor):                                                         # :66-77
    return (tensor.detach().clamp(min=-1, max=1).add(1).div_(2).mul(255).type(torch.uint8).permute(0, 2, 3, 1).to('cpu').numpy())


def _downsample_256(img):                                                       # :209-216
    batch, channel, height, width = img.shape
    if height > 256:
        factor = height // 256
        img = img.reshape(batch, channel, height // factor, factor, width // factor, factor).mean([3, 5])
    return img


def step_loss(g_ema, latent_in, param_in, noises, percept, tf, target, a, strength=None):
    """the loss of one step (:199-229) -> (loss, p_loss, n_loss, mse_loss); `strength` [512]: the latent noise (use_noise only)"""
    if a['use_noise']:
        latent_n = latent_in + torch.randn_like(latent_in) * strength.unsqueeze(-1) if strength is not None else latent_in
        img_gen, _, _ = g_ema(latent_n, param_in, use_spatial_mapping=False, use_style_mapping=False, noise=noises)
    else:
        img_gen, _, _ = g_ema(latent_in, param_in, use_spatial_mapping=False, use_style_mapping=False)
    img_gen = _downsample_256(img_gen)
    p_loss = percept(img_gen, tf).sum()
    n_loss = noise_regularize(noises)
    mse_loss = (img_gen - target).pow(2).mean()
    if a['use_noise']:
        loss = p_loss + a['noise_regularize'] * n_loss + a['mse'] * mse_loss
    else:
        loss = p_loss + a['mse'] * mse_loss
    return loss, p_loss, n_loss, mse_loss


def _one_image(g_ema, target, percept, stats, noise_single, a):
    latent_mean, latent_std, param_mean = stats
    batch = a['batch']
    noises = [n.repeat(batch, 1, 1, 1).normal_() for n in noise_single]
    latent_in = latent_mean.detach().clone().unsqueeze(0).repeat(batch, 1, 1).requires_grad_(True)
    param_in = param_mean.detach().clone().unsqueeze(0).repeat(batch, 1, 1).requires_grad_(True)
    for n in noises:
        n.requires_grad_(a['use_noise'])
    opt = FusedAdam([latent_in, param_in] + (noises if a['use_noise'] else []), lr=a['lr'])
    target = _downsample_256(target)
    tf = percept.target_features(target)
    n_rec = a['step'] // 10
    trace = torch.zeros(3, max(n_rec, 1), device=target.device)
    last = None
    for i in range(a['step']):
        t = i / a['step']
        opt.param_groups[0]['lr'] = get_lr(t, a['lr'], rampdown=a['lr_rampdown'], rampup=a['lr_rampup'])
        strength = latent_std * a['noise'] * max(0, 1 - t / a['noise_ramp']) ** 2 if a['use_noise'] else None
        loss, p_loss, n_loss, mse_loss = step_loss(g_ema, latent_in, param_in, noises, percept, tf, target, a, strength)
        opt.zero_grad()
        loss.backward()
        opt.step()
        noise_normalize_(noises)
        if (i + 1) % 100 == 0:
            last = (latent_in.detach().clone(), param_in.detach().clone())
        if (i + 1) % 10 == 0:
            trace[:, (i + 1) // 10 - 1] = torch.stack([p_loss.detach(), n_loss.detach(), mse_loss.detach()])
    with torch.no_grad():
        kw = dict(noise=noises) if a['use_noise'] else {}
        img, _, _ = g_ema(last[0], last[1], use_spatial_mapping=False, use_style_mapping=False, **kw)
    return last[0], last[1], [n.detach() for n in noises], img, trace[:, :n_rec]


def project(g_ema, imgs, percept, *, step=10000, lr=0.1, lr_rampup=0.05, lr_rampdown=0.25, noise=0.05, noise_ramp=0.75,
            noise_regularize=1e5, mse=0.0, batch=1, use_noise=False, truncation=1.0, n_mean_latent=10000, seed=0, para_num=16):
    """Project each image of imgs [n,3,H,W] (in [-1, 1]) separately, `batch` candidates per image.  `para_num`: the token count of
    the codes drawn for the latent statistics (prepare_noise_new / prepare_param with args.para_num, :155-156).
    -> dict(latent [n*batch,512,16], param [n*batch,512,16], noises (maps of the last image), image [n*batch,3,size,size],
            perceptual / noise / mse: [n, step // 10] loss traces)"""
    if step < 100:
        raise ValueError(f'project: step must be >= 100 (the result is the snapshot at the last multiple of 100), got {step}')
    a = dict(step=step, lr=lr, lr_rampup=lr_rampup, lr_rampdown=lr_rampdown, noise=noise, noise_ramp=noise_ramp,
             noise_regularize=noise_regularize, mse=mse, batch=batch, use_noise=use_noise)
    dev = imgs.device
    params = list(g_ema.parameters())
    flags = [p.requires_grad for p in params]
    out = dict(latent=[], param=[], image=[], perceptual=[], noise=[], mse=[], noises=None)
    try:
        for p in params:
            p.requires_grad_(False)
        with torch.random.fork_rng(devices=[dev] if dev.type == 'cuda' else []), packed_weights_cache({}):
            torch.manual_seed(seed)
            with torch.no_grad():                                               # :155-163, once per call
                latent_dim = 512
                noise_sample = torch.randn(n_mean_latent, latent_dim, para_num, device=dev) * truncation
                para_base = torch.randn(n_mean_latent, latent_dim, para_num, device=dev) * truncation
                z_plus = g_ema(noise_sample, para_base, return_only_mapped_z=True)
                p_plus = g_ema(noise_sample, para_base, return_only_mapped_p=True)
                latent_mean = z_plus.mean(0)
                latent_std = ((z_plus - latent_mean).pow(2).sum([0, 2]) / n_mean_latent) ** 0.5
                param_mean = p_plus.mean(0)
                del z_plus, p_plus, noise_sample, para_base
            noise_single = g_ema.make_noise()
            for k in range(imgs.shape[0]):
                lat, par, noises, img, trace = _one_image(g_ema, imgs[k:k + 1].contiguous(), percept,
                                                          (latent_mean, latent_std, param_mean), noise_single, a)
                out['latent'].append(lat)
                out['param'].append(par)
                out['image'].append(img)
                out['noises'] = noises
                for j, key in enumerate(('perceptual', 'noise', 'mse')):
                    out[key].append(trace[j])
    finally:
        for p, f in zip(params, flags):
            p.requires_grad_(f)
    for key in ('latent', 'param', 'image', 'perceptual', 'noise', 'mse'):
        out[key] = torch.cat(out[key]) if key in ('latent', 'param', 'image') else torch.stack(out[key])
    return out


# ------------------------------------------------------------------------------------------------------------------------ CLI
def build_parser():
    """the reference's flags with their names and defaults (:83-106), plus --vgg16, --lpips_lin and --seed"""
    parser = argparse.ArgumentParser(description='invert images into (z+, p+) (projector_optimization.py)')
    parser.add_argument('--ckpt', type=str, required=True)
    parser.add_argument('--dataset_dir', type=str, required=True)
    parser.add_argument('--size', type=int, default=256)
    parser.add_argument('--para_num', type=int, default=16)
    parser.add_argument('--lr_rampup', type=float, default=0.05)
    parser.add_argument('--lr_rampdown', type=float, default=0.25)
    parser.add_argument('--lr', type=float, default=0.1)
    parser.add_argument('--noise', type=float, default=0.05)
    parser.add_argument('--noise_ramp', type=float, default=0.75)
    parser.add_argument('--step', type=int, default=10000)
    parser.add_argument('--noise_regularize', type=float, default=1e5)
    parser.add_argument('--mse', type=float, default=0)
    parser.add_argument('--batch', type=int, default=1)
    parser.add_argument('--output_dir', type=str, default='./projection/optimization')
    parser.add_argument('--pixel_norm_op_dim', type=int, default=1)
    parser.add_argument('--num_trans', type=int, default=8)
    parser.add_argument('--old_version', action='store_true', default=False)
    parser.add_argument('--n_mlp', type=int, default=8)
    parser.add_argument('--truncation', type=float, default=1.0)
    parser.add_argument('--use_noise', action='store_true', default=False)
    parser.add_argument('--no_trans', action='store_true', default=False)
    parser.add_argument('--no_spatial_map', action='store_true', default=False)
    parser.add_argument('--num_region', type=int, default=1)
    parser.add_argument('--inject_noise', action='store_true', default=False)
    parser.add_argument('--channel_multiplier', type=int, default=2)
    parser.add_argument('--vgg16', type=str, default=None, help='torchvision vgg16 state dict (default: the torch hub cache path)')
    parser.add_argument('--lpips_lin', type=str, required=True, help='LPIPS v0.1 vgg head weights (weights/v0.1/vgg.pth)')
    parser.add_argument('--seed', type=int, default=0)
    return parser


def load_image(path, size):
    """utils/dataset_projector.py: Resize(size) (shorter side to `size`, bilinear, as torchvision does on a PIL image), ToTensor,
    Normalize(0.5, 0.5) -> [3, h, w] in [-1, 1]"""
    from PIL import Image
    img = Image.open(path).convert('RGB')
    w, h = img.size
    short, long = (w, h) if w <= h else (h, w)
    if short != size:
        new_short, new_long = size, int(size * long / short)
        img = img.resize((new_short, new_long) if w <= h else (new_long, new_short), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255)
    return (x - 0.5) / 0.5


def output_dir_for(output_dir, ckpt):
    """:137-141: <output_dir>/<experiment>/<iteration> for a '<exp>/checkpoint/<iteration>.pt' path, else <output_dir>/<file stem>"""
    stem = os.path.splitext(os.path.basename(ckpt))[0]
    parts = str(ckpt).split('/')
    try:
        return os.path.join(output_dir, parts[-3], f'{int(stem)}') if len(parts) >= 3 else os.path.join(output_dir, stem)
    except ValueError:
        return os.path.join(output_dir, stem)


def main(argv=None):
    from PIL import Image
    from .lpips import PerceptualLoss
    from .model_spatial_query import Generator
    from .train_step import load_checkpoint_into
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('transeditor_amd.project needs a GPU (the generator and LPIPS run on the gfx950 kernels only)')
    device = 'cuda'
    args.latent = 512
    args.token = 2 * (int(math.log(args.size, 2)) - 1)
    g_ema = Generator(args.size, args.latent, args.latent, args.token, channel_multiplier=args.channel_multiplier,
                      layer_noise_injection=args.inject_noise, use_spatial_mapping=not args.no_spatial_map, num_region=args.num_region,
                      n_trans=args.num_trans, pixel_norm_op_dim=args.pixel_norm_op_dim, no_trans=args.no_trans).to(device)
    load_checkpoint_into(args.ckpt, g_ema, device=device, g_ema_only_ok=True)
    g_ema.eval()
    sample_path = output_dir_for(args.output_dir, args.ckpt)
    os.makedirs(sample_path, exist_ok=True)
    files = [os.path.join(args.dataset_dir, f) for f in sorted(os.listdir(args.dataset_dir))]
    percept = PerceptualLoss(model='net-lin', net='vgg', use_gpu=True, vgg_path=args.vgg16, lin_path=args.lpips_lin)
    imgs = torch.stack([load_image(f, args.size) for f in files]).to(device)
    res = project(g_ema, imgs, percept, step=args.step, lr=args.lr, lr_rampup=args.lr_rampup, lr_rampdown=args.lr_rampdown,
                  noise=args.noise, noise_ramp=args.noise_ramp, noise_regularize=args.noise_regularize, mse=args.mse, batch=args.batch,
                  use_noise=args.use_noise, truncation=args.truncation, seed=args.seed, para_num=args.para_num)
    img_or, img_ar = make_image(imgs), make_image(res['image'])
    for it in range(len(files)):
        Image.fromarray(img_or[it]).save(os.path.join(sample_path, f'origin_{it}.png'))
        Image.fromarray(img_ar[it * args.batch]).save(os.path.join(sample_path, f'project_{it}.png'))
    print('res_latent.shape', res['latent'].shape)
    print('res_param.shape', res['param'].shape)
    np.save(os.path.join(sample_path, 'latents.npy'), res['latent'].cpu().numpy())
    np.save(os.path.join(sample_path, 'param.npy'), res['param'].cpu().numpy())
    np.save(os.path.join(sample_path, 'perceptual.npy'), res['perceptual'][:, -1].cpu().numpy().tolist())
    np.save(os.path.join(sample_path, 'noise.npy'), res['noise'][:, -1].cpu().numpy().tolist())
    np.save(os.path.join(sample_path, 'mse.npy'), res['mse'][:, -1].cpu().numpy().tolist())
    return sample_path


if __name__ == '__main__':
    main()

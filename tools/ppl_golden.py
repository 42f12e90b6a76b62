"""Writes tests/golden/ppl64.json: the yardstick of the PPL check in tests/test_gpu_ppl.py.  CPU only, a few minutes.

    python tools/ppl_golden.py [--out tests/golden/ppl64.json]

For a 64 px, 8-block generator with synthetic weights (synth.fill_state_dict, seed 21), random LPIPS weights
(lpips_restated.write_weights, seed 1) and fixed endpoint codes (synth.latents, seed 5; 4 paths per configuration), the PPL distances
of all 24 configurations (space x eval_plus x slerp x crop) are computed twice by one restatement of metrics/evaluate_query.py:164-236
on the CPU oracle (oracle.te_oracle) and the restated LPIPS (tests/lpips_restated.py): everything in float64 from the endpoint codes
on, and everything in float32.  Stored: the float64 distances and the float32 run's deviation from them, per sample, relative to the
float64 distance.  The float32 run is the reference's own arithmetic in its own precision; what it loses against float64 is what a
correct fp32 implementation may lose, and the test allows the library twice the largest such loss (two correct fp32 evaluations
differ by rounding order).
"""
import argparse
import itertools
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

SIZE, PATHS, G_SEED, LPIPS_SEED, LATENT_SEED, EPS = 64, 4, 21, 1, 5, 1e-4
CONFIGS = list(itertools.product(('all', 'z', 'p'), (True, False), (False, True), (True, False)))   # space, eval_plus, slerp, crop


def endpoint_codes(space, paths=PATHS, seed=LATENT_SEED):
    """z, p [2 * paths, 512, 16] as the reference draws them (:154-162): the code a space holds fixed is one code repeated"""
    from transeditor_amd import synth
    z, p = synth.latents(2 * paths, seed)
    if space == 'z':
        p = p[:1].repeat(2 * paths, 1, 1)
    if space == 'p':
        z = z[:1].repeat(2 * paths, 1, 1)
    return z, p


def normalize(x):
    return x / torch.sqrt(x.pow(2).sum(-1, keepdim=True))


def slerp(a, b, t):
    a = normalize(a)
    b = normalize(b)
    d = (a * b).sum(-1, keepdim=True)
    p = t * torch.acos(d)
    c = normalize(b - d * a)
    d = a * torch.cos(p) + c * torch.sin(p)
    return normalize(d)


def lerp(a, b, t):
    return a + (b - a) * t


def oracle_distances(P, vgg_sd, lin_sd, z, p, space, eval_plus, use_slerp, crop, dtype):
    """evaluate_query.py:164-236 on the CPU oracle in `dtype`, t = 0"""
    import torch.nn.functional as F
    import lpips_restated as R
    from oracle import te_oracle as O
    P = {k: v.to(dtype) if v.is_floating_point() else v for k, v in P.items()}
    vgg_sd = {k: v.to(dtype) for k, v in vgg_sd.items()}
    lin_sd = {k: v.to(dtype) for k, v in lin_sd.items()}
    z, p = z.to(dtype), p.to(dtype)
    with torch.no_grad():
        if eval_plus:
            _, _, z, p, _ = O.generator_latent(P, z, p, pixel_norm_dim=1)
        t = torch.zeros(1, dtype=dtype)
        f = slerp if use_slerp else lerp

        def inter(x):
            return torch.stack([f(x[::2], x[1::2], t), f(x[::2], x[1::2], t + EPS)], 1).view(*x.shape)
        lz = inter(z) if space in ('all', 'z') else z
        lp = inter(p) if space in ('all', 'p') else p
        image = O.generator_forward(P, lz, lp, SIZE, pixel_norm_dim=1, use_spatial_mapping=not eval_plus,
                                    use_style_mapping=not eval_plus)[0]
        if crop:
            c = image.shape[2] // 8
            image = image[:, :, c * 3:c * 7, c * 2:c * 6]
        factor = image.shape[2] // 256
        if factor > 1:
            image = F.interpolate(image, size=(256, 256), mode='bilinear', align_corners=False)
        return R.lpips(image[::2], image[1::2], vgg_sd, lin_sd).view(image.shape[0] // 2) / (EPS ** 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'ppl64.json'))
    a = ap.parse_args()
    import pathlib
    import lpips_restated as R
    from transeditor_amd import synth
    from transeditor_amd.model_spatial_query import Generator
    G = Generator(SIZE, 512, 512, 2 * (SIZE.bit_length() - 2), n_trans=8, pixel_norm_op_dim=1)
    sd = G.state_dict()
    synth.fill_state_dict(sd, G_SEED)
    vp, lp = R.write_weights(pathlib.Path(tempfile.mkdtemp()), seed=LPIPS_SEED)
    vgg_sd, lin_sd = torch.load(vp), torch.load(lp)
    out = {'size': SIZE, 'paths': PATHS, 'generator_seed': G_SEED, 'lpips_seed': LPIPS_SEED, 'latent_seed': LATENT_SEED, 'eps': EPS,
           'configs': []}
    worst = 0.0
    for space, eval_plus, use_slerp, crop in CONFIGS:
        z, p = endpoint_codes(space)
        d64 = oracle_distances(sd, vgg_sd, lin_sd, z, p, space, eval_plus, use_slerp, crop, torch.float64)
        d32 = oracle_distances(sd, vgg_sd, lin_sd, z, p, space, eval_plus, use_slerp, crop, torch.float32)
        dev = ((d32.double() - d64) / d64).abs()
        worst = max(worst, float(dev.max()))
        out['configs'].append({'space': space, 'eval_plus': eval_plus, 'use_slerp': use_slerp, 'crop': crop,
                               'fp64': [float(x) for x in d64], 'fp32_rel_dev': [float(x) for x in dev]})
        print(f'{space:3s} plus={eval_plus!s:5s} slerp={use_slerp!s:5s} crop={crop!s:5s}  fp64 {[f"{float(x):.4g}" for x in d64]}  '
              f'fp32 rel dev {[f"{float(x):.2e}" for x in dev]}', flush=True)
    out['fp32_max_rel_dev'] = worst
    print(f'largest fp32 deviation: {worst:.3e}')
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()

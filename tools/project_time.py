"""Step time of the projector (transeditor_amd.project) on the MI355X: a 256-px, 8-block generator (random weights, or --ckpt) with
random LPIPS weights, batches 1 and 4.

    python tools/project_time.py [--ckpt 790000.pt] [--steps 200] [--warmup 20] [--out profiles/project_time.json] [--steps-only]

Per batch: (1) ms per projector step over `steps` steps between two device synchronisations after `warmup` steps; (2) a second run
with events around the generator forward+backward, the LPIPS forward+backward and Adam + noise normalisation; (3) alternating, the
HIP LPIPS forward+backward against a plain-torch (MIOpen) restatement at 256^2.  Both sides of (3) get the target's normalised
tap features computed once beforehand, so each call is one trunk forward + data gradient over the pred batch and the five heads.
--steps-only: (1) alone (for kernel traces: two runs with different --steps give the dispatches of one step).  GPU only.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ckpt', default=None)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batches', default='1,4')
    ap.add_argument('--out', default=None)
    ap.add_argument('--steps-only', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('project_time.py needs a GPU')
    import lpips_restated as R
    from transeditor_amd import synth
    from transeditor_amd.lpips import PerceptualLoss
    from transeditor_amd.model_spatial_query import Generator
    from transeditor_amd.op.noisereg import noise_normalize_
    from transeditor_amd.op.weight_cache import packed_weights_cache
    from transeditor_amd.optim import FusedAdam
    from transeditor_amd.project import get_lr, step_loss
    dev = 'cuda'
    G = Generator(256, 512, 512, 14, n_trans=8, pixel_norm_op_dim=1)
    if a.ckpt:
        from transeditor_amd.train_step import load_checkpoint_into
        load_checkpoint_into(a.ckpt, G, g_ema_only_ok=True)
    else:
        sd = G.state_dict()
        synth.fill_state_dict(sd, 3)
        G.load_state_dict(sd)
    G = G.to(dev)
    for p in G.parameters():
        p.requires_grad_(False)
    tmp = tempfile.mkdtemp()
    vp, lp = R.write_weights(__import__('pathlib').Path(tmp))
    percept = PerceptualLoss(vgg_path=vp, lin_path=lp)
    vgg_sd = {k: v.to(dev) for k, v in torch.load(vp).items()}
    lin_sd = {k: v.to(dev) for k, v in torch.load(lp).items()}
    shown = [x for i, x in enumerate(sys.argv[1:]) if x != '--out' and (i == 0 or sys.argv[i] != '--out')]     # (where it was written to is not part of the run)
    res = {'command': ' '.join(['python tools/project_time.py'] + shown), 'size': 256, 'steps': a.steps, 'warmup': a.warmup,
           'batches': {}}
    torch.manual_seed(0)
    target = torch.rand(1, 3, 256, 256, device=dev) * 2 - 1
    for B in [int(b) for b in a.batches.split(',')]:
        cfg = dict(use_noise=True, noise_regularize=1e5, mse=0.0)
        latent_in = torch.randn(B, 512, 16, device=dev, requires_grad=True)
        param_in = torch.randn(B, 512, 16, device=dev, requires_grad=True)
        noises = [n.repeat(B, 1, 1, 1).normal_().requires_grad_(True) for n in G.make_noise()]
        latent_std = torch.ones(512, device=dev)
        opt = FusedAdam([latent_in, param_in] + noises, lr=0.1)
        tf = percept.target_features(target)
        ev = {}

        def step(i, n, split=False):
            t = i / max(n, 1)
            opt.param_groups[0]['lr'] = get_lr(t, 0.1)
            strength = latent_std * 0.05 * max(0, 1 - t / 0.75) ** 2
            if split:
                e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
                e[0].record()
                latent_n = latent_in + torch.randn_like(latent_in) * strength.unsqueeze(-1)
                img = G(latent_n, param_in, use_spatial_mapping=False, use_style_mapping=False, noise=noises)[0]
                e[1].record()
                img_d = img.detach().requires_grad_(True)
                p_loss = percept(img_d, tf).sum()
                p_loss.backward()
                e[2].record()
                from transeditor_amd.op.noisereg import noise_regularize
                loss = (img * img_d.grad).sum() + 1e5 * noise_regularize(noises)
                e[3].record()
                opt.zero_grad()
                loss.backward()
                e[4].record()
                opt.step()
                noise_normalize_(noises)
                e[5].record()
                ev.setdefault('gen_fwd', []).append((e[0], e[1]))
                ev.setdefault('lpips_fwd_bwd', []).append((e[1], e[2]))
                ev.setdefault('gen_bwd_and_noise_reg', []).append((e[2], e[4]))
                ev.setdefault('adam_and_noise_normalize', []).append((e[4], e[5]))
                return
            loss = step_loss(G, latent_in, param_in, noises, percept, tf, target, cfg, strength)[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
            noise_normalize_(noises)

        with packed_weights_cache({}):
            for i in range(a.warmup):
                step(i, a.steps)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(a.steps):
                step(i, a.steps)
            e.record()
            torch.cuda.synchronize()
            ms_step = s.elapsed_time(e) / a.steps
            if a.steps_only:
                res['batches'][B] = {'ms_per_step': ms_step}
                print(f'batch {B}: {ms_step:.2f} ms/step', flush=True)
                continue
            for i in range(a.steps):
                step(i, a.steps, split=True)
            torch.cuda.synchronize()
        split = {k: sum(x.elapsed_time(y) for x, y in v) / len(v) for k, v in ev.items()}
        # HIP LPIPS forward + backward vs the plain-torch (MIOpen) restatement, alternating
        pred = torch.rand(B, 3, 256, 256, device=dev) * 2 - 1
        with torch.no_grad():
            t_taps = R.target_taps(target, vgg_sd)              # the plain side's cached target, as `tf` is the HIP side's

        def hip():
            x = pred.clone().requires_grad_(True)
            percept(x, tf).sum().backward()

        def plain():
            x = pred.clone().requires_grad_(True)
            R.lpips_from_taps(x, t_taps, vgg_sd, lin_sd).sum().backward()
        times = {'hip': [], 'torch_miopen': []}
        for f in (hip, plain, hip, plain):
            f()
        torch.cuda.synchronize()
        for _ in range(5):
            for name, f in (('hip', hip), ('torch_miopen', plain)):
                s.record()
                for _ in range(10):
                    f()
                e.record()
                torch.cuda.synchronize()
                times[name].append(s.elapsed_time(e) / 10)
        res['batches'][B] = {'ms_per_step': ms_step, 'split_ms': split,
                             'lpips_fwd_bwd_ms': {k: sorted(v)[len(v) // 2] for k, v in times.items()},
                             'lpips_fwd_bwd_ms_all': times}
        print(f'batch {B}: {ms_step:.2f} ms/step; split {json.dumps({k: round(v, 3) for k, v in split.items()})}; '
              f'LPIPS fwd+bwd median ms {json.dumps({k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()})}', flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

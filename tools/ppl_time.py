"""Time of a perceptual-path-length run (transeditor_amd.metrics.evaluate_ppl) on the MI355X: a 256-px, 8-block generator (random
weights, or --ckpt) with random LPIPS weights, space 'all', eval_plus, lerp, crop, batch 64.

    python tools/ppl_time.py [--ckpt 790000.pt] [--n-sample 144] [--batch 64] [--reps 5] [--out profiles/ppl/ppl_time.json] [--only new]

Two loops over the same codes, timed alternately between device synchronisations after every batch shape has run once on both:
  new      : evaluate_ppl (GeneratorSampler graphs, te_crop_resize_bilinear_f32, PerceptualLoss.pair_distance);
  baseline : the same loop from the pieces the library had before the metric: the eager generator, the crop as a torch slice, and
             percept(image[::2], image[1::2]) (target_features + forward: the trunk twice over half the batch, the normalised
             target features written and read back).
--only new: the new loop alone, `reps` times (for `rocprofv3 --kernel-trace --stats`).  GPU only.
"""
import argparse
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ckpt', default=None)
    ap.add_argument('--n-sample', type=int, default=144)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', choices=['new'], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ppl_time.py needs a GPU')
    import lpips_restated as R
    from transeditor_amd import metrics, synth
    from transeditor_amd.inference import GeneratorSampler
    from transeditor_amd.lpips import PerceptualLoss
    from transeditor_amd.model_spatial_query import Generator
    from transeditor_amd.utils.sample import prepare_noise_new, prepare_param
    dev = 'cuda'
    G = Generator(256, 512, 512, 14, n_trans=8, pixel_norm_op_dim=1)
    if a.ckpt:
        from transeditor_amd.train_step import load_checkpoint_into
        load_checkpoint_into(a.ckpt, G, g_ema_only_ok=True)
    else:
        sd = G.state_dict()
        synth.fill_state_dict(sd, 3)
        G.load_state_dict(sd)
    G = G.to(dev).eval()
    for p in G.parameters():
        p.requires_grad_(False)
    vp, lp = R.write_weights(__import__('pathlib').Path(tempfile.mkdtemp()))
    percept = PerceptualLoss(vgg_path=vp, lin_path=lp)
    sampler = GeneratorSampler(G)
    kw = dict(space='all', eval_plus=True, use_slerp=False, crop=True, n_sample=a.n_sample, batch=a.batch, seed=1)
    eps = 1e-4

    def new():
        return metrics.evaluate_ppl(sampler, percept, **kw)

    @torch.no_grad()
    def baseline():
        args = types.SimpleNamespace(latent=512, para_num=16)
        out = []
        with torch.random.fork_rng(devices=[torch.device(dev, 0)]):
            torch.manual_seed(kw['seed'])
            for b in metrics.batch_sizes(a.n_sample, a.batch):
                z = prepare_noise_new(b * 2, args, dev, method='query')
                p = prepare_param(b * 2, args, dev, method='spatial')
                z, p = G(z, p, return_mapped_codes=True)
                t = torch.zeros(1, device=dev)
                lz = torch.stack([metrics.lerp(z[::2], z[1::2], t), metrics.lerp(z[::2], z[1::2], t + eps)], 1).view(*z.shape)
                lp_ = torch.stack([metrics.lerp(p[::2], p[1::2], t), metrics.lerp(p[::2], p[1::2], t + eps)], 1).view(*p.shape)
                image, _, _ = G(lz, lp_, use_style_mapping=False, use_spatial_mapping=False)
                c = image.shape[2] // 8
                image = image[:, :, c * 3:c * 7, c * 2:c * 6]
                if image.shape[2] // 256 > 1:
                    image = F.interpolate(image, size=(256, 256), mode='bilinear', align_corners=False)
                out.append(percept(image[::2], image[1::2]).view(b) / (eps ** 2))
        d = torch.cat(out).to('cpu').numpy()
        return metrics.filter_mean(d), d

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(f):
        torch.cuda.synchronize()
        s.record()
        r = f()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), r

    if a.only == 'new':
        new()
        ts = [timed(new)[0] for _ in range(a.reps)]
        print(f'new: ms per run {[round(x, 2) for x in ts]}', flush=True)
        return
    (pn, dn), (pb, db) = new(), baseline()                    # every batch shape once on both sides (graph capture, weight packing)
    new(), baseline()
    times = {'new': [], 'baseline': []}
    for _ in range(a.reps):
        for name, f in (('new', new), ('baseline', baseline)):
            times[name].append(timed(f)[0])
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    shown = [x for i, x in enumerate(sys.argv[1:]) if x != '--out' and (i == 0 or sys.argv[i] != '--out')]
    res = {'command': ' '.join(['python tools/ppl_time.py'] + shown), 'size': 256, 'n_sample': a.n_sample, 'batch': a.batch,
           'batches': metrics.batch_sizes(a.n_sample, a.batch), 'config': {k: kw[k] for k in ('space', 'eval_plus', 'use_slerp', 'crop')},
           'ms_per_run_median': med, 'ms_per_sample_median': {k: v / a.n_sample for k, v in med.items()}, 'ms_per_run_all': times,
           'speedup': med['baseline'] / med['new'], 'ppl': {'new': pn, 'baseline': pb},
           'max_rel_difference_of_distances': float(abs(dn - db).max() / abs(db).max())}
    print(json.dumps({k: res[k] for k in ('ms_per_run_median', 'speedup', 'ppl', 'max_rel_difference_of_distances')}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

"""Attribute editing in the two mapped spaces (z+, p+): the reference's our_interfaceGAN/train_boundary.py, linear_interpolation.py and
the sampling and sweep loops of edit_all_noinversion_ffhq.py, from the attribute scores on.

    python -m transeditor_amd.edit --codes c.npy --scores s.npy --write_boundary b.npy [--ratio 0.02 --split_ratio 0.7 --seed 0]
    python -m transeditor_amd.edit --ckpt 790000.pt --size 256 --z_boundary zb.npy --p_boundary pb.npy --z_distance 30 --p_distance 30
                                   --steps 61 --n 8 --seed 0 --out sweep.npz

The reference copies every mapped code to the host and fits sklearn's SVC(kernel='linear') (libsvm's SMO on the CPU) to the extreme
samples.  Here the codes stay on the device: select_extremes sorts and splits there, and train_boundary runs the Gram matrix, the SMO
solve and the weight vector on the gfx950 kernels of csrc/svm.hip (te_gram_f32, te_svm_smo_f64, te_svm_coef_f32).  edit_sweep builds
all count x steps edited codes on the device and pushes them through a GeneratorSampler in batches instead of one image per call.

Differences from the reference, all deliberate:
  - no shrinking in the SMO solve (libsvm's heuristic that drops bounded variables from the working set; it changes the path, not the
    optimum), and ties in the working-set selection go to the lowest index, so a solve is bit-reproducible;
  - the train / validation split is drawn from a seeded torch generator (`seed`), not from np.random's global state;
  - `score_fn` is any callable images [B,3,S,S] -> [B], and it is handed the generator's image as it is.  The DEX age / gender
    classifier is transeditor_amd.dex.DEXScorer, whose stem does the reference's conversion to BGR in [0, 255] and the centre crop
    itself; fit_boundaries (also transeditor_amd.dex.fit_boundaries) goes from a generator and a scorer to the z+ and p+ boundaries;
  - at most 8192 training rows (the one-workgroup solver's limit; the reference's default run needs 4200);
  - make_image does not clamp its argument in place.
With invalid_value=None nothing synchronises with the host before the report and the boundary are read; filtering invalid scores
needs the number of valid ones, which is one more read.
"""
import argparse
import json
import sys
import types
import warnings

import numpy as np
import torch

_NO_GPU = 'transeditor_amd.edit.train_boundary needs a GPU (the SVM kernels are gfx950 only; there is no CPU path)'
MAX_TRAIN_ROWS = 8192


# ---------------------------------------------------------------------------------------------------------------- the training set
def _as_tensor(a, device=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t if device is None else t.to(device)


def select_extremes(codes, scores, chosen_num_or_ratio=0.02, split_ratio=0.7, invalid_value=None, seed=None):
    """train_boundary.py:33-88 on index tensors: the samples with the highest scores are the positive set, those with the lowest the
    negative set, each `chosen_num` long (a ratio in (0, 1] of the valid samples, else a count; capped at half of them) and split
    into int(chosen_num * split_ratio) training and the remaining validation samples by a permutation drawn from `seed` (None: torch's
    global generator).  codes [N,D] and scores [N,1]: torch tensors (any device) or numpy arrays; the codes are only looked at for
    their shape.  -> dict(train_pos, train_neg, val_pos, val_neg: int64 index tensors into `codes` on the scores' device; chosen_num)"""
    if not (isinstance(codes, np.ndarray) or torch.is_tensor(codes)) or codes.ndim != 2:
        raise ValueError('Input `codes` should be a numpy array or a torch tensor of shape [num_samples, latent_space_dim]!')
    if (not (isinstance(scores, np.ndarray) or torch.is_tensor(scores)) or scores.ndim != 2 or scores.shape[0] != codes.shape[0]
            or scores.shape[1] != 1):
        raise ValueError('Input `scores` should be a numpy array or a torch tensor of shape [num_samples, 1], where `num_samples` '
                         'should be exactly same as that of input `codes`!')
    if chosen_num_or_ratio <= 0:
        raise ValueError(f'Input `chosen_num_or_ratio` should be positive, but {chosen_num_or_ratio} received!')
    s = _as_tensor(scores)[:, 0]
    valid = None
    if invalid_value is not None:                                                      # :50-52
        valid = torch.nonzero(s != invalid_value)[:, 0]
        s = s[valid]
    order = torch.argsort(s, stable=True).flip(0)                                      # :55: ascending, reversed
    if valid is not None:
        order = valid[order]
    n = order.shape[0]
    chosen = int(n * chosen_num_or_ratio) if 0 < chosen_num_or_ratio <= 1 else int(chosen_num_or_ratio)      # :59-63
    chosen = min(chosen, n // 2)
    train_num = int(chosen * split_ratio)                                              # :67
    g = None if seed is None else torch.Generator().manual_seed(seed)
    pos = torch.randperm(chosen, generator=g).to(order.device)                         # :70-71
    neg = torch.randperm(chosen, generator=g).to(order.device)                         # :75-76
    top, bottom = order[:chosen], order[n - chosen:]
    return dict(train_pos=top[pos[:train_num]], train_neg=bottom[neg[:train_num]], val_pos=top[pos[train_num:]],
                val_neg=bottom[neg[train_num:]], chosen_num=chosen)


# ---------------------------------------------------------------------------------------------------------------- the boundary
@torch.no_grad()
def train_boundary(codes, scores, chosen_num_or_ratio=0.02, split_ratio=0.7, invalid_value=None, seed=None, C=1.0, tol=1e-3,
                   max_iter=1_000_000):
    """train_boundary.py on the device: select_extremes, then the linear C-SVC of the training rows (positive: the highest scores) by
    te_gram_f32, te_svm_smo_f64 and te_svm_coef_f32, then the division by the norm.  codes [N,D] float32 and scores [N,1]: tensors on
    the GPU, or numpy arrays, which are uploaded.
    -> (boundary [1,D] float32 numpy, unit norm, pointing toward high scores;
        report dict: train_accuracy, val_accuracy (None without validation samples) of sign(x . w - rho), iterations, converged,
        n_support, n_train, n_val, chosen_num, rho and norm = |w| of the un-normalised solution, so x . boundary - rho / norm has the
        same sign)."""
    sel = select_extremes(codes, scores, chosen_num_or_ratio, split_ratio, invalid_value, seed)
    if isinstance(codes, np.ndarray) and codes.dtype != np.float32 or torch.is_tensor(codes) and codes.dtype != torch.float32:
        raise ValueError(f'train_boundary: codes must be float32, got {codes.dtype}')
    train_num, val_num = sel['train_pos'].shape[0], sel['val_pos'].shape[0]
    if not 1 <= train_num <= MAX_TRAIN_ROWS // 2:
        raise ValueError(f'train_boundary: the training set has {train_num} positive and {train_num} negative rows; the solver takes '
                         f'1..{MAX_TRAIN_ROWS // 2} of each (lower chosen_num_or_ratio or split_ratio)')
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    from . import _lib
    x_all = _as_tensor(codes, 'cuda') if isinstance(codes, np.ndarray) else codes
    if not x_all.is_cuda:
        raise ValueError('train_boundary: a codes tensor must be on the GPU (pass numpy float32 to have it uploaded)')
    dev = x_all.device
    with torch.cuda.device(dev):
        x = x_all[torch.cat([sel['train_pos'], sel['train_neg']]).to(dev)].contiguous()
        y = np.concatenate([np.ones(train_num, np.int8), -np.ones(train_num, np.int8)])          # known from the shapes: no read-back
        K = _lib.gram(x)
        alpha, rho, info = _lib.svm_smo(K, y, C, tol, max_iter)
        w = _lib.svm_coef(x, alpha, y)
        w64 = w.double()
        norm = w64.norm()
        boundary = (w64 / norm).float().view(1, -1)

        def correct(rows, n_each):
            f = rows.double() @ w64 - rho
            return ((f[:n_each] > 0).sum() + (f[n_each:] <= 0).sum()).double()
        numbers = [correct(x, train_num)]
        if val_num:
            numbers.append(correct(x_all[torch.cat([sel['val_pos'], sel['val_neg']]).to(dev)], val_num))
        numbers += [(alpha > 0).sum().double(), info.double()[0], info.double()[1], rho[0], norm]
        numbers = torch.stack(numbers).tolist()                                                  # the one read of the report
        boundary = boundary.cpu().numpy()
    val_correct = numbers.pop(1) if val_num else None
    train_correct, n_support, iterations, converged, rho_, norm_ = numbers
    report = dict(train_accuracy=train_correct / (2 * train_num), val_accuracy=None if val_correct is None else val_correct / (2 * val_num),
                  iterations=int(iterations), converged=bool(converged), n_support=int(n_support), n_train=2 * train_num,
                  n_val=2 * val_num, chosen_num=sel['chosen_num'], rho=rho_, norm=norm_)
    if not report['converged']:
        warnings.warn(f'train_boundary: the SMO solve stopped at max_iter = {max_iter} before Gmax - Gmin < {tol}; the boundary is the '
                      f'feasible iterate it reached', RuntimeWarning, stacklevel=2)
    return boundary, report


def reference_train_boundary(latent_codes, scores, chosen_num_or_ratio=0.02, split_ratio=0.7, invalid_value=None):
    """train_boundary with the reference's call surface (train_boundary.py:5-9): numpy in, the [1,D] boundary out"""
    return train_boundary(latent_codes, scores, chosen_num_or_ratio, split_ratio, invalid_value)[0]


# ---------------------------------------------------------------------------------------------------------------- moving a code
def linear_interpolate(code, boundary, start_distance=-100, end_distance=100, steps=10):
    """linear_interpolation.py:33-48: `steps` codes from `start_distance` to `end_distance` along the unit `boundary`.
    code [1,D] with boundary [1,D]: the distances are signed distances TO the boundary (the code's own projection is subtracted);
    code [1,L,D] (W+) with boundary [1,D]: every one of the L rows moves by the plain distance.  float32 torch tensors on one device
    -> a tensor there; numpy arrays -> a numpy array.  The distances are formed in float64 and rounded once, as in the reference."""
    as_numpy = isinstance(code, np.ndarray)
    c, b = _as_tensor(code), _as_tensor(boundary)
    if not (c.shape[0] == 1 and b.shape[0] == 1 and b.ndim == 2 and b.shape[1] == c.shape[-1]):
        raise AssertionError(f'linear_interpolate: needs a code [1,D] or [1,L,D] and a boundary [1,D], got {tuple(c.shape)} and '
                             f'{tuple(b.shape)}')
    b = b.to(c.device)
    lin = torch.linspace(start_distance, end_distance, steps, dtype=torch.float64, device=c.device)
    if c.ndim == 2:
        lin = lin - (c @ b.T).double().view(())
        out = c + lin.view(-1, 1).to(c.dtype) * b
    elif c.ndim == 3:
        out = c + lin.view(-1, 1, 1).to(c.dtype) * b.view(1, 1, -1)
    else:
        raise ValueError(f'Input `code` should be with shape [1, latent_space_dim] or [1, N, latent_space_dim] for W+ space!\n'
                         f'But {tuple(c.shape)} is received.')
    return out.numpy() if as_numpy else out


def make_image(tensor):
    """utils/editing_utils.py:8-19: images [B,3,H,W] in [-1, 1] -> uint8 numpy [B,H,W,3] (truncating, as the reference does)"""
    return tensor.detach().clamp(min=-1, max=1).add(1).div_(2).mul_(255).type(torch.uint8).permute(0, 2, 3, 1).to('cpu').numpy()


def flatten_codes(mapped):
    """mapped codes [B,latent,tokens] as the generator returns them -> [B, tokens * latent], the layout the boundaries live in
    (edit_all_noinversion_ffhq.py:110 and :146)"""
    return mapped.transpose(1, 2).reshape(mapped.shape[0], -1)


def unflatten_codes(flat, latent):
    """[M, tokens * latent] -> [M,latent,tokens] (:236-239)"""
    return flat.reshape(flat.shape[0], -1, latent).transpose(1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- generator loops
@torch.no_grad()
def sample_codes(generator, score_fn, *, n_sample, batch, truncation=0.7, seed=None, latent=512, para_num=16):
    """edit_all_noinversion_ffhq.py:103-148: n_sample codes drawn as the reference draws them (both multiplied by `truncation`), mapped
    into z+ and p+, rendered from the mapped codes and scored by score_fn(images [B,3,S,S]) -> [B].
    -> (z_codes [N, tokens * latent], p_codes [N, tokens * latent], scores [N,1]) float32 on the generator's device."""
    from .metrics import _as_sampler, batch_sizes
    from .utils.sample import prepare_noise_new, prepare_param
    sizes = batch_sizes(n_sample, batch)
    if not sizes:
        raise ValueError('sample_codes: n_sample must be positive')
    g = _as_sampler(generator)
    device = next(g.g.parameters()).device
    args = types.SimpleNamespace(latent=latent, para_num=para_num)
    zs, ps, scores = [], [], []
    with torch.random.fork_rng(devices=[device] if device.type == 'cuda' else [], enabled=seed is not None):
        if seed is not None:
            torch.manual_seed(seed)
        for b in sizes:
            noise = prepare_noise_new(b, args, device, 'query', truncation=truncation)
            para = prepare_param(b, args, device, method='spatial', truncation=truncation)
            z_plus, p_plus = g(noise, para, return_mapped_codes=True)                            # :107-108 in one call
            image, _, _ = g(z_plus, p_plus, use_spatial_mapping=False, use_style_mapping=False)
            s = score_fn(image)
            if s.numel() != b:
                raise ValueError(f'sample_codes: score_fn must return one score per image, got {tuple(s.shape)} for a batch of {b}')
            zs.append(flatten_codes(z_plus))
            ps.append(flatten_codes(p_plus))
            scores.append(s.reshape(b, 1).float())
    return torch.cat(zs).contiguous(), torch.cat(ps).contiguous(), torch.cat(scores).contiguous()


def fit_boundaries(generator, scorer, *, n_sample, batch, ratio=0.02, split_ratio=0.7, truncation=0.7, seed=None, latent=512,
                   para_num=16, invalid_value=None):
    """edit_all_noinversion_ffhq.py:103-166: sample n_sample codes, score their images with `scorer` and fit one boundary in z+ and one
    in p+ to the extreme scores (sample_codes, then train_boundary twice; `seed` seeds the sampling and both splits).
    -> dict(z_boundary, p_boundary: [1, tokens * latent] float32 numpy, unit norm; z_report, p_report: train_boundary's reports;
            scores: [n_sample, 1] on the device)"""
    z_codes, p_codes, scores = sample_codes(generator, scorer, n_sample=n_sample, batch=batch, truncation=truncation, seed=seed,
                                            latent=latent, para_num=para_num)
    z_boundary, z_report = train_boundary(z_codes, scores, ratio, split_ratio, invalid_value, seed)
    p_boundary, p_report = train_boundary(p_codes, scores, ratio, split_ratio, invalid_value, seed)
    return dict(z_boundary=z_boundary, p_boundary=p_boundary, z_report=z_report, p_report=p_report, scores=scores)


def _ends(distance):
    return (-distance, distance) if isinstance(distance, (int, float)) else tuple(distance)


def sweep_codes(z_plus, p_plus, z_boundary, p_boundary, *, z_distance, p_distance, steps):
    """the edited codes of edit_all_noinversion_ffhq.py:222-280, on the codes' device: dict 'p' / 'z' / 'pz' -> (z, p), each
    [count * steps, latent, tokens] with the steps of one input adjacent.  A boundary [1, tokens * latent] moves the flattened code
    (linear_interpolate's 2-D form, what the reference does); a boundary [1, latent] moves every token alike (its W+ form).  A
    distance d sweeps -d .. d (:225-226); a pair is (start, end)."""
    count, latent = z_plus.shape[0], z_plus.shape[1]

    def moved(mapped, boundary, distance):
        b = _as_tensor(boundary).to(mapped.device)
        flat = flatten_codes(mapped)
        start, end = _ends(distance)
        if b.shape[-1] == latent and flat.shape[1] != latent:
            rows = [linear_interpolate(flat[i:i + 1].reshape(1, -1, latent), b, start, end, steps).reshape(steps, -1) for i in range(count)]
        else:
            rows = [linear_interpolate(flat[i:i + 1], b, start, end, steps) for i in range(count)]
        return unflatten_codes(torch.cat(rows), latent)
    z_moved, p_moved = moved(z_plus, z_boundary, z_distance), moved(p_plus, p_boundary, p_distance)
    z_same, p_same = z_plus.repeat_interleave(steps, 0).contiguous(), p_plus.repeat_interleave(steps, 0).contiguous()
    return {'p': (z_same, p_moved), 'z': (z_moved, p_same), 'pz': (z_moved, p_moved)}


@torch.no_grad()
def edit_sweep(generator, z_plus, p_plus, z_boundary, p_boundary, *, z_distance, p_distance, steps, batch):
    """edit_all_noinversion_ffhq.py:222-280: for every mapped input (z_plus, p_plus [count,latent,tokens]) the three sweeps along the
    boundaries: p only, z only, both.  The codes of sweep_codes go through the sampler sweep by sweep, in batches of `batch` (the last
    one of a sweep shorter), with use_style_mapping=False, use_spatial_mapping=False.
    -> {'p', 'z', 'pz'}: images [count, steps, 3, S, S] on the device"""
    from .metrics import _as_sampler, batch_sizes
    if z_plus.ndim != 3 or z_plus.shape != p_plus.shape:
        raise ValueError(f'edit_sweep: z_plus and p_plus must both be [count,latent,tokens], got {tuple(z_plus.shape)}, {tuple(p_plus.shape)}')
    g = _as_sampler(generator)
    count = z_plus.shape[0]
    out = {}
    for name, (z, p) in sweep_codes(z_plus, p_plus, z_boundary, p_boundary, z_distance=z_distance, p_distance=p_distance,
                                    steps=steps).items():
        images, at = [], 0
        for b in batch_sizes(count * steps, batch):
            images.append(g(z[at:at + b], p[at:at + b], use_style_mapping=False, use_spatial_mapping=False)[0])
            at += b
        images = torch.cat(images)
        out[name] = images.view(count, steps, *images.shape[1:])
    return out


# ------------------------------------------------------------------------------------------------------------------------ CLI
class _Parser(argparse.ArgumentParser):
    """two modes that exclude each other; parse_args sets args.mode = 'boundary' | 'sweep'"""

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        boundary, sweep = (a.codes, a.scores, a.write_boundary), (a.ckpt, a.z_boundary, a.p_boundary, a.out)
        if any(v is not None for v in boundary) and any(v is not None for v in sweep):
            self.error('--codes / --scores / --write_boundary (train a boundary) and --ckpt / --z_boundary / --p_boundary / --out '
                       '(an edit sweep) exclude each other')
        if any(v is not None for v in boundary):
            if None in boundary:
                self.error('training a boundary needs --codes, --scores and --write_boundary')
            a.mode = 'boundary'
            return a
        if None in sweep:
            self.error('give --codes, --scores and --write_boundary, or --ckpt, --z_boundary, --p_boundary and --out')
        if a.size < 8 or a.size & (a.size - 1):
            self.error(f'--size must be a power of two >= 8, got {a.size}')
        if a.steps < 1 or a.n < 1:
            self.error('--steps and --n must be positive')
        a.mode = 'sweep'
        return a


def build_parser():
    parser = _Parser(description='train an editing boundary from codes and attribute scores (our_interfaceGAN/train_boundary.py), or '
                                 'sweep sampled codes along a z+ and a p+ boundary (edit_all_noinversion_ffhq.py:184-280)')
    parser.add_argument('--codes', help='.npy file of the flattened mapped codes [N,D], float32')
    parser.add_argument('--scores', help='.npy file of the attribute scores [N] or [N,1]')
    parser.add_argument('--write_boundary', help='output .npy file of the boundary [1,D]')
    parser.add_argument('--ratio', type=float, default=0.02, help='chosen_num_or_ratio')
    parser.add_argument('--split_ratio', type=float, default=0.7)
    parser.add_argument('--seed', type=int, default=None, help='seed of the train / validation split, or of the sampled codes')
    parser.add_argument('--ckpt', help='a checkpoint file')
    parser.add_argument('--z_boundary', help='.npy file of the z+ boundary')
    parser.add_argument('--p_boundary', help='.npy file of the p+ boundary')
    parser.add_argument('--z_distance', type=float, default=30.0, help='the z+ sweep runs from -z_distance to z_distance')
    parser.add_argument('--p_distance', type=float, default=30.0)
    parser.add_argument('--steps', type=int, default=61)
    parser.add_argument('--n', type=int, default=8, help='the number of sampled inputs')
    parser.add_argument('--out', help='output .npz file: p, z, pz uint8 [n,steps,S,S,3] and origin [n,S,S,3]')
    parser.add_argument('--size', type=int, default=256)
    parser.add_argument('--batch', type=int, default=16)
    parser.add_argument('--truncation', type=float, default=0.7)
    parser.add_argument('--para_num', type=int, default=16)
    parser.add_argument('--channel_multiplier', type=int, default=2)
    parser.add_argument('--num_trans', type=int, default=8)
    return parser


def _generator(args):
    """the sampler of the checkpoint args.ckpt"""
    import math
    from .inference import GeneratorSampler
    from .model_spatial_query import Generator
    from .train_step import load_checkpoint_into
    g = Generator(args.size, 512, 512, 2 * (int(math.log(args.size, 2)) - 1), channel_multiplier=args.channel_multiplier,
                  n_trans=args.num_trans, pixel_norm_op_dim=1).to('cuda')
    load_checkpoint_into(args.ckpt, g, device='cuda', g_ema_only_ok=True)
    return GeneratorSampler(g)


def scorer_parser(description, weights_help):
    """the command line of `python -m transeditor_amd.dex` / `.celeba_attr` (generator + scorer -> z+ and p+ boundaries) without the
    scorer's own options"""
    parser = argparse.ArgumentParser(description=description)
    parser.add_argument('--ckpt', required=True, help='a generator checkpoint file')
    parser.add_argument('--weights', required=True, help=weights_help)
    parser.add_argument('--num_sample', type=int, default=10000)
    parser.add_argument('--write_z_boundary', required=True, help='output .npy file of the z+ boundary [1,D]')
    parser.add_argument('--write_p_boundary', required=True, help='output .npy file of the p+ boundary [1,D]')
    parser.add_argument('--write_scores', help='output .npy file of the scores [N,1]')
    parser.add_argument('--ratio', type=float, default=0.02, help='chosen_num_or_ratio')
    parser.add_argument('--split_ratio', type=float, default=0.7)
    parser.add_argument('--seed', type=int, default=None, help='seed of the sampled codes and of the train / validation splits')
    parser.add_argument('--size', type=int, default=256)
    parser.add_argument('--batch', type=int, default=16)
    parser.add_argument('--truncation', type=float, default=0.7)
    parser.add_argument('--para_num', type=int, default=16)
    parser.add_argument('--channel_multiplier', type=int, default=2)
    parser.add_argument('--num_trans', type=int, default=8)
    return parser


def scorer_main(parser, argv, no_gpu, make_scorer):
    """parse, build the scorer and the generator, fit, save the arrays, print the JSON line.  make_scorer(args) -> (score_fn, the
    report's leading fields, its fields about the scorer); `no_gpu` is the scorer's message without a GPU."""
    args = parser.parse_args(argv)
    if args.size < 8 or args.size & (args.size - 1):
        parser.error(f'--size must be a power of two >= 8, got {args.size}')
    if args.num_sample < 1 or args.batch < 1:
        parser.error('--num_sample and --batch must be positive')
    if not torch.cuda.is_available():
        raise RuntimeError(no_gpu)
    score_fn, lead, own = make_scorer(args)
    out = fit_boundaries(_generator(args), score_fn, n_sample=args.num_sample, batch=args.batch, ratio=args.ratio,
                         split_ratio=args.split_ratio, truncation=args.truncation, seed=args.seed, para_num=args.para_num)
    np.save(args.write_z_boundary, out['z_boundary'])
    np.save(args.write_p_boundary, out['p_boundary'])
    scores = out['scores'].cpu().numpy()
    if args.write_scores:
        np.save(args.write_scores, scores)
    res = {**lead, 'ckpt': args.ckpt, 'weights': args.weights, 'n': args.num_sample, **own, 'score_mean': float(scores.mean()),
           'score_min': float(scores.min()), 'score_max': float(scores.max()), 'z': out['z_report'], 'p': out['p_report'],
           'wrote': [args.write_z_boundary, args.write_p_boundary] + ([args.write_scores] if args.write_scores else [])}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    if args.mode == 'boundary':
        codes = np.load(args.codes, allow_pickle=False)
        scores = np.load(args.scores, allow_pickle=False).astype(np.float32).reshape(-1, 1)
        boundary, report = train_boundary(codes, scores, args.ratio, args.split_ratio, seed=args.seed)
        np.save(args.write_boundary, boundary)
        res = {'mode': 'boundary', 'codes': args.codes, 'n': int(codes.shape[0]), 'dim': int(codes.shape[1]), 'wrote': args.write_boundary}
        res.update(report)
    else:
        from .utils.sample import prepare_noise_new, prepare_param
        sampler = _generator(args)
        ns = types.SimpleNamespace(latent=512, para_num=args.para_num)
        with torch.random.fork_rng(devices=['cuda'], enabled=args.seed is not None):
            if args.seed is not None:
                torch.manual_seed(args.seed)
            noise = prepare_noise_new(args.n, ns, 'cuda', 'query', truncation=args.truncation)           # :184-185
            para = prepare_param(args.n, ns, 'cuda', method='spatial', truncation=args.truncation)
        with torch.no_grad():
            z_plus, p_plus = sampler(noise, para, return_mapped_codes=True)                              # :203-204
            origin = sampler(z_plus, p_plus, use_style_mapping=False, use_spatial_mapping=False)[0]
        sweeps = edit_sweep(sampler, z_plus, p_plus, np.load(args.z_boundary, allow_pickle=False),
                            np.load(args.p_boundary, allow_pickle=False), z_distance=args.z_distance, p_distance=args.p_distance,
                            steps=args.steps, batch=args.batch)
        arrays = {k: make_image(v.flatten(0, 1)).reshape(args.n, args.steps, args.size, args.size, 3) for k, v in sweeps.items()}
        np.savez(args.out, origin=make_image(origin), **arrays)
        res = {'mode': 'sweep', 'ckpt': args.ckpt, 'n': args.n, 'steps': args.steps, 'size': args.size, 'z_distance': args.z_distance,
               'p_distance': args.p_distance, 'wrote': args.out}
    print(json.dumps(res), flush=True)
    return res


if __name__ == '__main__':
    main(sys.argv[1:])

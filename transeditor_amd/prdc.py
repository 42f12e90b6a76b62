"""Precision, recall, density and coverage (PRDC) of two feature sets: the reference's metrics/prdc.py (behind metrics/calc_prdc.py) on
the gfx950 kernels of csrc/prdc.hip.

    python -m transeditor_amd.prdc --real real.npy --fake fake.npy [--nearest_k 3]

The reference builds three dense distance matrices on the CPU (sklearn pairwise_distances) and thresholds them.  Here each of the three
is one pass of a fused fp32-MFMA distance GEMM whose epilogue does the reduction, so no N x M matrix exists anywhere:
  te_prdc_knn_f32 on the real set and on the fake set (the squared radius of every sample: prdc.py:41-51), then te_prdc_counts_f32 on
  real x fake (the three thresholded reductions of :75-93).  The four means are taken from the integer counts in float64.

Differences from the reference, all deliberate:
  - every comparison is made on SQUARED distances d2 = max(|x|^2 + |y|^2 - 2 x.y, 0) in fp32 (sklearn forms the same expression in
    fp32 blocks and takes the root); the root is monotone, so only pairs within rounding of their threshold can compare differently;
  - the features, the radii and the counts stay on the device; the host synchronises once, when the four numbers are read;
  - the feature extractor is NOT built: calc_prdc.py:101-104 uses torchvision's VGG16 up to fc7, whose classifier weights this library
    does not have, and the LPIPS stem here has the scaling layer fused in, so it is not that network's input path.  `feature_fn` of
    evaluate_prdc and the .npy files of the command line are the seam: any [B,D] fp32 features do;
  - nearest_k is limited to 1..15 (the kernel keeps the k+1 smallest in registers); the reference's default is 3 (calc_prdc.py).
"""
import argparse
import json
import sys
import types

import numpy as np
import torch

KEYS = ('precision', 'recall', 'density', 'coverage')
MAX_K = 15


def _check_shapes(real_shape, fake_shape, nearest_k):
    if len(real_shape) != 2 or len(fake_shape) != 2:
        raise ValueError(f'prdc: features must be [N,D] and [M,D], got {tuple(real_shape)} and {tuple(fake_shape)}')
    if real_shape[1] != fake_shape[1] or real_shape[1] < 1:
        raise ValueError(f'prdc: real and fake features must share one feature dimension, got {real_shape[1]} and {fake_shape[1]}')
    if not isinstance(nearest_k, (int, np.integer)) or isinstance(nearest_k, bool) or not 1 <= nearest_k <= MAX_K:
        raise ValueError(f'prdc: nearest_k must be an integer in 1..{MAX_K}, got {nearest_k!r}')
    if real_shape[0] < nearest_k + 1 or fake_shape[0] < nearest_k + 1:
        raise ValueError(f'prdc: each set needs at least nearest_k + 1 = {nearest_k + 1} samples, got {real_shape[0]} and '
                         f'{fake_shape[0]}')


def _check_kind(f, name):
    if isinstance(f, np.ndarray):
        if f.dtype != np.float32:
            raise ValueError(f'prdc: {name} features must be float32, got {f.dtype}')
    elif not torch.is_tensor(f):
        raise ValueError(f'prdc: {name} features must be a numpy array or a torch tensor, got {type(f).__name__}')


def _on_device(f, name):
    _check_kind(f, name)
    if isinstance(f, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError('transeditor_amd.prdc needs a GPU (the distance kernels are gfx950 only; there is no CPU path)')
        return torch.from_numpy(np.ascontiguousarray(f)).to('cuda')
    return f


@torch.no_grad()
def _device_details(real_features, fake_features, nearest_k):
    _check_kind(real_features, 'real')
    _check_kind(fake_features, 'fake')
    _check_shapes(real_features.shape, fake_features.shape, nearest_k)
    from . import _lib
    x, y = _on_device(real_features, 'real'), _on_device(fake_features, 'fake')
    nx, ny = _lib.row_sqnorm(x), _lib.row_sqnorm(y)
    rr2 = _lib.prdc_knn(x, nx, int(nearest_k))                                  # :68-69
    rf2 = _lib.prdc_knn(y, ny, int(nearest_k))                                  # :70-71
    col_count, row_any, row_min = _lib.prdc_counts(x, nx, rr2, y, ny, rf2)      # :72-93
    return dict(rr2=rr2, rf2=rf2, col_count=col_count, row_any=row_any, row_min=row_min)


def _numbers(d, nearest_k):
    """the four means of :75-93 as ratios of integer counts in float64; reading the counts is the one host synchronisation"""
    n, m = d['rr2'].shape[0], d['rf2'].shape[0]
    inside, recalled, total, covered = torch.stack([(d['col_count'] > 0).sum(), (d['row_any'] != 0).sum(),
                                                    d['col_count'].sum(dtype=torch.int64), (d['row_min'] < d['rr2']).sum()]).tolist()
    return dict(precision=inside / m, recall=recalled / n, density=total / (float(nearest_k) * m), coverage=covered / n)


def prdc_details(real_features, fake_features, nearest_k):
    """The per-sample arrays behind the four numbers, as numpy arrays:
        rr2 [N], rf2 [M]  squared distance of every real / fake sample to its nearest_k-th neighbour in its own set
        col_count [M]     how many real balls hold fake sample j (> 0: j counts for precision; the sum is density's)
        row_any [N]       real sample i lies inside some fake ball (recall)
        row_min [N]       squared distance of real sample i to its nearest fake sample (< rr2[i]: i is covered)
    so a caller can see WHICH samples fall off the other manifold."""
    d = _device_details(real_features, fake_features, nearest_k)
    return {k: v.cpu().numpy() for k, v in d.items()}


def compute_prdc(real_features, fake_features, nearest_k):
    """metrics/prdc.py:54-96 -> dict(precision, recall, density, coverage) of Python floats.  real_features [N,D] and fake_features
    [M,D]: fp32 tensors on the GPU (used in place) or float32 numpy arrays (uploaded)."""
    d = _device_details(real_features, fake_features, nearest_k)
    return _numbers(d, nearest_k)


@torch.no_grad()
def fake_features(generator, feature_fn, *, n_sample=50000, batch=64, seed=None, latent=512, para_num=16):
    """feature_fn(images [B,3,S,S]) -> [B,D] over n_sample generated images, drawn as transeditor_amd.metrics draws them
    (prepare_noise_new 'query', prepare_param 'spatial'); the features stay on the device -> [n_sample, D]"""
    from .metrics import _as_sampler, batch_sizes
    from .utils.sample import prepare_noise_new, prepare_param
    sizes = batch_sizes(n_sample, batch)
    if not sizes:
        raise ValueError('fake_features: n_sample must be positive')
    g = _as_sampler(generator)
    device = next(g.g.parameters()).device
    args = types.SimpleNamespace(latent=latent, para_num=para_num)
    feats = []
    with torch.random.fork_rng(devices=[device] if device.type == 'cuda' else [], enabled=seed is not None):
        if seed is not None:
            torch.manual_seed(seed)
        for b in sizes:
            z = prepare_noise_new(b, args, device, method='query')
            p = prepare_param(b, args, device, method='spatial')
            image, _, _ = g(z, p)
            f = feature_fn(image)
            if f.ndim != 2 or f.shape[0] != b:
                raise ValueError(f'fake_features: feature_fn must return [B,D] features, got {tuple(f.shape)} for a batch of {b}')
            feats.append(f.float())
    return torch.cat(feats).contiguous()


def evaluate_prdc(generator, feature_fn, real_features, *, n_sample=50000, batch=64, nearest_k=3, seed=None, latent=512, para_num=16):
    """calc_prdc.py's run for one generator: n_sample generated images -> feature_fn -> compute_prdc against real_features.
    `generator`: a Generator or a GeneratorSampler over it; `seed`: draw the codes from a generator state of their own."""
    fake = fake_features(generator, feature_fn, n_sample=n_sample, batch=batch, seed=seed, latent=latent, para_num=para_num)
    real = _on_device(real_features, 'real')
    if torch.is_tensor(real) and real.device != fake.device:
        real = real.to(fake.device)
    return compute_prdc(real, fake, nearest_k)


# ------------------------------------------------------------------------------------------------------------------------ CLI
def build_parser():
    parser = argparse.ArgumentParser(description='precision / recall / density / coverage of two feature files (metrics/prdc.py)')
    parser.add_argument('--real', required=True, help='.npy file of the real features [N,D], float32')
    parser.add_argument('--fake', required=True, help='.npy file of the generated features [M,D], float32')
    parser.add_argument('--nearest_k', type=int, default=3)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('transeditor_amd.prdc needs a GPU (the distance kernels are gfx950 only; there is no CPU path)')
    real = np.load(args.real, allow_pickle=False)
    fake = np.load(args.fake, allow_pickle=False)
    res = {'metric': 'prdc', 'real': args.real, 'fake': args.fake, 'n_real': int(real.shape[0]), 'n_fake': int(fake.shape[0]),
           'nearest_k': args.nearest_k}
    res.update(compute_prdc(real, fake, args.nearest_k))
    print(json.dumps(res), flush=True)
    return res


if __name__ == '__main__':
    main(sys.argv[1:])

"""Precision, recall, density and coverage (PRDC) of two feature sets: the reference's metrics/prdc.py (behind metrics/calc_prdc.py) on
the gfx950 kernels of csrc/prdc.hip.

    python -m transeditor_amd.prdc --real real.npy --fake fake.npy [--nearest_k 3]
    python -m transeditor_amd.prdc --ckpt 790000.pt --dataset ffhq_lmdb --size 256 --vgg16 vgg16-397923af.pth
                                   [--n_sample 50000 --batch 64 --nearest_k 3 --seed 0]        (calc_prdc.py's own run)

The reference builds three dense distance matrices on the CPU (sklearn pairwise_distances) and thresholds them.  Here each of the three
is one pass of a fused fp32-MFMA distance GEMM whose epilogue does the reduction, so no N x M matrix exists anywhere:
  te_prdc_knn_f32 on the real set and on the fake set (the squared radius of every sample: prdc.py:41-51), then te_prdc_counts_f32 on
  real x fake (the three thresholded reductions of :75-93).  The four means are taken from the integer counts in float64.

Differences from the reference, all deliberate:
  - every comparison is made on SQUARED distances d2 = max(|x|^2 + |y|^2 - 2 x.y, 0) in fp32 (sklearn forms the same expression in
    fp32 blocks and takes the root); the root is monotone, so only pairs within rounding of their threshold can compare differently;
  - the features, the radii and the counts stay on the device; the host synchronises once, when the four numbers are read;
  - the feature extractor of calc_prdc.py:101-104 (torchvision's VGG16 up to fc7) is transeditor_amd.vgg_features.VGG16Features, built
    from the vgg16 state dict file a user already has for LPIPS; torchvision is not used.  It is one choice of `feature_fn`: any
    callable images [B,3,S,S] -> [B,D] fp32 features serves evaluate_prdc / fake_features / dataset_features, and the two-file mode of
    the command line takes features made anywhere.  Nearly all of the extractor's time is the convolution trunk (profiles/README.md);
  - dataset_features draws its n_sample real images WITHOUT replacement (the head of one seeded permutation).  The reference builds a
    new shuffled loader for every batch and takes its first batch (calc_prdc.py:47-55), so it samples with replacement across batches
    and can count an image twice;
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


@torch.no_grad()
def dataset_features(dataset, feature_fn, *, n_sample, batch, seed=None, device=None):
    """feature_fn over n_sample images of `dataset` (any object with __len__ and __getitem__ -> [3,S,S] tensors in [-1, 1]): the first
    n_sample items of a permutation of the dataset (seeded by `seed`; the global generator otherwise), in batches of `batch`, the
    last one shorter -> [n_sample, D] on `device` (default: the GPU if there is one).  calc_prdc.py:37-61, but without replacement."""
    from .metrics import batch_sizes
    n = len(dataset)
    if not isinstance(n_sample, int) or n_sample < 1 or n_sample > n:
        raise ValueError(f'dataset_features: n_sample must be in 1..len(dataset) = {n} (sampling is without replacement), got {n_sample}')
    if device is None:
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
    order = torch.randperm(n) if seed is None else torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    order = order[:n_sample].tolist()
    feats, at = [], 0
    for b in batch_sizes(n_sample, batch):
        images = torch.stack([torch.as_tensor(dataset[i]) for i in order[at:at + b]]).to(device)
        at += b
        f = feature_fn(images)
        if f.ndim != 2 or f.shape[0] != b:
            raise ValueError(f'dataset_features: feature_fn must return [B,D] features, got {tuple(f.shape)} for a batch of {b}')
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
class _Parser(argparse.ArgumentParser):
    """the two modes exclude each other and each needs both of its inputs; parse_args sets args.mode = 'files' | 'model'"""

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        files, model = (a.real, a.fake), (a.ckpt, a.dataset)
        if any(v is not None for v in files) and any(v is not None for v in model):
            self.error('--real / --fake (two feature files) and --ckpt / --dataset (a checkpoint against a dataset) exclude each other')
        if any(v is not None for v in files):
            if None in files:
                self.error('the two-file mode needs both --real and --fake')
            a.mode = 'files'
            return a
        if None in model:
            self.error('give --real and --fake, or --ckpt and --dataset')
        if a.size < 32 or a.size & (a.size - 1):
            self.error(f'--size must be a power of two >= 32, got {a.size}')
        a.mode = 'model'
        return a


def build_parser():
    parser = _Parser(description='precision / recall / density / coverage (metrics/prdc.py): of two feature files (--real, --fake), or '
                                 'of a checkpoint against a dataset through VGG16 fc7 features (--ckpt, --dataset: metrics/calc_prdc.py)')
    parser.add_argument('--real', help='.npy file of the real features [N,D], float32')
    parser.add_argument('--fake', help='.npy file of the generated features [M,D], float32')
    parser.add_argument('--ckpt', help='a checkpoint file, or a directory of <iteration>.pt files')
    parser.add_argument('--dataset', help='LMDB directory of the real images (utils/dataset.py MultiResolutionDataset)')
    parser.add_argument('--size', type=int, default=256)
    parser.add_argument('--vgg16', default=None, help='torchvision vgg16 state dict (default: the torch hub cache path)')
    parser.add_argument('--n_sample', type=int, default=50000)
    parser.add_argument('--batch', type=int, default=64)
    parser.add_argument('--start_num', type=int, default=0)
    parser.add_argument('--nearest_k', type=int, default=3)
    parser.add_argument('--seed', type=int, default=None, help='seed of the generated codes and of the choice of real images')
    parser.add_argument('--para_num', type=int, default=16)
    parser.add_argument('--channel_multiplier', type=int, default=2)
    parser.add_argument('--num_trans', type=int, default=8)
    return parser


def real_image_transform(resize):
    """calc_prdc.py:91-98 without torchvision: Resize(resize) (bilinear, short side) -> CenterCrop(resize) -> ToTensor ->
    Normalize(0.5, 0.5) -> fp32 [3,resize,resize] in [-1, 1]"""
    from .utils.dataset import image_transform
    to_tensor = image_transform(flip_probability=0)

    def run(img):
        from PIL import Image
        w, h = img.size
        if min(w, h) != resize:
            nw, nh = (resize, int(resize * h / w)) if w <= h else (int(resize * w / h), resize)
            img = img.resize((nw, nh), Image.BILINEAR)
            w, h = nw, nh
        left, top = int(round((w - resize) / 2.0)), int(round((h - resize) / 2.0))
        return to_tensor(img.crop((left, top, left + resize, top + resize)))
    return run


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('transeditor_amd.prdc needs a GPU (the distance kernels are gfx950 only; there is no CPU path)')
    if args.mode == 'files':
        real = np.load(args.real, allow_pickle=False)
        fake = np.load(args.fake, allow_pickle=False)
        res = {'metric': 'prdc', 'real': args.real, 'fake': args.fake, 'n_real': int(real.shape[0]), 'n_fake': int(fake.shape[0]),
               'nearest_k': args.nearest_k}
        res.update(compute_prdc(real, fake, args.nearest_k))
        print(json.dumps(res), flush=True)
        return res
    import math
    from .inference import GeneratorSampler
    from .metrics import checkpoints
    from .model_spatial_query import Generator
    from .train_step import load_checkpoint_into
    from .utils.dataset import MultiResolutionDataset
    from .vgg_features import VGG16Features
    vgg = VGG16Features(args.vgg16)
    dataset = MultiResolutionDataset(args.dataset, real_image_transform(min(args.size, 256)), args.size)      # calc_prdc.py:79, :99
    real = dataset_features(dataset, vgg, n_sample=args.n_sample, batch=args.batch, seed=args.seed)
    results = []
    for model_path in checkpoints(args.ckpt, args.start_num):
        g = Generator(args.size, 512, 512, 2 * (int(math.log(args.size, 2)) - 1), channel_multiplier=args.channel_multiplier,
                      n_trans=args.num_trans, pixel_norm_op_dim=1).to('cuda')
        load_checkpoint_into(model_path, g, device='cuda', g_ema_only_ok=True)
        res = {'metric': 'prdc', 'ckpt': model_path, 'dataset': args.dataset, 'n_real': int(real.shape[0]), 'n_fake': args.n_sample,
               'nearest_k': args.nearest_k}
        res.update(evaluate_prdc(GeneratorSampler(g), vgg, real, n_sample=args.n_sample, batch=args.batch, nearest_k=args.nearest_k,
                                 seed=args.seed, para_num=args.para_num))
        print(json.dumps(res), flush=True)
        results.append(res)
    return results


if __name__ == '__main__':
    main(sys.argv[1:])

"""The Frechet inception distance (FID): the reference's metrics/fid_query.py and metrics/calc_inception.py, with the feature moments on
the gfx950 kernels of csrc/fid.hip and the Inception-v3 pool3 features of transeditor_amd.inception_features.

    python -m transeditor_amd.fid --real real.npy --fake fake.npy                    (two feature files, float32 [N,D])
    python -m transeditor_amd.fid --stats inception_ffhq.pkl --fake fake.npy         (the reference's statistics file against features)
    python -m transeditor_amd.fid --features real.npy --write_stats inception_x.pkl  (statistics of a feature file; .pkl or .npz)
    python -m transeditor_amd.fid --dataset lmdb --inception W.pth --write_stats inception_x.pkl     (calc_inception.py end to end)
    python -m transeditor_amd.fid --ckpt C --stats inception_x.pkl --inception W.pth                 (fid_query.py end to end;
                                                                  --dataset lmdb in place of --stats: real statistics on the fly)

The FID needs no features, only n, s = sum x and S = sum x x^T, and these add across batches, calls and ranks.  FeatureStats holds them
on the device in fp64 and folds every full staging buffer in with one te_fid_moments_f64 call (a symmetric rank-N update on the fp64
MFMA); frechet_distance turns two (mean, cov) pairs into the number on the host.

Differences from the reference, all deliberate:
  - the moments are accumulated in ONE pass, uncentred, in fp64 on the device (every fp32 x fp32 product is exact in fp64, only the
    sums round); the reference keeps all n_sample x D features on the host and calls np.cov (two-pass, fp64) at the end;
  - the mean is fp64; the reference's np.mean of float32 features is an fp32 mean (about 1e-7 relative on the FID);
  - the trace of (cov_a cov_b)^(1/2) is the sum of the square roots of the eigenvalues of cov_a^(1/2) cov_b cov_a^(1/2), symmetrised and
    clipped at 0, from two numpy.linalg.eigh calls; the reference calls scipy.linalg.sqrtm on the unsymmetric product.  The two agree for
    positive semi-definite inputs; this route never goes complex and needs no eps retry for rank-deficient covariances.  scipy is not
    a dependency;
  - no feature is copied to the host: the reference synchronises device and host once per batch (feat.to('cpu')), here finalize() is
    the one synchronisation.
The count n is known on the host from the shapes of the batches, so FeatureStats keeps it as a Python int and reading it never
synchronises.  `feature_fn` is any callable images [B,3,S,S] -> [B,D] fp32; the reference's network is
transeditor_amd.inception_features.InceptionV3Features (the TensorFlow-FID Inception-v3 up to pool3, on te_conv2d_f32), which the
--dataset and --ckpt modes of the command line build from a local weight file.
"""
import argparse
import json
import pickle
import sys
import types

import numpy as np
import torch

_NO_GPU = 'transeditor_amd.fid needs a GPU (the moment kernels are gfx950 only; there is no CPU path)'


class FeatureStats:
    """n, s = sum x and S = sum x x^T (upper triangle) of every feature row pushed in, fp64 on the device.  update() copies into a staging
    buffer of `chunk` rows and folds each full buffer in; nothing synchronises with the host before finalize()."""

    def __init__(self, dim, chunk=4096, device=None):
        if not isinstance(dim, (int, np.integer)) or isinstance(dim, bool) or not 1 <= dim <= 8192:
            raise ValueError(f'FeatureStats: dim must be an integer in 1..8192, got {dim!r}')
        if not isinstance(chunk, (int, np.integer)) or isinstance(chunk, bool) or chunk < 1:
            raise ValueError(f'FeatureStats: chunk must be a positive integer, got {chunk!r}')
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_GPU)
        self.dim, self.chunk = int(dim), int(chunk)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.S = torch.empty(self.dim, self.dim, device=self.device, dtype=torch.float64)
        self.s = torch.empty(self.dim, device=self.device, dtype=torch.float64)
        self._stage = torch.empty(self.chunk, self.dim, device=self.device, dtype=torch.float32)
        self._fill = 0              # rows waiting in the staging buffer
        self._folded = 0            # rows already in S and s (0: S and s hold nothing yet)

    @property
    def count(self):
        return self._folded + self._fill

    def _fold(self):
        if self._fill:
            from . import _lib
            _lib.fid_moments(self.S, self.s, self._stage[:self._fill], accumulate=self._folded > 0)
            self._folded += self._fill
            self._fill = 0

    @torch.no_grad()
    def update(self, features):
        if not torch.is_tensor(features) or features.ndim != 2:
            raise ValueError(f'FeatureStats.update: features must be a [B,{self.dim}] tensor, got '
                             f'{tuple(features.shape) if torch.is_tensor(features) else type(features).__name__}')
        if features.dtype != torch.float32:
            raise ValueError(f'FeatureStats.update: features must be float32, got {features.dtype}')
        if features.shape[1] != self.dim:
            raise ValueError(f'FeatureStats.update: features must be [B,{self.dim}], got {tuple(features.shape)}')
        if not features.is_cuda:
            raise ValueError(f'FeatureStats.update: features must be on the GPU, got {features.device}')
        at, B = 0, features.shape[0]
        while at < B:
            take = min(self.chunk - self._fill, B - at)
            self._stage[self._fill:self._fill + take].copy_(features[at:at + take])
            self._fill += take
            at += take
            if self._fill == self.chunk:
                self._fold()
        return self

    @torch.no_grad()
    def merge(self, other):
        """add the moments of another FeatureStats of the same dim (another rank's, another call's)"""
        if not isinstance(other, FeatureStats) or other.dim != self.dim:
            raise ValueError(f'FeatureStats.merge: needs a FeatureStats of dim {self.dim}')
        self._fold()
        other._fold()
        if other._folded:
            if self._folded:
                self.S += other.S.to(self.device)
                self.s += other.s.to(self.device)
            else:
                self.S.copy_(other.S)
                self.s.copy_(other.s)
            self._folded += other._folded
        return self

    @torch.no_grad()
    def finalize(self):
        """-> (mean [D], cov [D,D]) float64 numpy arrays: np.mean(x, 0) and np.cov(x, rowvar=False) of everything pushed in"""
        if self.count < 2:
            raise ValueError(f'FeatureStats.finalize: a covariance needs at least 2 samples, got {self.count}')
        from . import _lib
        self._fold()
        with torch.cuda.device(self.device):
            mean, cov = _lib.fid_finalize(self.S, self.s, self._folded)
        return mean.cpu().numpy(), cov.cpu().numpy()


def _sym_sqrt_trace(cov_a, cov_b):
    """tr (cov_a cov_b)^(1/2) = the sum of the square roots of the eigenvalues of cov_a^(1/2) cov_b cov_a^(1/2).  With
    cov_a = V diag(w) V^T the non-zero ones are those of F^T cov_b F, F = V_r diag(sqrt(w_r)) over the r eigenvalues above the numerical
    rank threshold D eps max(w) (numpy.linalg.matrix_rank's): a null direction of cov_a then contributes exactly nothing, instead of the
    square root of an eigenvalue of rounding noise."""
    w, v = np.linalg.eigh((cov_a + cov_a.T) * 0.5)
    keep = w > w.shape[0] * np.finfo(np.float64).eps * max(float(w[-1]), 0.0)
    if not keep.any():
        return 0.0
    f = v[:, keep] * np.sqrt(w[keep])
    m = f.T @ cov_b @ f
    ev = np.linalg.eigh((m + m.T) * 0.5)[0]
    return float(np.sqrt(np.clip(ev, 0.0, None)).sum())


def frechet_distance(mean_a, cov_a, mean_b, cov_b):
    """fid_query.py:45-68 in numpy float64 on the host: |mean_a - mean_b|^2 + tr cov_a + tr cov_b - 2 tr (cov_a cov_b)^(1/2)"""
    mean_a, mean_b = np.asarray(mean_a, np.float64), np.asarray(mean_b, np.float64)
    cov_a, cov_b = np.asarray(cov_a, np.float64), np.asarray(cov_b, np.float64)
    if mean_a.ndim != 1 or mean_b.shape != mean_a.shape or cov_a.shape != (mean_a.shape[0],) * 2 or cov_b.shape != cov_a.shape:
        raise ValueError(f'frechet_distance: needs mean [D] and cov [D,D] twice, got {mean_a.shape}, {cov_a.shape}, {mean_b.shape}, '
                         f'{cov_b.shape}')
    diff = mean_a - mean_b
    return float(diff @ diff + np.trace(cov_a) + np.trace(cov_b) - 2.0 * _sym_sqrt_trace(cov_a, cov_b))


def _stats_of(a, name):
    """a FeatureStats, a (mean, cov) pair or [N,D] features (float32 numpy, uploaded, or an fp32 tensor on the GPU) -> (mean, cov)"""
    if isinstance(a, FeatureStats):
        return a.finalize()
    if isinstance(a, (tuple, list)):
        if len(a) != 2:
            raise ValueError(f'compute_fid: {name} must be a FeatureStats, a (mean, cov) pair or [N,D] features')
        return np.asarray(a[0], np.float64), np.asarray(a[1], np.float64)
    if isinstance(a, np.ndarray):
        if a.dtype != np.float32:
            raise ValueError(f'compute_fid: {name} features must be float32, got {a.dtype}')
    elif torch.is_tensor(a):
        if a.dtype != torch.float32:
            raise ValueError(f'compute_fid: {name} features must be float32, got {a.dtype}')
    else:
        raise ValueError(f'compute_fid: {name} must be a FeatureStats, a (mean, cov) pair or [N,D] features, got {type(a).__name__}')
    if a.ndim != 2 or a.shape[0] < 2 or a.shape[1] < 1:
        raise ValueError(f'compute_fid: {name} features must be [N,D] with N >= 2, got {tuple(a.shape)}')
    if isinstance(a, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_GPU)
        a = torch.from_numpy(np.ascontiguousarray(a)).to('cuda')
    elif not a.is_cuda:
        raise ValueError(f'compute_fid: a {name} feature tensor must be on the GPU (pass numpy float32 to have it uploaded)')
    with torch.cuda.device(a.device):
        return FeatureStats(a.shape[1], chunk=min(max(a.shape[0], 1), 8192)).update(a).finalize()


def compute_fid(a, b):
    """the FID of two sets, each a FeatureStats, a (mean, cov) pair or [N,D] fp32 features -> a Python float"""
    ma, ca = _stats_of(a, 'first')
    mb, cb = _stats_of(b, 'second')
    return frechet_distance(ma, ca, mb, cb)


# ---------------------------------------------------------------------------------------------------------------- statistics files
def load_stats(path):
    """calc_inception.py:115-116's pickle (a dict with 'mean' and 'cov'; other keys are ignored) or an .npz with the same two arrays
    -> (mean, cov) float64"""
    if str(path).endswith('.npz'):
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in ('mean', 'cov') if k in z.files}
    else:
        with open(path, 'rb') as f:
            d = pickle.load(f)
    if not isinstance(d, dict) or 'mean' not in d or 'cov' not in d:
        raise ValueError(f'load_stats: {path} holds no mean and cov')
    mean, cov = np.asarray(d['mean'], np.float64), np.asarray(d['cov'], np.float64)
    if mean.ndim != 1 or cov.shape != (mean.shape[0],) * 2:
        raise ValueError(f'load_stats: {path}: mean {mean.shape} and cov {cov.shape} are not [D] and [D,D]')
    return mean, cov


def save_stats(path, mean, cov, **extra):
    """write (mean, cov) and any extra keys as calc_inception.py's pickle, or as .npz where the path ends so"""
    mean, cov = np.asarray(mean), np.asarray(cov)
    if str(path).endswith('.npz'):
        np.savez(path, mean=mean, cov=cov, **extra)
    else:
        with open(path, 'wb') as f:
            pickle.dump({'mean': mean, 'cov': cov, **extra}, f)


# ---------------------------------------------------------------------------------------------------------------- generator / dataset
def _push(stats, f, b, who):
    if f.ndim != 2 or f.shape[0] != b:
        raise ValueError(f'{who}: feature_fn must return [B,D] features, got {tuple(f.shape)} for a batch of {b}')
    if stats is None:
        with torch.cuda.device(f.device):
            stats = FeatureStats(f.shape[1])
    return stats.update(f.float())


@torch.no_grad()
def fake_stats(generator, feature_fn, *, n_sample=50000, batch=64, truncation=1.0, seed=None, latent=512, para_num=16):
    """fid_query.py:24-42: feature_fn over n_sample generated images, the codes drawn as prdc.fake_features draws them and both
    multiplied by `truncation`; every batch's features go straight into a FeatureStats, which is returned.  As in the reference, both
    mapping networks open with a PixelNorm, so this scaling reaches the images only through the norm's 1e-8 epsilon."""
    from .metrics import _as_sampler, batch_sizes
    from .utils.sample import prepare_noise_new, prepare_param
    sizes = batch_sizes(n_sample, batch)
    if not sizes:
        raise ValueError('fake_stats: n_sample must be positive')
    g = _as_sampler(generator)
    device = next(g.g.parameters()).device
    args = types.SimpleNamespace(latent=latent, para_num=para_num)
    stats = None
    with torch.random.fork_rng(devices=[device] if device.type == 'cuda' else [], enabled=seed is not None):
        if seed is not None:
            torch.manual_seed(seed)
        for b in sizes:
            z = prepare_noise_new(b, args, device, method='query')
            p = prepare_param(b, args, device, method='spatial')
            if truncation != 1.0:
                z, p = z * truncation, p * truncation
            image, _, _ = g(z, p)
            stats = _push(stats, feature_fn(image), b, 'fake_stats')
    return stats


@torch.no_grad()
def dataset_stats(dataset, feature_fn, *, n_sample, batch, seed=None):
    """calc_inception.py:60-111: feature_fn over n_sample images of `dataset` (any object with __len__ and __getitem__ -> [3,S,S] tensors
    in [-1, 1]), the head of one seeded permutation as prdc.dataset_features takes it -> the FeatureStats"""
    from .metrics import batch_sizes
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    n = len(dataset)
    if not isinstance(n_sample, int) or n_sample < 1 or n_sample > n:
        raise ValueError(f'dataset_stats: n_sample must be in 1..len(dataset) = {n} (sampling is without replacement), got {n_sample}')
    order = torch.randperm(n) if seed is None else torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    order = order[:n_sample].tolist()
    stats, at = None, 0
    for b in batch_sizes(n_sample, batch):
        images = torch.stack([torch.as_tensor(dataset[i]) for i in order[at:at + b]]).to('cuda')
        at += b
        stats = _push(stats, feature_fn(images), b, 'dataset_stats')
    return stats


def evaluate_fid(generator, feature_fn, real_stats, **kw):
    """fid_query.py's run for one generator: fake_stats(generator, feature_fn, **kw) against real_stats (anything compute_fid takes,
    or the path of a statistics file) -> a Python float"""
    if isinstance(real_stats, str):
        real_stats = load_stats(real_stats)
    return compute_fid(fake_stats(generator, feature_fn, **kw), real_stats)


# ------------------------------------------------------------------------------------------------------------------------ CLI
class _Parser(argparse.ArgumentParser):
    """five modes that exclude each other; parse_args sets args.mode = 'files' | 'stats' | 'write' (from feature files) |
    'dataset' (a dataset through the Inception network into a statistics file) | 'model' (a checkpoint against statistics)"""

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if a.ckpt is not None:
            if any(v is not None for v in (a.real, a.fake, a.features, a.write_stats)):
                self.error('--ckpt (a checkpoint through the Inception network) excludes --real, --fake, --features and --write_stats')
            if (a.stats is None) == (a.dataset is None):
                self.error('--ckpt needs the real statistics: exactly one of --stats (a file) and --dataset (computed on the fly)')
            if a.size < 32 or a.size & (a.size - 1):
                self.error(f'--size must be a power of two >= 32, got {a.size}')
            a.mode = 'model'
            return a
        if a.dataset is not None:
            if a.write_stats is None:
                self.error('--dataset needs --write_stats (the statistics file to write) or --ckpt (a checkpoint to evaluate)')
            if any(v is not None for v in (a.real, a.fake, a.stats, a.features)):
                self.error('--dataset / --write_stats (write a statistics file) exclude --real, --stats, --fake and --features')
            a.mode = 'dataset'
            return a
        if a.inception is not None:
            self.error('--inception (the network weights) goes with --dataset or --ckpt; the other modes start from features')
        if (a.features is None) != (a.write_stats is None):
            self.error('--features and --write_stats go together')
        if a.features is not None:
            if a.real is not None or a.fake is not None or a.stats is not None:
                self.error('--features / --write_stats (write a statistics file) exclude --real, --stats and --fake')
            a.mode = 'write'
            return a
        if a.real is not None and a.stats is not None:
            self.error('--real (a feature file) and --stats (a statistics file) exclude each other')
        if a.real is None and a.stats is None:
            self.error('give --real and --fake, --stats and --fake, --features and --write_stats, --dataset and --write_stats, or --ckpt')
        if a.fake is None:
            self.error('--real / --stats need --fake')
        a.mode = 'files' if a.real is not None else 'stats'
        return a


def build_parser():
    parser = _Parser(description='Frechet inception distance (metrics/fid_query.py) of two feature files (--real, --fake) or of a '
                                 'statistics file against a feature file (--stats, --fake); write the statistics file of a feature '
                                 'file (--features, --write_stats) or of a dataset through the Inception network (--dataset, '
                                 '--write_stats: metrics/calc_inception.py); or evaluate a checkpoint (--ckpt with --stats or --dataset)')
    parser.add_argument('--real', help='.npy file of the real features [N,D], float32')
    parser.add_argument('--fake', help='.npy file of the generated features [M,D], float32')
    parser.add_argument('--stats', help="statistics of the real set: calc_inception.py's pickle, or an .npz with mean and cov")
    parser.add_argument('--features', help='.npy file of features [N,D], float32, whose statistics are written')
    parser.add_argument('--write_stats', help='output statistics file (.pkl as calc_inception.py writes it, or .npz)')
    parser.add_argument('--ckpt', help='a checkpoint file, or a directory of <iteration>.pt files')
    parser.add_argument('--dataset', help='LMDB directory of the real images (utils/dataset.py MultiResolutionDataset)')
    parser.add_argument('--inception', default=None, help='pytorch-fid Inception-v3 state dict (default: the torch hub cache path)')
    parser.add_argument('--size', type=int, default=256)
    parser.add_argument('--n_sample', type=int, default=50000)
    parser.add_argument('--batch', type=int, default=64)
    parser.add_argument('--start_num', type=int, default=0)
    parser.add_argument('--truncation', type=float, default=1.0)
    parser.add_argument('--seed', type=int, default=None, help='seed of the generated codes and of the choice of real images')
    parser.add_argument('--flip', action='store_true', help='random horizontal flips of the real images (calc_inception.py --flip)')
    parser.add_argument('--para_num', type=int, default=16)
    parser.add_argument('--channel_multiplier', type=int, default=2)
    parser.add_argument('--num_trans', type=int, default=8)
    return parser


def _dataset_stats_of(args, net):
    """calc_inception.py:93-111: the statistics of min(n_sample, len) images of the LMDB dataset at --size"""
    from .utils.dataset import MultiResolutionDataset, image_transform
    dataset = MultiResolutionDataset(args.dataset, image_transform(flip_probability=0.5 if args.flip else 0), args.size)
    n = min(args.n_sample, len(dataset))
    return dataset_stats(dataset, net, n_sample=n, batch=args.batch, seed=args.seed), n


def _network_modes(args):
    import math
    from .inception_features import InceptionV3Features
    net = InceptionV3Features(args.inception)
    if args.mode == 'dataset':
        stats, n = _dataset_stats_of(args, net)
        mean, cov = stats.finalize()
        save_stats(args.write_stats, mean, cov, size=args.size, path=args.dataset)              # calc_inception.py:115-116's keys
        res = {'metric': 'fid_stats', 'dataset': args.dataset, 'n': n, 'dim': int(mean.shape[0]), 'wrote': args.write_stats}
        print(json.dumps(res), flush=True)
        return res
    from .inference import GeneratorSampler
    from .metrics import checkpoints
    from .model_spatial_query import Generator
    from .train_step import load_checkpoint_into
    real = load_stats(args.stats) if args.stats is not None else _dataset_stats_of(args, net)[0].finalize()
    results = []
    for model_path in checkpoints(args.ckpt, args.start_num):
        g = Generator(args.size, 512, 512, 2 * (int(math.log(args.size, 2)) - 1), channel_multiplier=args.channel_multiplier,
                      n_trans=args.num_trans, pixel_norm_op_dim=1).to('cuda')
        load_checkpoint_into(model_path, g, device='cuda', g_ema_only_ok=True)
        res = {'metric': 'fid', 'ckpt': model_path, 'stats': args.stats, 'dataset': args.dataset, 'n_fake': args.n_sample,
               'truncation': args.truncation}
        res['fid'] = evaluate_fid(GeneratorSampler(g), net, real, n_sample=args.n_sample, batch=args.batch, truncation=args.truncation,
                                  seed=args.seed, para_num=args.para_num)
        print(json.dumps(res), flush=True)
        results.append(res)
    return results


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    if args.mode in ('dataset', 'model'):
        return _network_modes(args)
    if args.mode == 'write':
        f = np.load(args.features, allow_pickle=False)
        mean, cov = _stats_of(f, '--features')
        save_stats(args.write_stats, mean, cov)
        res = {'metric': 'fid_stats', 'features': args.features, 'n': int(f.shape[0]), 'dim': int(f.shape[1]), 'wrote': args.write_stats}
    else:
        fake = np.load(args.fake, allow_pickle=False)
        res = {'metric': 'fid', 'fake': args.fake, 'n_fake': int(fake.shape[0])}
        if args.mode == 'files':
            real = np.load(args.real, allow_pickle=False)
            res.update(real=args.real, n_real=int(real.shape[0]))
        else:
            real = load_stats(args.stats)
            res.update(stats=args.stats)
        res['fid'] = compute_fid(real, fake)
    print(json.dumps(res), flush=True)
    return res


if __name__ == '__main__':
    main(sys.argv[1:])

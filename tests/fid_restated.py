"""The FID pipeline restated in numpy float64: the one-pass moments n, s, S; np.mean / np.cov; the Frechet distance by the symmetric
eigenvalue route (written here independently of transeditor_amd.fid); the draws of the golden cases; and the |x_i||x_j| bound arrays of
the fp64 summation."""
import numpy as np

CASES = {'a': ((257, 96), (130, 96)), 'b': ((40, 64), (50, 64)), 'c': ((300, 33), (300, 33))}
SEED = 2


def draw(real_shape, fake_shape, rng):
    """real = max(N(0,1) A + 0.4, 0) with A a D x D mixing matrix scaled by 1 / sqrt(D) (drawn after the normals), then
    fake = max(0.9 N(0,1) + 0.3, 0); both float32"""
    D = real_shape[1]
    z = rng.standard_normal(real_shape)
    A = rng.standard_normal((D, D)) / np.sqrt(D)
    real = np.maximum(z @ A + 0.4, 0.0).astype(np.float32)
    fake = np.maximum(0.9 * rng.standard_normal(fake_shape) + 0.3, 0.0).astype(np.float32)
    return real, fake


def draw_all():
    """the golden cases, each from its own np.random.default_rng(SEED) -> {case: (real, fake)}"""
    return {name: draw(rs, fs, np.random.default_rng(SEED)) for name, (rs, fs) in CASES.items()}


def moments(x):
    """-> (n, s [D], S [D,D]) in float64, uncentred, one pass"""
    x = np.asarray(x, np.float64)
    return x.shape[0], x.sum(0), x.T @ x


def abs_moments(x):
    """sum_k |x_ki| |x_kj|: what the rounding of any summation order of S is bounded by"""
    a = np.abs(np.asarray(x, np.float64))
    return a.T @ a


def mean_cov(x):
    x = np.asarray(x, np.float64)
    return x.mean(0), np.atleast_2d(np.cov(x, rowvar=False))


def one_pass_mean_cov(x):
    n, s, S = moments(x)
    return s / n, (S - np.outer(s, s) / n) / (n - 1)


def psd_sqrt(c):
    w, v = np.linalg.eigh((c + c.T) / 2)
    return (v * np.sqrt(np.maximum(w, 0.0))) @ v.T


def frechet(mean_a, cov_a, mean_b, cov_b):
    r = psd_sqrt(cov_a)
    m = r @ cov_b @ r
    ev = np.linalg.eigvalsh((m + m.T) / 2)
    d = mean_a - mean_b
    return float(d @ d + np.trace(cov_a) + np.trace(cov_b) - 2 * np.sqrt(np.maximum(ev, 0.0)).sum())


def fid_of_features(a, b):
    return frechet(*mean_cov(a), *mean_cov(b))

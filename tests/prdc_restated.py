"""metrics/prdc.py restated in numpy float64 on SQUARED distances: d2(i,j) = sum_k (x[i,k] - y[j,k])^2 formed directly (no norm
expansion), the diagonal of a set against itself exactly 0 (sklearn's X-is-Y path), thresholds the squared radii, strict <."""
import numpy as np


def sq_distances(x, y):
    """[N,D], [M,D] -> [N,M] float64, in row blocks so the difference tensor stays small"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.empty((x.shape[0], y.shape[0]))
    step = max(1, (1 << 22) // max(1, y.shape[0] * x.shape[1]))
    for a in range(0, x.shape[0], step):
        d = x[a:a + step, None, :] - y[None, :, :]
        out[a:a + step] = np.einsum('ijk,ijk->ij', d, d)
    return out


def radii2(x, k):
    """prdc.py:41-51: element k of every sorted row of the self-distance matrix (the k+1 smallest, the self-distance 0 among them)"""
    d = sq_distances(x, x)
    np.fill_diagonal(d, 0.0)
    return np.sort(d, axis=1)[:, k]


def details(real, fake, k):
    """-> dict(rr2 [N], rf2 [M], d2 [N,M], col_count [M] int64, row_any [N] bool, row_min [N])"""
    rr2, rf2 = radii2(real, k), radii2(fake, k)
    d2 = sq_distances(real, fake)
    inside_real = d2 < rr2[:, None]                                            # :75-78 / :85-88
    return dict(rr2=rr2, rf2=rf2, d2=d2, col_count=inside_real.sum(0), row_any=(d2 < rf2[None, :]).any(1),   # :80-83
                row_min=d2.min(1))                                             # :90-93


def numbers(d, k):
    """the four values as exact ratios of counts"""
    n, m = d['rr2'].shape[0], d['rf2'].shape[0]
    return dict(precision=int((d['col_count'] > 0).sum()) / m, recall=int(d['row_any'].sum()) / n,
                density=int(d['col_count'].sum()) / (float(k) * m), coverage=int((d['row_min'] < d['rr2']).sum()) / n)


def compute_prdc(real, fake, k):
    return numbers(details(real, fake, k), k)


def min_relative_gap(d):
    """the smallest relative distance between any d2 and a threshold it is compared with (fp64): a condition on the INPUTS under which
    an fp32 evaluation with a smaller relative error must reproduce every comparison"""
    d2, rr2, rf2 = d['d2'], d['rr2'], d['rf2']
    g = [np.abs(d2 - rr2[:, None]) / rr2[:, None], np.abs(d2 - rf2[None, :]) / rf2[None, :], np.abs(d['row_min'] - rr2) / rr2]
    return min(float(x.min()) for x in g)

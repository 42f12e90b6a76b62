"""The linear C-SVC of an editing boundary restated in numpy float64: libsvm's SMO (second-order working-set selection, no shrinking) on
a GIVEN Gram matrix, exactly the algorithm of csrc/svm.hip, plus the seeded cases of tests/golden/boundary_ref.npz
(tools/gen_boundary_golden.py) and the training-set rule of train_boundary.py:45-82 at split_ratio = 1."""
import numpy as np

TAU = 1e-12
#        N     D   ratio or count  score noise  seed
CASES = {'a': (1500, 96, 0.04, 0.5, 7),
         'b': (2000, 8, 0.05, 2.0, 7),
         'c': (600, 33, 65, 1.0, 7)}


def draw(case):
    """codes [N,D] float32 standard normal, scores [N,1] float32 = a random unit linear functional of the codes plus noise"""
    N, D, _, noise, seed = CASES[case]
    rng = np.random.default_rng(seed)
    codes = rng.standard_normal((N, D)).astype(np.float32)
    u = rng.standard_normal(D)
    scores = codes.astype(np.float64) @ (u / np.linalg.norm(u)) + noise * rng.standard_normal(N)
    return codes, scores.astype(np.float32).reshape(N, 1)


def training_set(codes, scores, chosen_num_or_ratio):
    """train_boundary.py:54-82 with split_ratio = 1 and no shuffle: (rows [n,D], labels [n] = +1 for the top scores, -1 for the bottom)"""
    order = np.argsort(scores, axis=0)[::-1, 0]
    n = codes.shape[0]
    chosen = int(n * chosen_num_or_ratio) if 0 < chosen_num_or_ratio <= 1 else int(chosen_num_or_ratio)
    chosen = min(chosen, n // 2)
    rows = np.concatenate([codes[order[:chosen]], codes[order[-chosen:]]], axis=0)
    return rows, np.concatenate([np.ones(chosen, np.int8), -np.ones(chosen, np.int8)])


def gram32(x):
    """x x^T with the fp32 rounding of the stored entries (libsvm's Qfloat); the order of summation is numpy's, not the kernel's"""
    x = np.asarray(x, np.float32)
    return (x.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)


def bounds(y, a, C):
    """(I_up, I_low) of the C-SVC dual"""
    return np.where(y > 0, a < C, a > 0), np.where(y > 0, a > 0, a < C)


def extremes(K, y, alpha, C):
    """(Gmax, Gmin) of the dual at alpha: the largest -y_t G_t over I_up and the smallest over I_low, recomputed in float64"""
    K, y, alpha = np.asarray(K, np.float64), np.asarray(y, np.float64), np.asarray(alpha, np.float64)
    v = -y * ((K * np.outer(y, y)) @ alpha - 1.0)
    up, low = bounds(y, alpha, C)
    return float(v[up].max()), float(v[low].min())


def violation(K, y, alpha, C):
    """Gmax - Gmin: the stop criterion's left side"""
    gmax, gmin = extremes(K, y, alpha, C)
    return gmax - gmin


def smo(K, y, C=1.0, eps=1e-3, max_iter=1_000_000):
    """-> (alpha [n], rho, iterations, converged): min 1/2 a^T Q a - e^T a, 0 <= a <= C, y^T a = 0, Q = y y^T * K.  Ties in both
    selections go to the lowest index (np.argmax)."""
    K, y = np.asarray(K, np.float64), np.asarray(y, np.float64)
    n, qd = y.shape[0], np.diag(K).copy()
    a, G, it, converged = np.zeros(n), -np.ones(n), 0, False
    while it < max_iter:
        v = -y * G
        up, low = bounds(y, a, C)
        i = int(np.argmax(np.where(up, v, -np.inf)))
        b = v[i] - v
        q = qd[i] + qd - 2.0 * K[i]
        q = np.where(q > 0, q, TAU)
        cand = low & (b > 0) & up[i]
        if not cand.any() or v[i] - v[low].min() < eps:
            converged = True
            break
        j = int(np.argmax(np.where(cand, b * b / q, -np.inf)))
        ai, aj = a[i], a[j]
        if y[i] != y[j]:
            delta, diff = (-G[i] - G[j]) / q[j], ai - aj
            ai, aj = ai + delta, aj + delta
            if diff > 0:
                if aj < 0:
                    ai, aj = diff, 0.0
                if ai > C:
                    ai, aj = C, C - diff
            else:
                if ai < 0:
                    ai, aj = 0.0, -diff
                if aj > C:
                    ai, aj = C + diff, C
        else:
            delta, s = (G[i] - G[j]) / q[j], ai + aj
            ai, aj = ai - delta, aj + delta
            if s > C:
                if ai > C:
                    ai, aj = C, s - C
                if aj > C:
                    ai, aj = s - C, C
            else:
                if aj < 0:
                    ai, aj = s, 0.0
                if ai < 0:
                    ai, aj = 0.0, s
        G += (y * y[i] * K[i]) * (ai - a[i]) + (y * y[j] * K[j]) * (aj - a[j])
        a[i], a[j] = ai, aj
        it += 1
    yG, free = y * G, (a > 0) & (a < C)
    ub = yG[((a >= C) & (y < 0)) | ((a <= 0) & (y > 0))]
    lb = yG[((a >= C) & (y > 0)) | ((a <= 0) & (y < 0))]
    rho = yG[free].mean() if free.any() else (ub.min() + lb.max()) / 2.0
    return a, float(rho), it, converged


def direction(x, y, alpha):
    """sum_i alpha_i y_i x_i in float64, divided by its norm -> [D]"""
    w = (np.asarray(alpha, np.float64) * np.asarray(y, np.float64)) @ np.asarray(x, np.float64)
    return w / np.linalg.norm(w)


def one_minus_cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(1.0 - a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))

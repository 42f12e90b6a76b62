"""The linear C-SVC of an editing boundary restated in numpy float64: libsvm's SMO (second-order working-set selection, no shrinking) on
a GIVEN Gram matrix, exactly the algorithm of csrc/svm.hip, plus the seeded cases of tests/golden/boundary_ref.npz and
boundary_ref_large.npz (tools/gen_boundary_golden.py), the training-set rule of train_boundary.py:45-82 at split_ratio = 1, and the
synthetic problems of the tests above 1024 rows (margin_problem, tie_problem), where a thread of the one-workgroup solver owns several
rows ("slots": row idx sits in slot idx // 1024 of thread idx % 1024)."""
import numpy as np

TAU = 1e-12
#        N     D   ratio or count  score noise  seed
CASES = {'a': (1500, 96, 0.04, 0.5, 7),
         'b': (2000, 8, 0.05, 2.0, 7),
         'c': (600, 33, 65, 1.0, 7),
         'd': (6000, 12, 0.35, 1.0, 7)}            # n = 4200, the reference's default size; tests/golden/boundary_ref_large.npz
SMALL_CASES, LARGE_CASES = ('a', 'b', 'c'), ('d',)
SLOT = 1024                                        # threads of the solver's workgroup


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
    v = -y * (y * (K @ (y * alpha)) - 1.0)                    # Q alpha - e with Q = y y^T * K: the signs are exact, no n x n temporary
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


# ---------------------------------------------------------------------------------------------------------- problems above 1024 rows
def slots(index):
    """the sorted slots (idx // 1024) that the rows `index` fall in"""
    return sorted({int(i) // SLOT for i in np.atleast_1d(index)})


def margin_problem(n, D=16, margin=0.5, noise=0.3, hardest_last=True):
    """(x [n,D] float32, y [n] int8) from default_rng(n): x ~ N(0, 1) in fp32, a random unit u, y = sign(x . u + noise * N(0, 1)), every
    row pushed by margin * y * u.  hardest_last: the rows sorted by their distance |x . u| to the boundary, the nearest at the highest
    indices, so that every support vector (and every selected i and j) lies in the last slots; else the random order of the draw."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, D)).astype(np.float32)
    u = rng.standard_normal(D)
    u /= np.linalg.norm(u)
    y = np.where(x.astype(np.float64) @ u + noise * rng.standard_normal(n) > 0, 1, -1).astype(np.int8)
    x = (x.astype(np.float64) + margin * y[:, None] * u[None, :]).astype(np.float32)
    if hardest_last:
        order = np.argsort(-np.abs(x.astype(np.float64) @ u), kind='stable')
        x, y = np.ascontiguousarray(x[order]), np.ascontiguousarray(y[order])
    return x, y


# Two rows whose Gram entries 1.25, 1.0625 and -1 are exact in fp32: K_pp + K_qq - 2 K_pq = 4.3125, so the unconstrained step is
# 2 / 4.3125 = 0.4638 per class: one iteration at C = 1, and at C = 0.125 three full steps and a partial one (4 iterations).
TIE_ROWS = np.array([[1.0, 0.5, 0.0], [-1.0, 0.0, 0.25]], np.float32)
TIE_N = 2050
# layout -> the rows of the class placed by hand (the other class takes the rest, so its lowest rows are 0, 1, 2, ...).  Sorted, the
# first two are the pair a wrong preference would swap; at least five rows, so the box C = 0.125 fills four of them in order.
TIE_LAYOUTS = {
    'i_two_slots_of_one_thread': [5] + list(range(1029, 1041)),           # 5 and 1029 = 5 + 1024: thread 5, slots 0 and 1
    'ii_high_lane_then_lane0_of_a_later_wave': [191, 256, 257, 258, 300, 1500],    # lane 63 of wave 2, then lane 0 of wave 4
    'iii_wave15_slot0_then_wave0_slot1': list(range(1023, 1031)),         # 1023: wave 15, slot 0; 1024: wave 0, slot 1
    'iv_blocks': list(range(1030, 2050)),                                 # the classes are 0 .. 1029 and 1030 .. 2049
    'v_low_lane_holds_the_higher_row': [60, 1027, 1028, 1090, 1091, 2049],         # wave 0: lane 60 holds 60, lane 3 holds 1027
}


def tie_problem(layout, flip=False):
    """(K [n,n] float32, y [n] int8), n = 2050: all rows of a class are the same vector, so every working-set selection is a tie among
    all candidates of a class.  The rows TIE_LAYOUTS[layout] are +1 (selection A sees their tie first), with flip -1 (selection B)."""
    placed = np.zeros(TIE_N, bool)
    placed[TIE_LAYOUTS[layout]] = True
    y = np.where(placed ^ flip, 1, -1).astype(np.int8)
    cls = (y < 0).astype(np.intp)                                          # +1 rows are TIE_ROWS[0]
    base = gram32(TIE_ROWS)
    return np.ascontiguousarray(base[cls][:, cls]), y


def tie_support(y, C):
    """what the lowest-index rule must give on a tie_problem, worked out by hand: the k lowest rows of each class, k = 1 iteration at
    C = 1 and 4 at C = 0.125 -> (sorted support indices, iterations)"""
    k = {1.0: 1, 0.125: 4}[C]
    idx = np.arange(len(y))
    return sorted(idx[y > 0][:k].tolist() + idx[y < 0][:k].tolist()), k

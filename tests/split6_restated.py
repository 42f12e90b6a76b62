"""The split-bf16 arithmetic of csrc/split6_common.h restated in plain torch on the CPU, and the three instruments that
tests/test_gpu_split6_forms.py holds the kernels to.  Importable without a GPU and without the library.

The family's numeric claim: an fp32 operand v is three bf16 pieces, h = bf16(v), m = bf16(v - h), l = bf16(v - h - m) (both
subtractions in fp32, where they are exact), and a multiply-add is the six piece products mm, hl, lh, hm, mh, hh (first letter: the
piece of the first operand), each exact in fp32, accumulated in fp32 with the five small ones kept apart from hh.  emulate() builds the
arithmetic of every kind of the family from split3 and six_products:
    'direct9'   the nine-tap sum of the strided kind (S2S6; T2S6's body is the same sum read the other way)
    'tap1'      the one-tap sum (1X1S6)
    'wino_row'  the F(2,3) row form of wino6: V = B^T d over column pairs in fp32, U = G w in fp32, both split, four component sums,
                out = A^T M in fp32
    'wg_pair'   the pair form of wgrad6: u = [g0, g0 + g1, g0 - g1, -g1], t = B^T e in fp32, both split, four sums per kernel row,
                folded to three taps in fp32
    'wg_tap1'   the 1x1 weight gradient: the one-tap sum over pixels
`drop` leaves a product out, `swap` exchanges the m and l pieces of one operand: the smallest defects the family can grow (a lost
product of weight 2^-16 or 2^-17 of the sum's terms).  yardstick() is torch's fp32 result of the same operation, reference() the fp64 one.

The instruments.  Worst-case elementwise bounds cannot see such a defect from about 32 channels up: L u already exceeds 2^-17.  What
separates an intact kernel from a mutated one is
    grouped_rms   per structural group of outputs, rms(got - ref) <= RMS_FACTOR rms(fp32 - ref) + RMS_FLOOR rms(ref): the family's
                  whole-tensor L2 figure applied to the groups in which a defect would be confined (one wave, one tile line, one slot)
    live_rms      one live channel (nine products per output, or one): rms(got - ref) <= bar rms(ref) per group; the intact split
                  sits at 2^-25, fp32 at 2^-24, the smallest defect at 2^-18.5, the bar LIVE_BAR = 2^-21 about eight times from either
Groups are integer label tensors that broadcast against the output; a group below MIN_GROUP elements is pooled with its neighbours
(labels in ascending order), never skipped.
"""
import torch
import torch.nn.functional as F

PRODUCTS = ('mm', 'hl', 'lh', 'hm', 'mh', 'hh')              # the order of split6_product
PIECE = {'h': 0, 'm': 1, 'l': 2}
RMS_FACTOR, RMS_FLOOR = 2.5, 1e-7
LIVE_BAR = 2.0 ** -21
MIN_GROUP = 512
KINDS = ('direct9', 'tap1', 'wino_row', 'wg_pair', 'wg_tap1')


def split3(v):
    """(h, m, l) of an fp32 tensor, each bf16-valued and held in fp32"""
    assert v.dtype == torch.float32
    h = v.bfloat16().float()
    r = v - h
    m = r.bfloat16().float()
    l = (r - m).bfloat16().float()
    return h, m, l


def six_products(a_pieces, b_pieces, mm, drop=None, swap=None):
    """sum of the piece products of mm(a, b), an fp32 contraction: the five small ones in the kernels' order, then + hh.
    drop: a name of PRODUCTS to leave out; swap: 'a' or 'b', the operand whose m and l pieces change places"""
    a, b = list(a_pieces), list(b_pieces)
    if swap == 'a':
        a[1], a[2] = a[2], a[1]
    elif swap == 'b':
        b[1], b[2] = b[2], b[1]
    else:
        assert swap is None
    assert drop is None or drop in PRODUCTS
    small = None
    for name in PRODUCTS[:5]:
        if name == drop:
            continue
        p = mm(a[PIECE[name[0]]], b[PIECE[name[1]]])
        small = p if small is None else small + p
    if drop == 'hh':
        return small
    return mm(a[0], b[0]) + small


# ---- the kinds.  Each is (transform of the two operands in `dt`, contraction, output transform in `dt`); w / g is the first operand.
def _wino_v(x):
    """B^T d of F(2,3) over the column pairs of the zero-padded image: [4][B, K, H + 2, W / 2]"""
    xp = F.pad(x, (1, 1, 1, 1))
    W = x.shape[-1]
    d = [xp[..., k:k + W:2] for k in range(4)]
    return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]


def _wino_u(w):
    """G w of F(2,3) along kx: [4][M, K, 3, 1]"""
    w0, w1, w2 = w[..., 0:1], w[..., 1:2], w[..., 2:3]
    return [w0, 0.5 * (w0 + w1 + w2), 0.5 * (w0 - w1 + w2), w2]


def _pairs(t):
    return t[..., 0::2], t[..., 1::2]


def _wg_u(g):
    g0, g1 = _pairs(g)
    return [g0, g0 + g1, g0 - g1, -g1]


def _wg_t(x):
    """B^T e per kernel row ky over the column pairs: [3][4][B, Ci, H, W / 2]"""
    xp = F.pad(x, (1, 1, 1, 1))
    H, W = x.shape[-2:]
    rows = []
    for ky in range(3):
        e = [xp[..., ky:ky + H, k:k + W:2] for k in range(4)]
        rows.append([e[0] - e[2], e[1] + e[2], e[2] - e[1], e[1] - e[3]])
    return rows


def _corr(u, t):
    return torch.einsum('bohw,bihw->oi', u, t)


def _run(kind, a, b, product):
    """the kind's arithmetic with `product(A, B, mm)` standing for one transformed-operand contraction"""
    if kind == 'direct9':
        return product(a, b, lambda w, x: F.conv2d(x, w, stride=2))
    if kind == 'tap1':
        return product(a, b, lambda w, x: F.conv2d(x, w))
    if kind == 'wino_row':
        U, V = _wino_u(a), _wino_v(b)
        M = [product(U[c], V[c], lambda u, v: F.conv2d(v, u)) for c in range(4)]
        out = torch.stack([M[0] + M[1] + M[2], M[1] - M[2] - M[3]], -1)
        return out.flatten(-2)
    if kind == 'wg_pair':
        u, rows = _wg_u(a), _wg_t(b)
        taps = []
        for ky in range(3):
            m = [product(u[c], rows[ky][c], _corr) for c in range(4)]
            hs = 0.5 * (m[1] + m[2])
            taps += [m[0] + hs, 0.5 * (m[1] - m[2]), hs + m[3]]
        return torch.stack(taps, -1)
    assert kind == 'wg_tap1', kind
    return product(a, b, _corr)[..., None]


def emulate(kind, a, b, drop=None, swap=None):
    """the split kernel's result restated: a = weights [M, K, k, k] (conv kinds) or g [B, Co, H, W] (weight gradients), b = x"""
    return _run(kind, a, b, lambda A, B, mm: six_products(split3(A), split3(B), mm, drop, swap))


def yardstick(kind, a, b):
    """torch's fp32 result of the same operation (the untransformed one for the two Winograd-transformed kinds)"""
    return _plain(kind, a, b)


def reference(kind, a, b):
    return _plain(kind, a.double(), b.double())


def _plain(kind, a, b):
    if kind == 'direct9':
        return F.conv2d(b, a, stride=2)
    if kind == 'tap1':
        return F.conv2d(b, a)
    if kind == 'wino_row':
        return F.conv2d(b, a, padding=1)
    if kind == 'wg_pair':
        return torch.nn.grad.conv2d_weight(b, (a.shape[1], b.shape[1], 3, 3), a, padding=1).flatten(-2)
    return _corr(a, b)[..., None]


def abs_sum(kind, a, b):
    """S of the elementwise bound in fp64: the sum of the absolute values of the products that reach an output, propagated through
    the transforms for the two transformed kinds (|A^T| (|G||w| . |B^T||x|), every subtraction an addition)"""
    a, b = a.double().abs(), b.double().abs()
    if kind == 'wino_row':
        w0, w1, w2 = a[..., 0:1], a[..., 1:2], a[..., 2:3]
        U = [w0, 0.5 * (w0 + w1 + w2), 0.5 * (w0 + w1 + w2), w2]
        xp = F.pad(b, (1, 1, 1, 1))
        W = b.shape[-1]
        d = [xp[..., k:k + W:2] for k in range(4)]
        V = [d[0] + d[2], d[1] + d[2], d[2] + d[1], d[1] + d[3]]
        M = [F.conv2d(V[c], U[c]) for c in range(4)]
        return torch.stack([M[0] + M[1] + M[2], M[1] + M[2] + M[3]], -1).flatten(-2)
    if kind == 'wg_pair':
        g0, g1 = _pairs(a)
        u = [g0, g0 + g1, g0 + g1, g1]
        xp = F.pad(b, (1, 1, 1, 1))
        H, W = b.shape[-2:]
        taps = []
        for ky in range(3):
            e = [xp[..., ky:ky + H, k:k + W:2] for k in range(4)]
            t = [e[0] + e[2], e[1] + e[2], e[2] + e[1], e[1] + e[3]]
            A = [_corr(u[c], t[c]) for c in range(4)]
            mid = 0.5 * (A[1] + A[2])
            taps += [A[0] + mid, mid, mid + A[3]]
        return torch.stack(taps, -1)
    return _plain(kind, a, b)


# ---- the instruments
def _rms(t):
    return float(t.double().pow(2).mean().sqrt()) if t.numel() else 0.0


def group_sums(label, shape, keep, squares):
    """(counts, [sums]) per value 0 .. max of an integer label tensor that broadcasts to `shape`: the kept elements of each group and
    the sum of every tensor of `squares` over them.  Negative labels belong to no group.  The axes along which the label does not vary
    are summed first, so a group costs one pass over the tensors."""
    dev = squares[0].device
    label = label.to(dev).view((1,) * (len(shape) - label.dim()) + tuple(label.shape))
    dims = [i for i in range(len(shape)) if label.shape[i] == 1 and shape[i] != 1]
    red = (lambda t: t.sum(dims, keepdim=True)) if dims else (lambda t: t)
    if keep is not None:
        w = keep.to(dev).double()
        cnt_t, squares = red(w), [t * w for t in squares]
    else:
        cnt_t = None
    sums_t = [red(t.double()) for t in squares]
    lab = label.expand(sums_t[0].shape).reshape(-1).long().clamp_min(-1) + 1
    n = int(lab.max()) + 1
    per = 1
    for i in dims:
        per *= shape[i]
    cnt = torch.bincount(lab, minlength=n).double() * per if cnt_t is None else torch.bincount(lab, weights=cnt_t.reshape(-1), minlength=n)
    return cnt[1:].round().long().cpu(), [torch.bincount(lab, weights=t.reshape(-1), minlength=n)[1:].cpu() for t in sums_t]


def pooled(counts, min_group=MIN_GROUP):
    """the groups as lists of label values, ascending: a label with fewer than min_group elements is pooled with the next ones (what is
    left at the end with the pool before it), never skipped; labels without elements belong to no pool"""
    pools, cur, n = [], [], 0
    for v, c in enumerate(counts.tolist()):
        if c == 0:
            continue
        cur.append(v)
        n += c
        if n >= min_group:
            pools.append(cur)
            cur, n = [], 0
    if cur:
        if pools:
            pools[-1] += cur
        else:
            pools.append(cur)
    return pools


def _group_rms(groups, shape, keep, tensors, min_group):
    """yields (name of the group, [rms of each tensor over it]); tensors: differences (or values) of the output's shape"""
    squares = [t.double() ** 2 for t in tensors]
    for name, label in groups.items():
        cnt, sums = group_sums(label, shape, keep, squares)
        for i, pool in enumerate(pooled(cnt, min_group)):
            n = float(cnt[pool].sum())
            yield f'{name}[{i}]', [float(s[pool].sum() / n) ** 0.5 for s in sums]


def grouped_rms(got, yard, ref, groups, keep=None, min_group=MIN_GROUP):
    """(worst, checked, where): the largest rms(got - ref) / (RMS_FACTOR rms(yard - ref) + RMS_FLOOR rms(ref)) over the groups of
    `groups` ({name: integer labels broadcastable to the output}), the number of groups looked at, and the name of the worst.  Elements
    outside `keep` are left out of all three.  The comparison runs where ref is."""
    dev = ref.device
    worst, checked, where = 0.0, 0, ''
    for name, (eg, ey, er) in _group_rms(groups, ref.shape, keep, (got.to(dev).double() - ref, yard.to(dev).double() - ref, ref), min_group):
        limit = RMS_FACTOR * ey + RMS_FLOOR * er
        ratio = eg / limit if limit > 0 else (0.0 if eg == 0 else float('inf'))
        checked += 1
        if ratio > worst:
            worst, where = ratio, name
    return worst, checked, where


def live_rms(got, ref, groups, bar=LIVE_BAR, min_group=MIN_GROUP):
    """(worst, checked, where): the largest rms(got - ref) / (bar rms(ref)) over the whole output and over the groups (a group whose
    reference is all zeros against the whole output's rms: the transformed kinds leave rounding noise where a tap reads only padding)"""
    err = got.to(ref.device).double() - ref
    assert _rms(ref) > 0
    worst, checked, where = _rms(err) / (bar * _rms(ref)), 1, 'all'
    whole = _rms(ref)
    for name, (eg, er) in _group_rms(groups, ref.shape, None, (err, ref), min_group):
        checked += 1
        scale = er if er > 0 else whole           # (a group whose reference is all zeros - a tap that only reads padding - is measured against the output's rms)
        if eg / (bar * scale) > worst:
            worst, where = eg / (bar * scale), name
    return worst, checked, where


def whole_tensor_figures(got, yard, ref):
    """the two figures of the family's older tests: (max |err| / max |ref|, l2(got), 2.5 l2(yard) + 1e-7)"""
    l2 = lambda t: float((t.double() - ref).norm() / ref.norm())
    return float((got.double() - ref).abs().max() / ref.abs().max()), l2(got), 2.5 * l2(yard) + 1e-7

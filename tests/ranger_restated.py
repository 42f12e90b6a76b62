"""Ranger (the reference's pSp/training/ranger.py:79-165) restated on plain tensors, in any float dtype, and the deterministic
inputs the Ranger tests share.  A helper, not a test: tests/test_ranger_cpu.py, tests/test_gpu_ranger.py and
tools/ranger_golden.py import it.

Every tensor of the shape list has a fixed id (its index in SHAPES).  The id, not the position in whatever list a test builds,
seeds the tensor's data and decides its param group, so a tensor goes through the same trajectory alone, in the small list of
the golden fixture and in the full list.
"""
import math

import torch

# the smallest shapes at which the kernel can go wrong (what each covers: the comments)
SHAPES = [
    (3,),            # 0: 1-D, no centralisation
    (1,),            # 1: 1-D, a single element
    (20000,),        # 2: 1-D, more than two chunks
    (5, 1),          # 3: rows of one element: the centralised gradient is exactly 0
    (16, 14),        # 4: L = 14
    (1171, 14),      # 5: many rows per block, the last block partial
    (7, 3, 3, 3),    # 6: L = 27, not a multiple of 4
    (4, 6, 1, 1),    # 7: the SE fc form
    (3, 512, 3, 3),  # 8: L = 4608, one row per block
    (2, 20003),      # 9: rows longer than two tiles, odd length
]
SMALL_IDS = [0, 1, 3, 4, 6, 7]          # what tests/golden/ranger_ref.npz holds (the fixture stays far below 1 MB)
STEPS = 13                              # steps 1-5 unrectified, 6-13 rectified (beta2 = 0.999); lookahead at 6 and 12 (k = 6)
RECORD = (7, 13)
STATE_KEYS = ('exp_avg', 'exp_avg_sq', 'slow_buffer')

_DEFAULTS = dict(alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0, use_gc=True, gc_conv_only=False)
CONFIGS = {
    # lr = 2**-5: the 13-step displacement stands well clear of the rounding of p
    'a': dict(_DEFAULTS, lrs=(2.0 ** -5,)),
    'b': dict(_DEFAULTS, betas=(0.9, 0.99), k=5, alpha=0.8, weight_decay=0.01, gc_conv_only=True, lrs=(2.0 ** -5, 2.0 ** -7)),
}

_M32 = 0xFFFFFFFF


def _hash24(numel, a, b):
    """24 well-mixed bits per element index, from integer torch ops only (the same on every machine)"""
    x = torch.arange(numel, dtype=torch.int64)
    x = (x * 0x9E3779B1 + a * 0x85EBCA77 + b * 0xC2B2AE3D + 0x27D4EB2F) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x2C1B3C6D) & _M32
    x = x ^ (x >> 12)
    x = (x * 0x297A2D39) & _M32
    x = x ^ (x >> 15)
    return x & 0xFFFFFF


def grad(tid, step):
    """the fp32 gradient of tensor `tid` at `step`: multiples of 2^-23 in [-0.6875, 1.3125), mean 0.3125 (so the row means that
    centralisation removes are of the size of the gradient itself); exact in fp32, hence bit-identical everywhere"""
    shape = SHAPES[tid]
    k = _hash24(math.prod(shape), step, tid) - 2 ** 23 + 5 * 2 ** 19
    return (k.to(torch.float32) * 2.0 ** -23).reshape(shape)


def param0(tid):
    """the fp32 initial value of tensor `tid`: multiples of 2^-24 in [-0.5, 0.5)"""
    shape = SHAPES[tid]
    k = _hash24(math.prod(shape), 1000003, tid) - 2 ** 23
    return (k.to(torch.float32) * 2.0 ** -24).reshape(shape)


def group_of(tid, cfg):
    return tid % len(CONFIGS[cfg]['lrs'])


def ctor_kwargs(cfg):
    return {k: v for k, v in CONFIGS[cfg].items() if k != 'lrs'}


def make_optimizer(cls, params, ids, cfg):
    """an optimiser of class `cls` (ours or the reference's) over `params` (tensor ids `ids`) in configuration `cfg`"""
    lrs = CONFIGS[cfg]['lrs']
    groups = [dict(params=[p for p, t in zip(params, ids) if group_of(t, cfg) == g], lr=lr) for g, lr in enumerate(lrs)]
    return cls(groups, **ctor_kwargs(cfg))


def schedule(step, beta1, beta2, threshold):
    """(N_sma, step_size, rectified) at `step`, restated from ranger.py:134-143"""
    b2t = beta2 ** step
    n_max = 2.0 / (1.0 - beta2) - 1.0
    n_sma = n_max - 2.0 * step * b2t / (1.0 - b2t)
    bias1 = 1.0 - beta1 ** step
    if n_sma > threshold:
        r = (1.0 - b2t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max / (n_max - 2.0)
        return n_sma, math.sqrt(r) / bias1, True
    return n_sma, 1.0 / bias1, False


def centralised(tid, cfg):
    c = CONFIGS[cfg]
    return c['use_gc'] and len(SHAPES[tid]) > (3 if c['gc_conv_only'] else 1)


def run(ids, cfg, dtype=torch.float64, steps=STEPS, record=RECORD, start=None):
    """Steps the tensors `ids` in configuration `cfg` with every quantity held in `dtype`; the gradients are the fp32 ones of grad().
    start: None (from param0, fresh state) or (step, {tid: {'p', 'exp_avg', 'exp_avg_sq', 'slow_buffer'}}) to continue from.
    Returns {step: {tid: {'p', 'exp_avg', 'exp_avg_sq', 'slow_buffer'}}} for the steps in `record`."""
    c = CONFIGS[cfg]
    beta1, beta2 = c['betas']
    first = 1
    if start is None:
        st = {}
        for t in ids:
            p = param0(t).to(dtype)
            st[t] = dict(p=p, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p), slow_buffer=p.clone())
    else:
        first = start[0] + 1
        st = {t: {k: v.to(dtype).clone() for k, v in start[1][t].items()} for t in ids}
    out = {}
    for step in range(first, steps + 1):
        _, step_size, rectified = schedule(step, beta1, beta2, c['N_sma_threshhold'])
        for t in ids:
            s = st[t]
            lr = c['lrs'][group_of(t, cfg)]
            g = grad(t, step).to(dtype)
            if centralised(t, cfg):
                rows = g.reshape(g.shape[0], -1)
                g = (rows - rows.mean(dim=1, keepdim=True)).reshape(g.shape)
            s['exp_avg_sq'] = s['exp_avg_sq'] * beta2 + (1 - beta2) * g * g
            s['exp_avg'] = s['exp_avg'] * beta1 + (1 - beta1) * g
            p = s['p']
            if c['weight_decay'] != 0:
                p = p + (-c['weight_decay'] * lr) * p
            if rectified:
                p = p + (-step_size * lr) * (s['exp_avg'] / (s['exp_avg_sq'].sqrt() + c['eps']))
            else:
                p = p + (-step_size * lr) * s['exp_avg']
            if step % c['k'] == 0:
                s['slow_buffer'] = s['slow_buffer'] + c['alpha'] * (p - s['slow_buffer'])
                p = s['slow_buffer'].clone()
            s['p'] = p
        if step in record:
            out[step] = {t: {k: v.clone() for k, v in st[t].items()} for t in ids}
    return out

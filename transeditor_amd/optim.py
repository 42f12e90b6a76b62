"""Multi-tensor Adam, Ranger and EMA on the MI355X kernels (te_mt_adam_f32 / te_mt_ranger_f32 / te_mt_ema_f32): one launch per
optimiser step.

Reference: train_spatial_query.py:458-473 (``optim.Adam(generator.parameters(), lr=lr * ratio, betas=(0 ** ratio,
0.99 ** ratio))`` for G and D) and ``accumulate`` (:56-61).  ``FusedAdam`` is a ``torch.optim.Optimizer`` with exactly
``torch.optim.Adam``'s state layout (``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter), so ``state_dict()`` /
``load_state_dict()`` interchange with the reference's ``g_optim`` / ``d_optim`` checkpoints (:311-317).

How a step works: the (static) parameter / state pointers and the (per-step) gradient pointers go into one int64 table
that is uploaded through a double-buffered pinned host buffer with an asynchronous copy (no host-device synchronisation:
the host keeps running ahead of the GPU), then ONE kernel walks every tensor in fixed-size chunks.  Gradients may live
anywhere (fresh autograd tensors, or slices of the GradSync buckets after the all-reduce).

``Ranger`` is the encoder's optimiser (pSp/training/ranger.py, chosen by pSp/training/coach_new.py:225-233: RAdam + Lookahead +
gradient centralisation) on the same mechanics; its work map is made of groups of whole gradient rows instead of flat chunks,
because centralisation needs each row's mean.
"""
import math

import torch

from . import _lib

CHUNK = 8192          # elements per block (256 threads x 8 x 16 bytes)
TILE = 8184           # Ranger: elements of gradient a block stages in LDS (32 KiB less the kernel's 32 bytes of bookkeeping)


class _Table:
    """Device-resident int64 pointer table [rows, n] + the static int32 chunk map [2, n_chunks] for a tensor list."""

    def __init__(self, numels, rows, device):
        self.n, self.rows, self.device = len(numels), rows, device
        self.chunks = self._work_map(numels).to(device)
        self.n_chunks = self.chunks.shape[1]
        self.dev = torch.zeros(rows, self.n, dtype=torch.int64, device=device)
        self._host = [torch.zeros(rows, self.n, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._evt = [None, None]
        self._turn = 0
        self._last = None

    @staticmethod
    def _work_map(numels):
        t_idx, c_idx = [], []
        for t, ne in enumerate(numels):
            nc = max(1, -(-ne // CHUNK))
            t_idx += [t] * nc
            c_idx += list(range(nc))
        return torch.tensor([t_idx, c_idx], dtype=torch.int32)

    def upload(self, rows):
        """rows: list of `self.rows` python-int lists.  Skips the copy when nothing changed."""
        if rows == self._last:
            return
        i = self._turn
        self._turn ^= 1
        if self._evt[i] is not None:
            self._evt[i].synchronize()               # the copy that last read this pinned buffer (two uploads ago) is done
        self._host[i].copy_(torch.tensor(rows, dtype=torch.int64))
        self.dev.copy_(self._host[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._evt[i] = ev
        self._last = rows


def row_groups(numels, row_lens, tile=TILE):
    """The static work map of te_mt_ranger_f32 for tensors of `numels` elements whose gradient rows are `row_lens` long (0: no
    centralisation, the tensor is cut into "rows" of `tile` elements): an int32 tensor [3, n_work] = tensor index, first row, row
    count.  An entry holds whole rows, at most `tile` elements of them and at least one row; every row is in exactly one entry."""
    parts = []
    for t, (ne, L) in enumerate(zip(numels, row_lens)):
        if ne == 0:
            continue
        if L == 0:
            n_rows, per = -(-ne // tile), 1
        else:
            if ne % L:
                raise ValueError(f'tensor {t}: {ne} elements are not whole rows of {L}')
            n_rows, per = ne // L, max(1, tile // L)
        first = torch.arange(0, n_rows, per, dtype=torch.int64)
        parts.append(torch.stack([torch.full_like(first, t), first, torch.clamp(n_rows - first, max=per)]))
    if not parts:
        return torch.zeros(3, 0, dtype=torch.int32)
    out = torch.cat(parts, 1)
    if int(out.max()) >= 2 ** 31:
        raise ValueError('a tensor has 2^31 rows or more')
    return out.to(torch.int32)


class _RowTable(_Table):
    """_Table with the row-group work map of te_mt_ranger_f32 in place of the chunk map"""

    def __init__(self, numels, row_lens, rows, device):
        self.row_lens = list(row_lens)
        super().__init__(numels, rows, device)

    def _work_map(self, numels):
        return row_groups(numels, self.row_lens)


def _check_param(p, who='FusedAdam / EMA'):
    if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
        raise RuntimeError(f'te_hip: {who} need{"" if "/" in who else "s"} contiguous fp32 parameters on the GPU, got {p.dtype} '
                           f'{p.device} (no CPU path exists)')


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (no weight decay, no amsgrad, not maximize) as one kernel launch per parameter group."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, **other):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError(f'invalid Adam hyper-parameters lr={lr} betas={betas} eps={eps}')
        if weight_decay or amsgrad or maximize:
            raise NotImplementedError('FusedAdam covers the reference\'s configuration: no weight decay / amsgrad / maximize')
        # param_groups carry every key torch.optim.Adam's do, so a state_dict written by either loads into the other
        defaults = dict(torch.optim.Adam([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False)
        super().__init__(params, defaults)
        self._tables = {}

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st['step'] = torch.tensor(0.0, dtype=torch.float32)          # torch.optim.Adam's layout (host scalar tensor)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        else:
            self._host_step(st)
        return st

    @staticmethod
    def _host_step(st):
        """`step` as a host fp32 scalar tensor.  The reference's torch 1.7 Adam (environment.yaml:130) stores a python int, and
        `torch.load(map_location=device)` moves a tensor `step` to the GPU, where `.item()` would synchronise once per parameter
        and step: both are normalised here (once, at load time or at the first step after it)."""
        s = st.get('step')
        if s is not None and not (torch.is_tensor(s) and s.device.type == 'cpu' and s.dtype == torch.float32 and s.ndim == 0):
            st['step'] = torch.tensor(float(s), dtype=torch.float32)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            self._host_step(st)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            params = group['params']
            if not params:
                continue
            active = [p for p in params if p.grad is not None]
            if not active:
                continue
            for p in active:
                _check_param(p)
                g = p.grad
                if g.is_sparse or g.dtype != torch.float32 or g.device != p.device:
                    raise RuntimeError('te_hip: FusedAdam needs dense fp32 gradients on the parameter\'s device')
                if not g.is_contiguous():
                    p.grad = g = g.contiguous()
                self._init_state(p)
            key = (gi, tuple(p.numel() for p in params))
            tab = self._tables.get(key)
            if tab is None or tab.device != params[0].device:
                tab = self._tables[key] = _Table([p.numel() for p in params], 5, params[0].device)
            beta1, beta2 = group['betas']
            # parameters of a group normally share one step count; if not (a parameter that skipped steps), one launch per count
            steps = {}
            for p in active:
                st = self.state[p]
                st['step'] += 1
                steps.setdefault(int(st['step'].item()), set()).add(p)
            for step, members in steps.items():
                rows = [[], [], [], [], []]
                for p in params:
                    on = p in members
                    st = self.state.get(p) if on else None
                    rows[0].append(p.data_ptr())
                    rows[1].append(p.grad.data_ptr() if on else 0)
                    rows[2].append(st['exp_avg'].data_ptr() if on else 0)
                    rows[3].append(st['exp_avg_sq'].data_ptr() if on else 0)
                    rows[4].append(p.numel())
                tab.upload(rows)
                _lib.mt_adam(tab.dev, tab.chunks, tab.n, tab.n_chunks, CHUNK, float(group['lr']), float(beta1), float(beta2),
                             float(group['eps']), step)
            # the kernel wrote the parameters through raw pointers: tell autograd / the frozen-weight caches (op/modconv.py)
            torch.autograd.graph.increment_version(active)
        return loss


def radam_schedule(step, beta1, beta2, n_sma_threshold=5):
    """(N_sma, step_size, rectified) of RAdam at `step` (1-based), as ranger.py:134-143 computes them, in python floats (double).
    rectified: the variance is tractable (N_sma > threshold) and the step divides by sqrt(v) + eps; otherwise it is a plain
    momentum step."""
    beta2_t = beta2 ** step
    n_sma_max = 2 / (1 - beta2) - 1
    n_sma = n_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma > n_sma_threshold:
        step_size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma * n_sma_max
                              / (n_sma_max - 2)) / (1 - beta1 ** step)
        return n_sma, step_size, True
    return n_sma, 1.0 / (1 - beta1 ** step), False


def gc_row_len(shape, use_gc=True, gc_conv_only=False):
    """length of the rows whose mean ranger.py:118-119 subtracts from a gradient of `shape` (the mean is over every dim but the
    first), or 0 where it does not centralise: gradients of dim() <= 1, or <= 3 under gc_conv_only, or use_gc off"""
    if not use_gc or len(shape) <= (3 if gc_conv_only else 1) or shape[0] == 0:
        return 0
    n = 1
    for d in shape[1:]:
        n *= d
    return n


class Ranger(torch.optim.Optimizer):
    """The reference's Ranger (pSp/training/ranger.py: RAdam + Lookahead + gradient centralisation; same constructor, defaults,
    ValueErrors, param-group keys and state layout) as one kernel launch per parameter group and step.

    State per parameter, exactly the reference's: ``step`` (python int), ``exp_avg``, ``exp_avg_sq``, ``slow_buffer`` (a copy of
    the parameter made at its first step); a ``state_dict()`` written by either class loads into the other.  Parameters without
    a gradient are skipped and get no state.  Like the reference, the lookahead rate and the N_sma threshold are the
    constructor's (``self.alpha``, ``self.N_sma_threshhold``), the lookahead period is the group's ``k``.

    Not reproduced from the reference:
    * its ``radam_buffer`` caches (N_sma, step_size) under ``step % 10`` alone, so a second param group with other betas gets the
      first group's schedule.  Here ``radam_schedule`` is evaluated per group from that group's own betas.
    * it centralises ``p.grad`` in place (for fp32 its ``.float()`` is no copy).  Here ``p.grad`` is left as it was.
    * sparse gradients and parameters that are not fp32 on the GPU are refused (its ``.float()`` round trip is the identity for
      fp32)."""

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0,
                 use_gc=True, gc_conv_only=False):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f'Invalid slow update rate: {alpha}')
        if not 1 <= k:
            raise ValueError(f'Invalid lookahead steps: {k}')
        if not lr > 0:
            raise ValueError(f'Invalid Learning Rate: {lr}')
        if not eps > 0:
            raise ValueError(f'Invalid eps: {eps}')
        defaults = dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps,
                        weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.N_sma_threshhold = N_sma_threshhold
        self.alpha = alpha
        self.k = k
        self.use_gc = use_gc
        self.gc_gradient_threshold = 3 if gc_conv_only else 1
        self._tables = {}

    def _row_len(self, p):
        return gc_row_len(tuple(p.shape), self.use_gc, self.gc_gradient_threshold == 3)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            params = group['params']
            active = [p for p in params if p.grad is not None]
            if not active:
                continue
            for p in active:
                _check_param(p, 'Ranger')
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError('te_hip: Ranger does not support sparse gradients')
                if g.dtype != torch.float32 or g.device != p.device:
                    raise RuntimeError('te_hip: Ranger needs dense fp32 gradients on the parameter\'s device')
                if not g.is_contiguous():
                    p.grad = g = g.contiguous()
                st = self.state[p]
                if len(st) == 0:
                    st['step'] = 0
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st['slow_buffer'] = p.detach().clone(memory_format=torch.contiguous_format)
                else:
                    for key in ('exp_avg', 'exp_avg_sq', 'slow_buffer'):
                        _check_param(st[key], f'Ranger (state {key})')
                    st['step'] = int(st['step'])
            row_lens = [self._row_len(p) for p in params]
            key = (gi, tuple(tuple(p.shape) for p in params), tuple(row_lens))
            tab = self._tables.get(key)
            if tab is None or tab.device != active[0].device:
                tab = self._tables[key] = _RowTable([p.numel() for p in params], row_lens, 7, active[0].device)
            if tab.n_chunks == 0:
                continue
            beta1, beta2 = group['betas']
            # parameters of a group normally share one step count; if not (a parameter that skipped steps), one launch per count
            steps = {}
            for p in active:
                st = self.state[p]
                st['step'] += 1
                steps.setdefault(st['step'], set()).add(p)
            numels = [p.numel() for p in params]
            for step, members in steps.items():
                rows = [[], [], [], [], [], numels, row_lens]
                for p in params:
                    on = p in members
                    st = self.state.get(p) if on else None
                    rows[0].append(p.data_ptr())
                    rows[1].append(p.grad.data_ptr() if on else 0)
                    rows[2].append(st['exp_avg'].data_ptr() if on else 0)
                    rows[3].append(st['exp_avg_sq'].data_ptr() if on else 0)
                    rows[4].append(st['slow_buffer'].data_ptr() if on else 0)
                tab.upload(rows)
                _, step_size, rectified = radam_schedule(step, beta1, beta2, self.N_sma_threshhold)
                _lib.mt_ranger(tab.dev, tab.chunks, tab.n, tab.n_chunks, TILE, step_size * group['lr'],
                               group['weight_decay'] * group['lr'], beta1, beta2, group['eps'], self.alpha, rectified,
                               step % group['k'] == 0)
            # the kernel wrote the parameters through raw pointers: tell autograd / the frozen-weight caches (op/modconv.py)
            torch.autograd.graph.increment_version(active)
        return loss


def encoder_optimizer(params, optim_name='ranger', lr=1e-4):
    """The reference's configure_optimizers (pSp/training/coach_new.py:225-233): Adam when optim_name is 'adam', Ranger for
    anything else, both at lr and otherwise at their defaults."""
    if optim_name == 'adam':
        return FusedAdam(params, lr=lr)
    return Ranger(params, lr=lr)


class MultiTensorEMA:
    """dst <- decay * dst + (1 - decay) * src over all parameters, one launch (reference accumulate(), :56-61)."""

    def __init__(self, dst_module, src_module):
        d, s = dict(dst_module.named_parameters()), dict(src_module.named_parameters())
        self.pairs = [(d[k], s[k]) for k in d.keys()]                    # KeyError on a structure mismatch, like the reference
        self._table = None

    @torch.no_grad()
    def update(self, decay):
        if not self.pairs:
            return
        for a, b in self.pairs:
            _check_param(a)
            _check_param(b)
            if a.shape != b.shape:
                raise RuntimeError(f'EMA: parameter shapes differ {tuple(a.shape)} vs {tuple(b.shape)}')
        dev = self.pairs[0][0].device
        if self._table is None or self._table.device != dev:
            self._table = _Table([a.numel() for a, _ in self.pairs], 3, dev)
        t = self._table
        t.upload([[a.data_ptr() for a, _ in self.pairs], [b.data_ptr() for _, b in self.pairs],
                  [a.numel() for a, _ in self.pairs]])
        _lib.mt_ema(t.dev, t.chunks, t.n, t.n_chunks, CHUNK, decay)
        torch.autograd.graph.increment_version([a for a, _ in self.pairs])      # written through raw pointers

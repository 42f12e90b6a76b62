"""The contract of op/recorded.py::recorded_backward - the one place where a fused node's backward that is itself recorded
(create_graph) is written - on toy Functions: pure torch, fp64, no kernel library.  The toy nodes differentiate the very expression
the plain route evaluates, so the comparisons are `torch.equal`, not a tolerance (one exception, reasoned where it stands: sums of
three and more terms that the two graphs add in different orders).  Plus the predicate the backward functions ask
about `no_weight_grads()`, from the calling thread and from another one (the autograd engine's)."""
import threading

import torch
from torch.autograd import Function

from transeditor_amd.op import recorded
from transeditor_amd.op.recorded import recorded_backward

F64 = torch.float64


def _expr(x, w, s, b):
    y = torch.sin(x * w) * s
    return y if b is None else y + b * x.square()


class _Toy(Function):
    """y = sin(x w) s [+ b x^2]; `mask`: need flags switched off on top of needs_input_grad (what a site does under no_weight_grads())"""
    @staticmethod
    def forward(ctx, x, w, s, b, mask):
        ctx.save_for_backward(x, w, s, b)
        ctx.mask = mask
        return _expr(x, w, s, b)

    @staticmethod
    def backward(ctx, g):
        assert torch.is_grad_enabled(), 'only the recorded branch is under test'
        need = [n and m for n, m in zip(ctx.needs_input_grad[:4], ctx.mask)]
        return tuple(recorded_backward(_expr, ctx.saved_tensors, need, g)) + (None,)


def _leaves(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(5, dtype=F64, generator=g).requires_grad_(True) for _ in range(4)]


def _three_orders(f, ins):
    """value, then three successive recorded gradients of the previous level (fixed cotangents) w.r.t. every input"""
    out, level = [], f(*ins)
    for k in range(3):
        out.append(level)
        cot = torch.randn(level.shape, dtype=F64, generator=torch.Generator().manual_seed(10 + k))
        gs = torch.autograd.grad(level, ins, cot, create_graph=True, allow_unused=True)
        level = torch.stack([g for g in gs if g is not None])
    return out + [level]


def test_single_output_none_input_through_third_derivative():
    x, w, s, _ = _leaves()
    want = _three_orders(lambda x, w, s: _expr(x, w, s, None), (x, w, s))
    got = _three_orders(lambda x, w, s: _Toy.apply(x, w, s, None, (True,) * 4), (x, w, s))
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), k


def test_need_mask_and_none_input_slots():
    x, w, s, b = _leaves(1)
    g = torch.ones(5, dtype=F64)
    full = recorded_backward(_expr, (x, w, s, b), (True,) * 4, g)
    want = torch.autograd.grad(_expr(x, w, s, b), (x, w, s, b), g)
    assert all(torch.equal(a, c) for a, c in zip(full, want))
    part = recorded_backward(_expr, (x, w, s, None), (True, False, True, True), g)
    assert part[1] is None and part[3] is None            # not needed; the input is None
    want = torch.autograd.grad(_expr(x, w, s, None), (x, s), g)
    assert torch.equal(part[0], want[0]) and torch.equal(part[2], want[1])
    assert part[0].requires_grad                          # recorded: differentiable again


def test_dependent_inputs_give_partial_derivatives():
    """s is a function of x in the OUTER graph (the demodulation coefficient of a style scale): the helper returns d/dx with s held
    fixed, the outer graph supplies ds/dx, and the total equals the plain expression's.  First order: x receives two terms, whose sum
    does not depend on the order the engine adds them in, so `torch.equal`.  From the second order on x receives three and more
    terms and the two graphs add them in different orders: equal to fp64 round-off, a few ulp (2.2e-16) of terms of size <= 10."""
    x, w, _, b = _leaves(2)
    dep = lambda x: torch.cos(x) * 0.5 + 1.5
    g = torch.ones(5, dtype=F64)
    gx, _, gs, _ = recorded_backward(_expr, (x, w, dep(x), b), (True, False, True, False), g)
    s_fixed = dep(x).detach().requires_grad_(True)
    want = torch.autograd.grad(_expr(x, w, s_fixed, b), (x, s_fixed), g)
    assert torch.equal(gx, want[0]) and torch.equal(gs, want[1])
    want = _three_orders(lambda x, w, b: _expr(x, w, dep(x), b), (x, w, b))
    got = _three_orders(lambda x, w, b: _Toy.apply(x, w, dep(x), b, (True,) * 4), (x, w, b))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for k in (2, 3):
        assert torch.allclose(got[k], want[k], rtol=0, atol=1e-13), k


def _pair(x, w, u):
    return torch.sin(x * w), torch.exp(u) * x


class _ToyPair(Function):
    @staticmethod
    def forward(ctx, x, w, u):
        ctx.save_for_backward(x, w, u)
        ctx.set_materialize_grads(False)
        return _pair(x, w, u)

    @staticmethod
    def backward(ctx, ga, gb):
        _ToyPair.seen = (ga is None, gb is None)
        return tuple(recorded_backward(_pair, ctx.saved_tensors, ctx.needs_input_grad, (ga, gb)))


def test_two_outputs_one_cotangent_none_and_unused_input():
    x, w, u, _ = _leaves(3)
    a, _ = _ToyPair.apply(x, w, u)
    cot = torch.linspace(-1, 2, 5, dtype=F64)
    got = torch.autograd.grad(a, (x, w, u), cot, create_graph=True, allow_unused=True)
    assert _ToyPair.seen == (False, True)
    want = torch.autograd.grad(_pair(x, w, u)[0], (x, w, u), cot, create_graph=True, allow_unused=True)
    assert got[2] is None and want[2] is None             # u feeds the dropped output only: unused
    for k in (0, 1):
        assert torch.equal(got[k], want[k])
        assert torch.equal(torch.autograd.grad(got[k].sum(), x, retain_graph=True)[0],
                           torch.autograd.grad(want[k].sum(), x, retain_graph=True)[0])
    # the helper itself: the output without a cotangent takes no part, whichever it is
    g = torch.ones(5, dtype=F64)
    ra = recorded_backward(_pair, (x, w, u), (True,) * 3, (g, None))
    rb = recorded_backward(_pair, (x, w, u), (True,) * 3, (None, g))
    assert ra[2] is None and rb[1] is None
    assert torch.equal(rb[0], torch.exp(u)) and torch.equal(rb[2], torch.exp(u) * x)
    both = recorded_backward(_pair, (x, w, u), (True,) * 3, (g, g))
    assert torch.equal(both[0], torch.autograd.grad(_pair(x, w, u), x, (g, g))[0])


def test_nothing_to_differentiate_returns_nones():
    """every needed input masked away (a weight-only request under no_weight_grads()), or no cotangent at all: all None, no
    exception (torch.autograd.grad raises on an empty input list), and the function is not even built"""
    x, w, s, b = _leaves(4)
    g = torch.ones(5, dtype=F64)

    def build(*a):
        raise AssertionError('built although nothing is to be differentiated')
    assert recorded_backward(build, (x, w, s, b), (False,) * 4, g) == [None] * 4
    assert recorded_backward(build, (None, None), (True, True), g) == [None] * 2
    assert recorded_backward(build, (x, w, s, b), (True,) * 4, None) == [None] * 4
    assert recorded_backward(build, (x, w), (True, True), (None, None)) == [None] * 2
    # end to end: only w requires a gradient and the site masks it
    y = _Toy.apply(x.detach(), w, s.detach(), None, (True, False, True, True))
    assert torch.autograd.grad(y.sum(), w, create_graph=True, allow_unused=True) == (None,)


def test_weights_skipped_predicate_across_threads():
    def elsewhere(*tokens):
        seen = []
        t = threading.Thread(target=lambda: seen.append([recorded.weights_skipped(*a) for a in [()] + [(k,) for k in tokens]]))
        t.start()
        t.join()
        return seen[0]
    with recorded.second_order() as tok:
        assert not recorded.weights_skipped() and not recorded.weights_skipped(tok)
    other = recorded._Graph()                              # the token of some other thread's forward
    assert elsewhere(tok, other) == [False, False, False]
    with recorded.no_weight_grads():                       # flips the token of the forward that just ended and the default one
        assert recorded.weights_skipped() and recorded.weights_skipped(tok)
        assert tok.skip_w and not other.skip_w
        assert elsewhere(tok, other) == [True, True, True]        # (a set default token covers every node)
    assert not recorded.weights_skipped() and not recorded.weights_skipped(tok)
    assert elsewhere(tok, other) == [False, False, False]
    # a context opened on another thread is seen here: the flag lives on the tokens, not in thread-local state
    inside, done = threading.Event(), threading.Event()

    def hold():
        with recorded.no_weight_grads():
            inside.set()
            done.wait(10)
    t = threading.Thread(target=hold)
    t.start()
    assert inside.wait(10)
    try:
        assert recorded.weights_skipped() and recorded.weights_skipped(recorded._STATE.graph)
    finally:
        done.set()
        t.join()
    assert not recorded.weights_skipped()

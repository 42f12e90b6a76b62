"""What the fused autograd nodes share when a backward is differentiated again (R1, path length): the hints of those steps and
the protocol of a recorded backward.  A leaf module: it imports nothing from the package, so every op module may import it.

Both hints are optional: ``second_order()`` around the forward makes the ops build their any-order differentiable form right away,
``no_weight_grads()`` around the recorded ``autograd.grad`` skips the first-order weight gradients.  Without them a fused node
finds out in its backward that it is being recorded (``torch.is_grad_enabled()``) and goes through ``recorded_backward``.

Threading: forward passes may run concurrently from several Python threads (the reference's metrics wrap the generator in
nn.DataParallel; te_hip.h promises thread-safe entry points), so `second_order` is THREAD-LOCAL (`_STATE`).  `skip_w` cannot be:
it is read inside backward functions, which the autograd engine runs on its own per-device thread.  It therefore lives on a small token object (`_Graph`) that every
`second_order()` context creates and every node built inside it keeps (`ctx.graph`); `no_weight_grads()` flips the flag on the
calling thread's most recent token (and on the process-wide default token that nodes built outside any `second_order()` context
share).  Backward functions ask `weights_skipped()`.
"""
import contextlib
import threading

import torch


class _Graph:
    __slots__ = ('skip_w',)

    def __init__(self):
        self.skip_w = False


_DEFAULT_GRAPH = _Graph()


class _Local(threading.local):
    """per-thread state; every thread starts from the defaults"""

    def __init__(self):
        self.second_order = False
        self.second_wrt = None               # second_order(wrt=...): where the recorded backward will stop
        self.graph = _DEFAULT_GRAPH          # token of the current / most recent second_order() context of this thread


_STATE = _Local()


def current_graph():
    """token the nodes created right now belong to (see the threading note above)"""
    return _STATE.graph if _STATE.second_order else _DEFAULT_GRAPH


def weights_skipped(graph=_DEFAULT_GRAPH):
    """Asked inside a backward function, on whatever thread it runs: is `no_weight_grads()` in force for a node that kept the token
    `graph` (`ctx.graph`), or for one built outside any `second_order()` context (no argument: the default token)?"""
    return graph.skip_w or _DEFAULT_GRAPH.skip_w


@contextlib.contextmanager
def second_order(wrt=None):
    """Forward passes inside this context are built from the any-order differentiable pieces right away (the caller knows
    a create_graph backward follows), which saves the forward recomputation inside the recorded backward.
    `wrt='latent'`: the recorded backward will stop at the generator's W+ latent (path-length regulariser,
    train_spatial_query.py:92-105 with `return_latents=True`), so everything that PRODUCES the latent - mapping networks,
    attention blocks, adjust_style - is differentiated once only and keeps its fused first-order nodes
    (Generator.forward suspends the hint for that section)."""
    old = (_STATE.second_order, _STATE.graph, _STATE.second_wrt)
    _STATE.second_order, _STATE.graph, _STATE.second_wrt = True, _Graph(), wrt
    try:
        yield _STATE.graph
    finally:
        _STATE.second_order = old[0]         # (the token stays current for the no_weight_grads() that follows the forward)
        _STATE.second_wrt = old[2]
        if old[0]:
            _STATE.graph = old[1]


@contextlib.contextmanager
def latent_producer_section():
    """Generator.forward wraps the part that produces the latent in this: under second_order(wrt='latent') the hint is off
    inside (see there); otherwise nothing changes."""
    if not (_STATE.second_order and _STATE.second_wrt == 'latent'):
        yield
        return
    _STATE.second_order = False
    try:
        yield
    finally:
        _STATE.second_order = True


@contextlib.contextmanager
def no_weight_grads():
    """Around `autograd.grad(..., inputs=<activations / latents>, create_graph=True)`: the first-order weight gradients
    of the convolutions are not among the requested inputs, so their correlation passes are skipped (autograd cannot tell
    a Python Function which of its outputs are consumed).  Do NOT use around a backward that accumulates into weights.
    Applies to the graph built by this thread's most recent `second_order()` forward and to nodes built outside any such
    context (those share one process-wide token: hint-less double backward is not meant to run concurrently)."""
    toks = {id(t): t for t in (_STATE.graph, _DEFAULT_GRAPH)}.values()
    old = [(t, t.skip_w) for t in toks]
    for t in toks:
        t.skip_w = True
    try:
        yield
    finally:
        for t, o in old:
            t.skip_w = o


def recorded_backward(build, inputs, need, grad_outputs):
    """The backward of a fused node that is itself being recorded (create_graph): -> list, one entry per input.

    `build(*aliases)` is the node's function from any-order differentiable pieces, one tensor or a sequence of them; `inputs` are
    the node's saved inputs (None allowed), `need` one flag per input, `grad_outputs` one cotangent or a sequence (an output whose
    cotangent is None takes no part).  The inputs may depend on each other in the OUTER graph (a demodulation coefficient is a
    function of the style scale): the function is differentiated w.r.t. fresh aliases, so each returned gradient is the PARTIAL
    derivative, while everything stays connected to the original tensors for the next differentiation.  A slot is None where the
    input is None, not needed or unused; with nothing to differentiate (no input picked, no cotangent) nothing is built."""
    grads = [None] * len(inputs)
    picked = [i for i, (t, n) in enumerate(zip(inputs, need)) if n and t is not None]
    single = grad_outputs is None or isinstance(grad_outputs, torch.Tensor)
    gouts = [grad_outputs] if single else list(grad_outputs)
    if not picked or all(g is None for g in gouts):
        return grads
    with torch.enable_grad():
        al = [None if t is None else t.view_as(t) for t in inputs]
        outs = build(*al)
        outs = [outs] if single else list(outs)
        kept = [(o, g) for o, g in zip(outs, gouts) if g is not None]
        res = torch.autograd.grad([o for o, _ in kept], [al[i] for i in picked], [g for _, g in kept],
                                  create_graph=True, allow_unused=True)
    for i, g in zip(picked, res):
        grads[i] = g
    return grads

"""The two weight caches of the convolution ops: packed layouts for a training loop that owns every write to its weights
(``packed_weights_cache``), packed layouts plus demodulation squares for an inference pipeline whose weights stay put
(``frozen_weights``).  Both are opt-in, both keep what they cache in a dict owned by the caller, and both are THREAD-LOCAL (forward
passes may run concurrently from several Python threads, op/recorded.py: a sampler in one thread does not switch the training forward
of another thread to cached weights).  Imports `_lib` and torch only, so every op module may import it.
"""
import contextlib
import threading

import torch

from .. import _lib


class _Local(threading.local):
    """which caches are open on this thread; every thread starts with none"""

    def __init__(self):
        self.frozen_on = False
        self.frozen_cache = None
        self.pack_cache = None               # dict while a packed_weights_cache() context is open on this thread


_CACHES = _Local()


# Frozen-weight cache (inference-only pipeline): inside `frozen_weights()` a forward that needs no gradient
# reuses the packed weight layout and the demodulation squares wsq[Co,Ci] of every layer instead of re-deriving them from
# the [Co,Ci,k,k] parameter on every call.  Opt-in because weights can be rewritten behind autograd's back (the reference's
# accumulate() goes through `.data`, train_spatial_query.py:60-61, which does not touch the version counter): whoever opens
# the context promises the weights stay put (inference.GeneratorSampler); an entry is still re-validated against the
# parameter's version counter and storage address.
@contextlib.contextmanager
def frozen_weights(cache):
    """`cache`: a dict owned by the caller (lives as long as the weights it describes)."""
    old = (_CACHES.frozen_on, _CACHES.frozen_cache)
    _CACHES.frozen_on, _CACHES.frozen_cache = True, cache
    try:
        yield
    finally:
        _CACHES.frozen_on, _CACHES.frozen_cache = old


# Packed-weight cache for a TRAINING loop that owns every write to the weights (train_step.TrainStep): inside
# `packed_weights_cache(d)` the packed layouts of a weight tensor are kept in `d` and reused as long as the tensor's version
# counter and storage address are unchanged.  One iteration runs the discriminator three times and the generator twice
# between optimiser steps (train_spatial_query.py:173-224), the regulariser steps pack the same weight once per autograd
# node: ~45 of ~110 packing launches per iteration disappear.  Opt-in and thread-local for the same reason as the
# frozen-weight cache: a write through `.data` does not move the version counter (FusedAdam / MultiTensorEMA do bump it).
@contextlib.contextmanager
def packed_weights_cache(cache):
    old = _CACHES.pack_cache
    _CACHES.pack_cache = cache
    try:
        yield
    finally:
        _CACHES.pack_cache = old


@contextlib.contextmanager
def cache_of(ctx):
    """Backward functions run on the autograd engine's device thread, where the forward thread's `packed_weights_cache()` is
    not visible (thread-local): a node keeps the cache it was built under (`ctx.pack_cache`, set by `keep_cache`) and re-opens
    it around its backward, so the layouts packed there - the data-gradient layout of the closed family in the recorded R1 /
    path-length backward - are cached like the forward's.  Entries stay validated by version counter and base parameter."""
    c = getattr(ctx, 'pack_cache', None)
    if c is None or _CACHES.pack_cache is not None:
        yield
        return
    with packed_weights_cache(c):
        yield


def keep_cache(ctx):
    ctx.pack_cache = _CACHES.pack_cache


def _pack_key(w, pack_kind, wscale):
    return (w.data_ptr(), tuple(w.shape), pack_kind, float(wscale))


def _cacheable(w):
    """only model parameters (or views of them) are cached: an intermediate tensor (the `ggw` of a double backward) may share
    address, shape and version 0 with an earlier one"""
    if _CACHES.pack_cache is None:
        return None
    base = w._base if w._base is not None else w
    return base if isinstance(base, torch.nn.Parameter) else None


def _current(ent, base):
    """THE validity rule of a packed-cache entry (version, layout, base parameter): it was packed from `base` itself, and nothing
    has written to `base` since (a view shares its base's version counter)"""
    return ent is not None and ent[0] == base._version and ent[2] is base


def _store(cache, key, base, wp):
    cache[key] = (base._version, wp, base)      # (keeps the storage alive: the key stays valid)
    return wp


def refresh_packed_weights(cache):
    """Re-derive every stale layout held by `cache` in ONE launch (te_conv_pack_weights_multi_f32), into new buffers.  Called right after an
    optimiser step: the layers that use the weights next then hit the cache instead of issuing ~60 small packing launches per
    iteration.  An entry whose parameter is gone / resized is dropped; entries of untouched parameters cost nothing."""
    jobs, fresh = [], []
    for key, ent in list(cache.items()):
        ptr, shape, pack_kind, wscale = key
        wp, base = ent[1], ent[2]
        if _current(ent, base):
            continue
        n = 1
        for d in shape:
            n *= d
        if not (base.data_ptr() == ptr and base.numel() == n and base.is_contiguous() and len(shape) == 4):
            del cache[key]                # a partial view of the parameter (or a resized one): repacked at its next use
            continue
        # a FRESH buffer per stale layout: the old one may still be held by an autograd node (ctx.wp_bwd / ctx.packs of a graph
        # that outlives the optimiser step - retain_graph, a custom step order); rewriting it in place would make that graph
        # differentiate through the NEW weights without an error
        jobs.append((torch.empty_like(wp), base.detach().view(shape), pack_kind, wscale))      # (ModulatedConv2d.weight is [1,Co,Ci,k,k]: same storage)
        fresh.append((key, base))
    _lib.conv_pack_multi(jobs)
    for (key, base), job in zip(fresh, jobs):
        _store(cache, key, base, job[0])
    return len(jobs)


def packed(w, pack_kind, wscale=1.0):
    """packed layout `pack_kind` of w (through the cache when one is open)"""
    base = _cacheable(w)
    if base is None:
        return _lib.conv_pack(w, pack_kind, wscale)
    cache, key = _CACHES.pack_cache, _pack_key(w, pack_kind, wscale)
    ent = cache.get(key)
    if _current(ent, base):
        return ent[1]
    return _store(cache, key, base, _lib.conv_pack(w, pack_kind, wscale))


def packed2(w, kind_a, kind_b, wscale=1.0):
    """two layouts of w; one launch when both have to be produced"""
    base = _cacheable(w)
    if base is None:
        return _lib.conv_pack2(w, kind_a, kind_b, wscale)
    cache = _CACHES.pack_cache
    ka, kb = _pack_key(w, kind_a, wscale), _pack_key(w, kind_b, wscale)
    if _current(cache.get(ka), base) or _current(cache.get(kb), base):
        return packed(w, kind_a, wscale), packed(w, kind_b, wscale)        # (at most one of them launches)
    wa, wb = _lib.conv_pack2(w, kind_a, kind_b, wscale)
    return _store(cache, ka, base, wa), _store(cache, kb, base, wb)


def frozen_entry(w, kind, wscale, want_wsq, pack_kind=_lib.PACK_FWD):
    """entry {'wp': packed layout, 'wsq': demodulation squares or None} of w in the open frozen-weight cache.  Its stamp is by value
    (the base's version counter and storage address) where _current compares the base by identity: the key already names the base
    (its id()), and the address catches a `.data` swap, which moves neither the id nor the version counter."""
    base = w._base if w._base is not None else w
    key = (id(base), w.data_ptr(), tuple(w.shape), kind, float(wscale), pack_kind)
    stamp = (base._version, base.data_ptr())
    ent = _CACHES.frozen_cache.get(key)
    if ent is None or ent['stamp'] != stamp:
        ent = {'stamp': stamp, 'wp': _lib.conv_pack(w, pack_kind, wscale), 'wsq': None, 'keep': base}
        _CACHES.frozen_cache[key] = ent
    if want_wsq and ent['wsq'] is None:
        w3 = w.reshape(w.shape[0], w.shape[1], -1)
        ent['wsq'] = (w3 * wscale).square().sum(dim=2).contiguous()
    return ent

"""The bottleneck_IR / bottleneck_IR_SE units of the reference's pSp/models/encoders/helpers.py:76-120, shared by the two networks built
on them (arcface.ArcFaceID, the identity network, and psp_encoder.DualSpaceEncoder, the inversion encoder), written once:

    parse_stem / parse_units : input_layer.{0,1,2} and body.N.* of a state dict -> the folded tensors the kernels take
    register_units           : those tensors as the buffers u{i}_{name} of a module
    unit_forward             : one unit on the device

A unit is te_conv2d_prelu_f32 (the leading BatchNorm2d as an affine GATHER in front of the zero-padded convolution: its shift cannot be a
bias, the padded taps do not carry it; then PReLU), te_conv2d_f32 (the second convolution, stride 1 or 2, its batch norm folded in),
te_adaptive_avgpool_f32 to 1 x 1 and te_se_excite_f32 (the gates), the shortcut (the unit's input read with the stride, or te_conv2d_f32
1x1 with its batch norm folded) and te_se_scale_add_f32 (res * gate + shortcut).  Every message names the class the user called (`who`).
"""
import torch

from . import _lib
from .frozen_net import weight_bias
from .inception_features import fold_bn

BN_EPS = 1e-5
BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')
UNIT_BUFFERS = ('scale', 'shift', 'w1', 'slope', 'w2', 'b2', 'fc1', 'fc2')


def reader(sd, who, path, hint):
    """-> (get(key, shape) that returns sd[key] after the shape check and records the key, the set of recorded keys)"""
    read = set()

    def get(key, shape):
        read.add(key)
        return weight_bias(sd, key, None, shape, who, path, hint)
    return get, read


def bn_tensors(get, key, c):
    return [get(f'{key}.{t}', (c,)) for t in BN_KEYS]


def bn_affine(get, key, c):
    """an eval-mode batch norm as (scale, shift) in fp64"""
    g, b, m, v = (t.detach().double().cpu() for t in bn_tensors(get, key, c))
    scale = g / torch.sqrt(v + BN_EPS)
    return scale, b - m * scale


def parse_stem(get, dtype=torch.float32):
    """input_layer = Conv2d(3, c0, 3, 1, 1, bias=False) + BatchNorm2d + PReLU -> (w', b', slope), the batch norm folded in"""
    w0 = get('input_layer.0.weight', (None, 3, 3, 3))
    c0 = w0.shape[0]
    return (*fold_bn(w0, *bn_tensors(get, 'input_layer.1', c0), eps=BN_EPS, dtype=dtype),
            get('input_layer.2.weight', (c0,)).detach().to(dtype).contiguous())


def check_unit_list(units, who):
    if units is None:
        return None
    units = [tuple(int(v) for v in u) for u in units]
    if not units or any(len(u) != 3 or u[0] < 1 or u[1] < 1 or u[2] not in (1, 2) for u in units):
        raise ValueError(f'{who}: units must be a list of (in, depth, stride) with stride 1 or 2, got {units!r}')
    return units


def parse_units(sd, get, ci, units, who, path, hint, dtype=torch.float32):
    """body.0, body.1, ... as long as the keys go on (or as `units`, a checked list of (in, depth, stride), names them) ->
    [dict(cin, depth, stride, scale, shift, w1, slope, w2, b2, fc1, fc2, sc)]; ci: the channels the stem gives.  A stride is not stored
    in a state dict; the reference's rule is taken (helpers.py:26-27 get_block: the first unit of a stage has stride 2, and a stage
    starts at body.0 and wherever in != depth)."""
    parsed, n = [], 0
    while f'body.{n}.res_layer.1.weight' in sd or (units is not None and n < len(units)):
        p = f'body.{n}'
        w1 = get(f'{p}.res_layer.1.weight', (None, None, 3, 3))
        depth, cin = w1.shape[:2]
        if cin != ci:
            raise ValueError(f'{who}: {p}.res_layer.1.weight is {tuple(w1.shape)}: the unit takes {cin} channels, the layer before it gives {ci}')
        stride = 2 if n == 0 or cin != depth else 1
        if units is not None:
            if n >= len(units):
                raise ValueError(f'{who}: {path} has {p}.res_layer.1.weight, past the {len(units)} units that were named')
            if units[n][:2] != (cin, depth):
                raise ValueError(f'{who}: {p}.res_layer.1.weight is {tuple(w1.shape)}, which is not unit {n} of the list, {units[n]}')
            stride = units[n][2]
        scale, shift = bn_affine(get, f'{p}.res_layer.0', cin)
        u = dict(cin=cin, depth=depth, stride=stride, scale=scale.to(dtype).contiguous(), shift=shift.to(dtype).contiguous(),
                 w1=w1.detach().to(dtype).contiguous(), slope=get(f'{p}.res_layer.2.weight', (depth,)).detach().to(dtype).contiguous())
        u['w2'], u['b2'] = fold_bn(get(f'{p}.res_layer.3.weight', (depth, depth, 3, 3)), *bn_tensors(get, f'{p}.res_layer.4', depth), eps=BN_EPS,
                                   dtype=dtype)
        u['fc1'] = u['fc2'] = u['sc'] = None
        if f'{p}.res_layer.5.fc1.weight' in sd or f'{p}.res_layer.5.fc2.weight' in sd:
            fc1 = get(f'{p}.res_layer.5.fc1.weight', (None, depth, 1, 1))
            fc2 = get(f'{p}.res_layer.5.fc2.weight', (depth, fc1.shape[0], 1, 1))
            u['fc1'], u['fc2'] = (t.detach().to(dtype).reshape(t.shape[:2]).contiguous() for t in (fc1, fc2))
        if cin != depth or f'{p}.shortcut_layer.0.weight' in sd:
            u['sc'] = fold_bn(get(f'{p}.shortcut_layer.0.weight', (depth, cin, 1, 1)), *bn_tensors(get, f'{p}.shortcut_layer.1', depth), eps=BN_EPS,
                              dtype=dtype)
        parsed.append(u)
        ci, n = depth, n + 1
    if not parsed:
        raise ValueError(f'{who}: {path} has no body.0.res_layer.1.weight ({hint})')
    return parsed


def register_units(mod, parsed):
    """the units' tensors as buffers u{i}_{name} of `mod`; sets mod.units ((in, depth, stride), ...) and mod.se (has a gate, ...)"""
    mod.units = tuple((u['cin'], u['depth'], u['stride']) for u in parsed)
    mod.se = tuple(u['fc1'] is not None for u in parsed)
    for i, u in enumerate(parsed):
        for k in UNIT_BUFFERS:
            if u[k] is not None:
                mod.register_buffer(f'u{i}_{k}', u[k])
        mod.register_buffer(f'u{i}_zero', torch.zeros(u['depth']))                  # the first convolution has no bias
        if u['sc'] is not None:
            mod.register_buffer(f'u{i}_sc_w', u['sc'][0])
            mod.register_buffer(f'u{i}_sc_b', u['sc'][1])


def unit_forward(mod, i, x):
    """bottleneck_IR(_SE).forward.  An activation is dropped once its last reader has run: the first convolution's output when the
    second has read it, the unit's input (or its convolved shortcut) and the residual branch after the final addition."""
    def g(k):
        return getattr(mod, f'u{i}_{k}', None)
    stride = mod.units[i][2]
    t = _lib.conv2d_prelu(x, g('w1'), g('zero'), g('slope'), g('scale'), g('shift'), 1, (1, 1))
    r = _lib.conv2d(t, g('w2'), g('b2'), stride, (1, 1), act=0)
    del t
    gate = None
    if mod.se[i]:
        gate = _lib.se_excite(_lib.adaptive_avgpool(r, 1, 1).view(r.shape[0], -1), g('fc1'), g('fc2'))
    if g('sc_w') is not None:
        x, stride = _lib.conv2d(x, g('sc_w'), g('sc_b'), stride, (0, 0), act=0), 1
    return _lib.se_scale_add(r, gate, x, stride)


# ------------------------------------------------------------------------------------------------------------ the backward pass
# With respect to the unit's INPUT only: the networks are frozen.  unit_forward_keep is unit_forward (the same bits) that also returns
# what unit_backward reads: the first convolution's pre-activation (the PReLU branch cannot be read from its output: slopes may be
# negative) and, where the unit has a gate, the residual branch, the gates and the pooled vector.  Everything else is dropped.
def dgrad_weights(mod, i):
    """(made once per unit and device: the weights never change) the unit's convolutions in _lib.conv2d_dgrad's layout:
    dict(w1, w2, sc or None)"""
    cache = mod.__dict__.setdefault('_dgrad_weights', {})
    w1 = getattr(mod, f'u{i}_w1')
    key = (i, w1.device)
    if key not in cache:
        stride, sc = mod.units[i][2], getattr(mod, f'u{i}_sc_w', None)
        cache[key] = dict(w1=_lib.dgrad_weight(w1, 1, (1, 1)), w2=_lib.dgrad_weight(getattr(mod, f'u{i}_w2'), stride, (1, 1)),
                          sc=None if sc is None else _lib.dgrad_weight(sc, stride, (0, 0)))
    return cache[key]


def unit_forward_keep(mod, i, x):
    """-> (the unit's output, bitwise unit_forward's; (pre, r, gate, pooled) for unit_backward: r, gate, pooled None without a gate)"""
    def g(k):
        return getattr(mod, f'u{i}_{k}', None)
    stride = mod.units[i][2]
    t, pre = _lib.conv2d_prelu_keep(x, g('w1'), g('zero'), g('slope'), g('scale'), g('shift'), 1, (1, 1))
    r = _lib.conv2d(t, g('w2'), g('b2'), stride, (1, 1), act=0)
    del t
    gate = pooled = None
    if mod.se[i]:
        pooled = _lib.adaptive_avgpool(r, 1, 1).view(r.shape[0], -1)
        gate = _lib.se_excite(pooled, g('fc1'), g('fc2'))
    if g('sc_w') is not None:
        x, stride = _lib.conv2d(x, g('sc_w'), g('sc_b'), stride, (0, 0), act=0), 1
    out = _lib.se_scale_add(r, gate, x, stride)
    return out, (pre, r if mod.se[i] else None, gate, pooled)


def unit_backward(mod, i, kept, gout):
    """the gradient of the unit's input from the gradient of its output [B,depth,Ho,Wo] and what unit_forward_keep kept.  The shortcut
    takes gout as it is; the residual branch goes back through the gate (te_se_bwd_f32), the second convolution and the PReLU (one
    te_conv2d_dgrad_f32, stride 2 in its four phases), then the first convolution, whose epilogue applies the leading batch norm's scale
    and adds the shortcut's gradient: gout spread with the stride (the adjoint of MaxPool2d(1, s)) or the shortcut convolution's own
    data gradient."""
    def g(k):
        return getattr(mod, f'u{i}_{k}', None)
    pre, r, gate, pooled = kept
    cin, depth, stride = mod.units[i]
    B, _, H, W = pre.shape                                                      # the first convolution has stride 1: the input's plane
    wt = dgrad_weights(mod, i)
    gout = gout.contiguous()
    gr = _lib.se_bwd(gout, r, gate, pooled, g('fc1'), g('fc2')) if mod.se[i] else gout
    gt = _lib.conv2d_dgrad(gr, wt['w2'], (B, depth, H, W), (3, 3), stride, (1, 1), pre=pre, slope=g('slope'))
    del gr
    add, add_stride = gout, stride
    if wt['sc'] is not None:
        add, add_stride = _lib.conv2d_dgrad(gout, wt['sc'], (B, cin, H, W), (1, 1), stride, (0, 0)), 1
    return _lib.conv2d_dgrad(gt, wt['w1'], (B, cin, H, W), (3, 3), 1, (1, 1), in_scale=g('scale'), add=add, add_stride=add_stride)

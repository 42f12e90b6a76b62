"""Ranger on the GPU (transeditor_amd.optim.Ranger on te_mt_ranger_f32) against the fp64 restatement (tests/ranger_restated.py), with
the reference class's own fp32 error (tests/golden/ranger_ref.npz) as the yardstick, and the properties the kernel promises bit for
bit: repeatability, independence of the other tensors in the list and of the alignment path, exact zeros for rows of one element.

One optimiser holds the ten shapes of ranger_restated.SHAPES plus a parameter that never gets a gradient.  Thirteen steps cover the
unrectified steps (1-5), the rectified ones (6-13) and the lookahead steps (6 and 12, or 5 and 10 with k = 5).

Measured worst ratios error / bound: profiles/README.md, "Ranger".
"""
import pytest
import torch

import ranger_restated as RR
from conftest import load_golden
from test_ranger_cpu import _golden_state_dict, test_abi_refusals_launch_nothing as _abi_refusals
from transeditor_amd import optim as O

pytestmark = pytest.mark.gpu

ALL = list(range(len(RR.SHAPES)))
BIG = [t for t in ALL if t not in RR.SMALL_IDS]
QUANT = ('p',) + RR.STATE_KEYS
SKIPPED_SHAPE = (6, 5)


def _flat(n, offset):
    """n fp32 elements on the GPU whose address is `offset` floats past a 16-byte boundary"""
    buf = torch.zeros(n + 8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    return buf[offset:offset + n]


def gpu_run(ids, cfg, place='plain', record=RR.RECORD):
    """Steps the tensors `ids` on the GPU -> ({step: {tid: {p, exp_avg, exp_avg_sq, slow_buffer}}} on the CPU, the skipped parameter,
    the optimiser).  place: 'plain' (fresh tensors), 'grads' (gradients and states 4 bytes past a 16-byte boundary, parameters on
    one: the pointers disagree, the scalar path), 'all' (parameters too: the 16-byte path behind a scalar head)."""
    off_p, off_g = {'plain': (0, 0), 'grads': (0, 1), 'all': (1, 1)}[place]
    params = []
    for t in ids:
        src = RR.param0(t)
        v = _flat(src.numel(), off_p).view(src.shape)
        v.copy_(src)
        params.append(torch.nn.Parameter(v))
        assert params[-1].data_ptr() % 16 == 4 * off_p
    skipped = torch.nn.Parameter(torch.full(SKIPPED_SHAPE, 0.25, device='cuda'))
    opt = RR.make_optimizer(O.Ranger, params, ids, cfg)
    opt.add_param_group(dict(params=[skipped]))
    if place != 'plain':
        for p in params:                                   # states of the first step, as the optimiser would make them, but placed
            st = {k: _flat(p.numel(), off_g).view(p.shape) for k in RR.STATE_KEYS}
            st['slow_buffer'].copy_(p.detach())
            opt.state[p] = dict(step=0, **st)
    gbuf = [_flat(p.numel(), off_g).view(p.shape) for p in params]
    out = {}
    for step in range(1, RR.STEPS + 1):
        for t, p, g in zip(ids, params, gbuf):
            g.copy_(RR.grad(t, step))
            p.grad = g
            assert g.data_ptr() % 16 == 4 * off_g
        opt.step()
        if step in record:
            out[step] = {t: dict(p=p.detach().cpu(), **{k: opt.state[p][k].cpu() for k in RR.STATE_KEYS}) for t, p in zip(ids, params)}
    return out, skipped, opt


@pytest.fixture(scope='module')
def refs():
    """computed once, left unchanged: the fp64 restatement of every shape, and the yardstick max|x32 - x64| per tensor and quantity:
    the reference class's fp32 results from the fixture for the small shapes, the restatement in fp32 on the CPU for the others"""
    gold = load_golden('ranger_ref')
    x64, yard = {}, {}
    for cfg in RR.CONFIGS:
        x64[cfg] = RR.run(ALL, cfg, torch.float64)
        x32 = RR.run(BIG, cfg, torch.float32)
        for step in RR.RECORD:
            for t in ALL:
                for k in QUANT:
                    ref32 = gold[f'{cfg}_s{step}_{t}_{k}'] if t in RR.SMALL_IDS else x32[step][t][k]
                    yard[cfg, step, t, k] = float((ref32.double() - x64[cfg][step][t][k]).abs().max())
    return gold, x64, yard


@pytest.fixture(scope='module')
def plain():
    """the plain GPU run of each configuration, shared by the tests that compare against it"""
    return {cfg: gpu_run(ALL, cfg) for cfg in RR.CONFIGS}


def _check(got, x64, yard, cfg, ids, steps, label):
    worst = {}
    fails = []
    for step in steps:
        for t in ids:
            for k in QUANT:
                ref = x64[cfg][step][t][k]
                x = got[step][t][k]
                assert x.dtype == torch.float32 and x.shape == ref.shape
                err, mag = float((x.double() - ref).abs().max()), float(ref.abs().max())
                bound = max(4 * yard[cfg, step, t, k], 2.0 ** -20 * mag)
                ratio = err / bound if bound else (0.0 if err == 0 else float('inf'))
                if ratio > worst.get(k, (0.0,))[0]:
                    worst[k] = (ratio, step, t, err, bound)
                if not err <= bound:
                    fails.append((cfg, step, t, RR.SHAPES[t], k, err, bound))
    for k, (ratio, step, t, err, bound) in worst.items():
        print(f'ranger {label} ({cfg}) {k}: worst error / bound {ratio:.3f} (step {step}, {RR.SHAPES[t]}, err {err:.3e}, bound {bound:.3e})')
    assert not fails, fails


@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_accuracy_against_fp64(refs, plain, cfg):
    """per tensor, max|x_gpu - x64| <= max(4 * yardstick, 2^-20 max|x64|) for p, exp_avg, exp_avg_sq and slow_buffer after steps 7
    and 13 (the factor 4: the project's standing margin over torch's own fp32 error)"""
    _, x64, yard = refs
    _check(plain[cfg][0], x64, yard, cfg, ALL, RR.RECORD, 'accuracy')


def test_rows_of_one_element_are_exact(plain):
    """(5, 1) under the defaults: a row's mean is its one element, the centralised gradient is exactly 0, so nothing moves"""
    for step in RR.RECORD:
        s = plain['a'][0][step][3]
        assert torch.equal(s['p'], RR.param0(3)) and torch.equal(s['slow_buffer'], RR.param0(3))
        assert torch.equal(s['exp_avg'], torch.zeros(5, 1)) and torch.equal(s['exp_avg_sq'], torch.zeros(5, 1))


@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_parameter_without_gradient_is_skipped(plain, cfg):
    _, skipped, opt = plain[cfg]
    assert torch.equal(skipped.detach().cpu(), torch.full(SKIPPED_SHAPE, 0.25)) and skipped._version == 0
    assert skipped not in opt.state and len(opt.state) == len(ALL)
    assert all(type(st['step']) is int and st['step'] == RR.STEPS and set(st) == {'step', *RR.STATE_KEYS} for st in opt.state.values())


def _same_bits(a, b, ids, steps=RR.RECORD):
    return [(step, t, k) for step in steps for t in ids for k in QUANT if not torch.equal(a[step][t][k], b[step][t][k])]


@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_bitwise_repeat(plain, cfg):
    again, _, _ = gpu_run(ALL, cfg)
    assert not _same_bits(plain[cfg][0], again, ALL)


@pytest.mark.parametrize('tid', [5, 8])
def test_context_independence(plain, tid):
    """(1171, 14) and (3, 512, 3, 3) stepped alone give the bits they get inside the full list"""
    alone, _, _ = gpu_run([tid], 'a')
    assert not _same_bits(plain['a'][0], alone, [tid])


@pytest.mark.parametrize('place', ['grads', 'all'])
@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_alignment_paths_agree_bit_for_bit(plain, cfg, place):
    """gradients and states (and, for 'all', the parameters) 4 bytes past a 16-byte boundary inside a flat buffer, as gradients sit in
    the GradSync buckets: the scalar path, or the 16-byte path behind a scalar head, give the bits of the aligned run"""
    moved, _, _ = gpu_run(ALL, cfg, place=place)
    assert not _same_bits(plain[cfg][0], moved, ALL)


@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_continues_from_the_references_state_dict(refs, cfg):
    """the step-7 state_dict the reference's class wrote (the fixture) is loaded, steps 8-13 are taken, and the result is the
    reference's step 13 within the accuracy bound"""
    gold, x64, yard = refs
    sd, order = _golden_state_dict(gold, cfg, 7)
    params = [torch.nn.Parameter(gold[f'{cfg}_s7_{t}_p'].cuda()) for t in RR.SMALL_IDS]
    opt = RR.make_optimizer(O.Ranger, params, RR.SMALL_IDS, cfg)
    opt.load_state_dict(sd)
    for step in range(8, RR.STEPS + 1):
        for t, p in zip(RR.SMALL_IDS, params):
            p.grad = RR.grad(t, step).cuda()
        opt.step()
    got = {13: {t: dict(p=p.detach().cpu(), **{k: opt.state[p][k].cpu() for k in RR.STATE_KEYS}) for t, p in zip(RR.SMALL_IDS, params)}}
    assert all(opt.state[p]['step'] == 13 for p in params)
    _check(got, x64, yard, cfg, RR.SMALL_IDS, [13], 'from the state dict')


def test_version_counters_advance():
    p = torch.nn.Parameter(RR.param0(4).cuda())
    opt = O.Ranger([p])
    p.grad = RR.grad(4, 1).cuda()
    v0 = p._version
    opt.step()
    assert p._version > v0
    v1 = p._version
    opt.step()
    assert p._version > v1


def test_refusals():
    g = RR.grad(4, 1)
    cpu = torch.nn.Parameter(RR.param0(4))
    cpu.grad = g.clone()
    with pytest.raises(RuntimeError, match='Ranger needs contiguous fp32 parameters on the GPU'):
        O.Ranger([cpu]).step()
    half = torch.nn.Parameter(RR.param0(4).cuda().half())
    half.grad = g.cuda().half()
    with pytest.raises(RuntimeError, match='Ranger needs contiguous fp32 parameters on the GPU, got torch.float16'):
        O.Ranger([half]).step()
    sp = torch.nn.Parameter(RR.param0(4).cuda())
    sp.grad = g.cuda().to_sparse()
    opt = O.Ranger([sp])
    with pytest.raises(RuntimeError, match='Ranger does not support sparse gradients'):
        opt.step()
    assert torch.equal(sp.detach().cpu(), RR.param0(4)) and sp not in opt.state
    _abi_refusals()
    torch.cuda.synchronize()

"""Ranger without a GPU (transeditor_amd.optim.Ranger, te_mt_ranger_f32): the fp64 restatement (tests/ranger_restated.py) against
what the reference's own class computed in fp32 (tests/golden/ranger_ref.npz, written by tools/ranger_golden.py), the RAdam
schedule against the reference's, the class surface and the state_dict interchange, the host planner's work map, and the ABI."""
import ctypes
import json
import os
import re

import pytest
import torch

import ranger_restated as RR
from conftest import ROOT, load_golden
from oracle.ref_import import REF_ROOT
from transeditor_amd import optim as O

# where the oracle looks for the reference tree; the tests that want its class do without it where it is absent
REFERENCE_RANGER = os.path.join(REF_ROOT, 'pSp', 'training', 'ranger.py')


@pytest.fixture(scope='module')
def gold():
    return load_golden('ranger_ref')


# ------------------------------------------------------------------------------------------- restatement against golden
@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_restatement_matches_the_reference_to_fp32_rounding(gold, cfg):
    """max|x32 - x64| <= 2^-20 max|x64| per tensor, for p, m, v and slow after steps 7 and 13 (measured: at most 0.30 of the bound,
    tests/golden/RANGER_REPORT.txt)"""
    x64 = RR.run(RR.SMALL_IDS, cfg, torch.float64)
    for step in RR.RECORD:
        for t in RR.SMALL_IDS:
            for k in ('p',) + RR.STATE_KEYS:
                ref32, mine = gold[f'{cfg}_s{step}_{t}_{k}'], x64[step][t][k]
                assert ref32.dtype == torch.float32 and ref32.shape == mine.shape
                err, mag = float((ref32.double() - mine).abs().max()), float(mine.abs().max())
                assert err <= 2.0 ** -20 * mag, (cfg, step, t, k, err, mag)
    # the inputs are the fixture's: the initial parameters are bit for bit param0()
    assert all(torch.equal(gold[f'{cfg}_p0_{t}'], RR.param0(t)) for t in RR.SMALL_IDS)


def test_gradients_are_exact_and_off_centre():
    for t in range(len(RR.SHAPES)):
        g = RR.grad(t, 3)
        assert g.dtype == torch.float32 and g.shape == RR.SHAPES[t]
        k = g.double() * 2.0 ** 23
        assert torch.equal(k, k.round()) and float(g.min()) >= -0.6875 and float(g.max()) < 1.3125
        assert not torch.equal(g, RR.grad(t, 4))
    rows = RR.grad(5, 2).reshape(1171, 14).double().mean(1)
    assert float(rows.abs().median()) > 0.2 and abs(float(rows.mean()) - 0.3125) < 0.01      # centralisation moves every row
    assert abs(float(RR.grad(9, 2).double().mean()) - 0.3125) < 0.01


# ---------------------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_schedule_is_the_references(gold, cfg):
    c = RR.CONFIGS[cfg]
    ref = gold[f'{cfg}_schedule']
    assert ref.shape == (RR.STEPS, 2) and ref.dtype == torch.float64
    rect = []
    for step in range(1, RR.STEPS + 1):
        n_sma, step_size, rectified = O.radam_schedule(step, *c['betas'], c['N_sma_threshhold'])
        assert abs(n_sma - float(ref[step - 1, 0])) <= 1e-15 * abs(float(ref[step - 1, 0]))
        assert abs(step_size - float(ref[step - 1, 1])) <= 1e-15 * abs(float(ref[step - 1, 1]))
        assert (n_sma, step_size, rectified) == RR.schedule(step, *c['betas'], c['N_sma_threshhold'])
        rect.append(rectified)
    assert rect == [False] * 5 + [True] * 8           # N_sma passes 5 between steps 5 and 6 in both configurations


def test_schedule_is_per_group():
    """the reference shares (N_sma, step_size) between groups of different betas through radam_buffer; here each group has its own"""
    a, b = O.radam_schedule(8, 0.95, 0.999, 5), O.radam_schedule(8, 0.9, 0.99, 5)
    assert a != b and a[2] and b[2]
    assert O.radam_schedule(8, 0.9, 0.99, 8) == (b[0], 1.0 / (1 - 0.9 ** 8), False)


# ------------------------------------------------------------------------------------------------------- class surface
def _params(ids):
    return [torch.nn.Parameter(RR.param0(t).clone()) for t in ids]


def test_constructor_defaults_and_refusals():
    p = _params([0, 4])
    opt = O.Ranger(p)
    g = opt.param_groups[0]
    assert {k: v for k, v in g.items() if k != 'params'} == dict(lr=1e-3, alpha=0.5, k=6, step_counter=0, betas=(.95, 0.999),
                                                                 N_sma_threshhold=5, eps=1e-5, weight_decay=0)
    assert (opt.alpha, opt.k, opt.N_sma_threshhold, opt.use_gc, opt.gc_gradient_threshold) == (0.5, 6, 5, True, 1)
    assert O.Ranger(p, gc_conv_only=True).gc_gradient_threshold == 3
    assert isinstance(opt, torch.optim.Optimizer) and opt.state_dict()['state'] == {}
    for kw, msg in ((dict(alpha=1.5), 'Invalid slow update rate: 1.5'), (dict(alpha=-0.1), 'Invalid slow update rate'),
                    (dict(k=0), 'Invalid lookahead steps: 0'), (dict(lr=0), 'Invalid Learning Rate: 0'),
                    (dict(lr=-1.0), 'Invalid Learning Rate'), (dict(eps=0), 'Invalid eps: 0')):
        with pytest.raises(ValueError, match=msg):
            O.Ranger(p, **kw)


def test_no_cpu_path():
    p = _params([4])
    p[0].grad = RR.grad(4, 1)
    with pytest.raises(RuntimeError, match='Ranger needs contiguous fp32 parameters on the GPU'):
        O.Ranger(p).step()
    assert O.Ranger(p).state_dict()['state'] == {}
    q = _params([4])                                    # without a gradient nothing is touched and nothing raises
    O.Ranger(q).step()


def _reference_class():
    import importlib.util
    spec = importlib.util.spec_from_file_location('reference_ranger', REFERENCE_RANGER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Ranger


def _golden_state_dict(gold, cfg, step):
    """the state_dict() the reference's class wrote at `step`, put together from the fixture"""
    groups = json.loads(str(gold[f'{cfg}_param_groups']))
    state = {}
    order = [t for g in range(len(groups)) for t in RR.SMALL_IDS if RR.group_of(t, cfg) == g]
    for i, t in enumerate(order):
        state[i] = dict(step=step, **{k: gold[f'{cfg}_s{step}_{t}_{k}'].clone() for k in RR.STATE_KEYS})
    assert [i for g in groups for i in g['params']] == list(range(len(order)))
    return {'state': state, 'param_groups': groups}, order


@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_state_dict_interchange(gold, cfg):
    sd, order = _golden_state_dict(gold, cfg, 7)
    params = _params(RR.SMALL_IDS)
    opt = RR.make_optimizer(O.Ranger, params, RR.SMALL_IDS, cfg)
    # the param-group layout is the reference's, key for key and value for value
    mine = opt.state_dict()['param_groups']
    assert json.loads(json.dumps(mine)) == sd['param_groups']
    opt.load_state_dict(sd)
    by_id = dict(zip(RR.SMALL_IDS, params))
    for t in order:
        st = opt.state[by_id[t]]
        assert set(st) == {'step', 'exp_avg', 'exp_avg_sq', 'slow_buffer'} and type(st['step']) is int and st['step'] == 7
        for k in RR.STATE_KEYS:
            assert st[k].dtype == torch.float32 and torch.equal(st[k], gold[f'{cfg}_s7_{t}_{k}'])
    out = opt.state_dict()
    assert json.loads(json.dumps(out['param_groups'])) == sd['param_groups'] and set(out['state']) == set(sd['state'])
    if os.path.exists(REFERENCE_RANGER):
        # ours -> the reference's class, which then steps on from it as from its own
        Ref = _reference_class()
        import warnings
        p_ref = [torch.nn.Parameter(gold[f'{cfg}_s7_{t}_p'].clone()) for t in RR.SMALL_IDS]
        ref = RR.make_optimizer(Ref, p_ref, RR.SMALL_IDS, cfg)
        assert json.loads(json.dumps(ref.state_dict()['param_groups'])) == sd['param_groups']
        ref.load_state_dict(out)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for step in range(8, RR.STEPS + 1):
                for t, p in zip(RR.SMALL_IDS, p_ref):
                    p.grad = RR.grad(t, step).clone()
                ref.step()
        for t, p in zip(RR.SMALL_IDS, p_ref):
            assert torch.equal(p.detach(), gold[f'{cfg}_s13_{t}_p']) and ref.state[p]['step'] == 13
            assert all(torch.equal(ref.state[p][k], gold[f'{cfg}_s13_{t}_{k}']) for k in RR.STATE_KEYS)


def test_encoder_optimizer_is_configure_optimizers():
    p = _params([0, 4])
    a = O.encoder_optimizer(p, 'adam', 3e-4)
    assert type(a) is O.FusedAdam and a.param_groups[0]['lr'] == 3e-4 and a.param_groups[0]['betas'] == (0.9, 0.999)
    for name in ('ranger', 'sgd', ''):
        r = O.encoder_optimizer(p, name, 1e-4)
        assert type(r) is O.Ranger and r.param_groups[0]['lr'] == 1e-4 and r.param_groups[0]['betas'] == (.95, 0.999)
    assert type(O.encoder_optimizer(p)) is O.Ranger


# ------------------------------------------------------------------------------------------------------------ work map
def _encoder_shapes():
    """the parameters of the true encoder (the key and shape list of the reference's GradualStyleEncoder in the fixture, which
    tests/test_psp_encoder_cpu.py holds equal to psp_encoder_restated.state_dict's)"""
    z = load_golden('psp_encoder_ref')
    shapes = [tuple(int(v) for v in str(s).split(',') if v) for k, s in zip(z['keys'], z['shapes'])
              if not str(k).endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
    assert len(shapes) > 500 and shapes.count((512, 512, 3, 3)) == 138 + 5           # (the heads' and the body's)
    assert (16, 14) in shapes
    return shapes


@pytest.mark.parametrize('conv_only', [False, True])
@pytest.mark.parametrize('tile', [O.TILE, 2048])
def test_work_map_properties(conv_only, tile):
    shapes = list(RR.SHAPES) + _encoder_shapes()
    numels = [torch.Size(s).numel() for s in shapes]
    lens = [O.gc_row_len(s, True, conv_only) for s in shapes]
    # L == 0 exactly for the tensors the reference would not centralise (grad.dim() > threshold, ranger.py:118), else the row
    for s, ne, L in zip(shapes, numels, lens):
        if len(s) > (3 if conv_only else 1):
            assert L == ne // s[0] and L * s[0] == ne and L > 0
        else:
            assert L == 0
    assert all(O.gc_row_len(s, False, conv_only) == 0 for s in shapes)
    w = O.row_groups(numels, lens, tile)
    assert w.dtype == torch.int32 and w.shape[0] == 3 and w.shape[1] > 0
    t, first, count = (w[i].to(torch.int64) for i in range(3))
    ne, L = torch.tensor(numels)[t], torch.tensor(lens)[t]
    row = torch.where(L > 0, L, torch.full_like(L, tile))                     # L == 0: "rows" of `tile` elements
    rows_of = torch.where(L > 0, ne // torch.clamp(L, min=1), -(-ne // tile))
    assert bool((count >= 1).all()) and bool((first >= 0).all()) and bool((first + count <= rows_of).all())      # whole rows
    assert bool(((count * row <= tile) | (count == 1)).all())                  # over the tile only as a single row
    # every row of every tensor is in exactly one entry: per tensor, the entries tile [0, rows) in order without gaps
    assert bool((t[1:] >= t[:-1]).all()) and set(t.tolist()) == set(range(len(shapes)))
    same = t[1:] == t[:-1]
    assert bool(((first[1:] == first[:-1] + count[:-1]) | ~same).all())
    starts = torch.ones_like(t, dtype=torch.bool)
    starts[1:] = ~same
    ends = torch.ones_like(starts)
    ends[:-1] = ~same
    assert bool((first[starts] == 0).all()) and bool(((first + count)[ends] == rows_of[ends]).all())
    # and the groups are as large as the tile allows
    full = ~ends & (L > 0) & (L <= tile)
    assert bool(((count[full] + 1) * L[full] > tile).all())


def test_work_map_small_cases():
    w = O.row_groups([3, 20000, 16 * 14, 2 * 20003, 0], [0, 0, 14, 20003, 0])
    assert w.tolist() == [[0, 1, 1, 1, 2, 3, 3], [0, 0, 1, 2, 0, 0, 1], [1, 1, 1, 1, 16, 1, 1]]
    w = O.row_groups([1171 * 14], [14])
    assert w.tolist() == [[0, 0, 0], [0, 584, 1168], [584, 584, 3]] and 584 * 14 <= O.TILE < 585 * 14
    with pytest.raises(ValueError, match='whole rows'):
        O.row_groups([10], [3])
    assert O.TILE % 4 == 0 and O.TILE * 4 + 32 == 32768


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_abi_entry_point():
    from transeditor_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    assert len(re.findall(r'\bte_mt_ranger_f32\b', header)) == 1
    assert 'te_mt_ranger_f32' in _lib.EXPORTS and _lib.mt_ranger in _lib._OPS
    assert _lib.EXPORTS.index('te_mt_ranger_f32') == _lib.EXPORTS.index('te_mt_ema_f32') + 1       # next to its siblings
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, 'te_mt_ranger_f32')
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert tuple(_lib.lib().te_mt_ranger_f32.argtypes) == (P, P, I, I, I, D, D, D, D, D, D, I, I, P)


def test_abi_refusals_launch_nothing():
    """the argument checks are host code: NULL tables, non-positive counts, a bad tile, beta, eps or alpha return the error code and
    set te_last_error_string"""
    from transeditor_amd import _lib
    L = _lib.lib()
    ok = dict(table=8, work=8, n=1, n_work=1, tile=O.TILE, step_lr=1e-3, decay=0.0, beta1=0.95, beta2=0.999, eps=1e-5, alpha=0.5,
              rect=1, look=0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.te_mt_ranger_f32(a['table'], a['work'], a['n'], a['n_work'], a['tile'], a['step_lr'], a['decay'], a['beta1'], a['beta2'],
                                  a['eps'], a['alpha'], a['rect'], a['look'], None)
    cases = [(dict(table=None), -1, 'NULL'), (dict(work=None), -1, 'NULL'), (dict(n=0), -2, 'dims'), (dict(n_work=0), -2, 'dims'),
             (dict(n_work=-3), -2, 'dims'), (dict(tile=8182), -2, 'multiple of 4'), (dict(tile=0), -2, 'tile'),
             (dict(tile=8188), -2, 'tile'), (dict(beta1=1.0), -2, 'beta'), (dict(beta2=-0.1), -2, 'beta'), (dict(eps=0.0), -2, 'eps'),
             (dict(alpha=1.5), -2, 'alpha'), (dict(alpha=-0.5), -2, 'alpha')]
    for kw, code, word in cases:
        assert call(**kw) == code, kw
        msg = L.te_last_error_string().decode()
        assert msg.startswith('te_mt_ranger_f32') and word in msg, (kw, msg)

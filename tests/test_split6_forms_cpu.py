"""The instruments of tests/test_gpu_split6_forms.py proved on the CPU restatement of the split (tests/split6_restated.py) before any GPU
sees them, and the form table of the split-bf16 family (tests/split6_forms.py) held to the library's queries.  No GPU: the restatement
is plain torch, the plans are host code.

For every kind of arithmetic in the family: the intact restatement passes the elementwise bound, the grouped rms and the live-channel
bar; with one of the products mm / hl / lh dropped, or the m and l pieces of one operand swapped, in ONE group of outputs (dense
operands) or for ONE live channel (sweep), the matching instrument fails - while the whole-tensor figures of the family's older tests
(max err / max ref < 5e-6, l2 < 2.5 l2_fp32 + 1e-7) pass on the same mutated data.  That last assertion is the reason the module exists.
"""
import ctypes as C
import itertools
import math

import pytest
import torch

import host_plans as hp
import split6_forms as sf
import split6_restated as sr
from fp64_check import KINK_CAP, U32 as U
from transeditor_amd import _lib

IDS = lambda e: e.name
MUTATIONS = ({'drop': 'mm'}, {'drop': 'hl'}, {'drop': 'lh'}, {'swap': 'a'}, {'swap': 'b'})
K = 32


# ------------------------------------------------------------------------------------------------ the restatement and the instruments
def _operands(kind):
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(s, generator=g)
    if kind == 'direct9':
        return rn(64, K, 3, 3) / math.sqrt(9 * K), rn(2, K, 17, 33)
    if kind == 'tap1':
        return rn(128, 4 * K, 1, 1) / math.sqrt(4 * K), rn(2, 4 * K, 16, 32)
    if kind == 'wino_row':
        return rn(64, K, 3, 3) / math.sqrt(9 * K), rn(2, K, 8, 32)
    if kind == 'wg_pair':
        return rn(2, 64, 16, 32), rn(2, 64, 16, 32)
    return rn(2, 128, 16, 32), rn(2, 128, 16, 32)


def _groups(kind, shape):
    """(groups, mask of the outputs that the dense mutations hit: a quarter of one column class - four rows of a tile in one sample -, one
    tap, or the cross of a channel quarter on either side)"""
    ar = lambda n: torch.arange(n)
    if kind in ('wg_pair', 'wg_tap1'):
        Co, Ci, taps = shape
        g = {'co': (ar(Co) % 128 // 32).view(Co, 1, 1), 'ci': (ar(Ci) % 128 // 32).view(1, Ci, 1)}
        if taps == 9:
            g['tap'] = ar(9).view(1, 1, 9)
            return g, (g['tap'] == 4).expand(shape)
        return g, ((g['co'] == 1) & (g['ci'] == 2)).expand(shape)
    B, M, H, W = shape
    wcol = 32 if kind == 'wino_row' else 16
    g = {'m quarter': (ar(M) % 128 // 32).view(1, M, 1, 1), 'sample': ar(B).view(B, 1, 1, 1), 'row % 8': (ar(H) % 8).view(1, 1, H, 1),
         f'col % {wcol}': (ar(W) % wcol).view(1, 1, 1, W)}
    return g, ((g[f'col % {wcol}'] == 5) & (g['sample'] == 0) & (g['row % 8'] < 4)).expand(shape)


def _coefficient(kind, a, b):
    """the multiple of u S that bounds the restatement (two accumulators, as six_products keeps them): L (1 + 5 / 128) + 1 for a chain
    of L products, the transforms' roundings and 0.5 for the dropped terms (docstring of tests/test_gpu_split6_forms.py)"""
    chain = lambda L: L * (1 + 5 / 128) + 1
    if kind == 'direct9':
        return chain(9 * a.shape[1]) + 0.5
    if kind == 'tap1':
        return chain(a.shape[1]) + 0.5
    if kind == 'wino_row':
        return chain(3 * a.shape[1]) + 1 + 2 + 2 + 0.5
    pixels = b.shape[0] * b.shape[2] * b.shape[3]
    return chain(pixels // 2) + 2 + 3 + 0.5 if kind == 'wg_pair' else chain(pixels) + 0.5


@pytest.fixture(scope='module', params=sr.KINDS)
def case(request):
    """operands, fp64 reference, fp32 yardstick and intact restatement of a kind, computed once"""
    kind = request.param
    a, b = _operands(kind)
    ref = sr.reference(kind, a, b)
    groups, hit = _groups(kind, ref.shape)
    return {'kind': kind, 'a': a, 'b': b, 'ref': ref, 'yard': sr.yardstick(kind, a, b), 'got': sr.emulate(kind, a, b),
            'bound': _coefficient(kind, a, b) * U * sr.abs_sum(kind, a, b), 'groups': groups, 'hit': hit}


def _older_figures_pass(got, yard, ref):
    rel, l2, limit = sr.whole_tensor_figures(got, yard, ref)
    return rel < 5e-6 and l2 < limit


def test_intact_restatement_passes_the_dense_instruments(case):
    c = case
    err = (c['got'].double() - c['ref']).abs()
    assert float((err / c['bound']).max()) <= 1.0 and float(((c['yard'].double() - c['ref']).abs() / c['bound']).max()) <= 1.0
    worst, n, where = sr.grouped_rms(c['got'], c['yard'], c['ref'], c['groups'])
    print(f'{c["kind"]}: {n} groups, worst rms / limit {worst:.3f} at {where}')
    assert n >= 6 and worst < 0.5
    assert _older_figures_pass(c['got'], c['yard'], c['ref'])


@pytest.mark.parametrize('mutation', MUTATIONS, ids=lambda m: '_'.join(f'{k}_{v}' for k, v in m.items()))
def test_a_product_lost_in_one_group_fails_the_grouped_rms_only(case, mutation):
    c = case
    bad = torch.where(c['hit'], sr.emulate(c['kind'], c['a'], c['b'], **mutation), c['got'])
    share = float(c['hit'].double().mean())
    assert 0 < share <= 1 / 9
    worst, n, where = sr.grouped_rms(bad, c['yard'], c['ref'], c['groups'])
    rel, l2, limit = sr.whole_tensor_figures(bad, c['yard'], c['ref'])
    ew = float(((bad.double() - c['ref']).abs() / c['bound']).max())
    print(f'{c["kind"]} {mutation} in {share:.3f} of the outputs: group rms / limit {worst:.2f} at {where}; max err / max ref {rel:.2e}, l2 {l2:.2e} < {limit:.2e}; '
          f'max err / bound {ew:.3f}')
    assert worst > 1.2, 'the grouped rms must see it'
    assert rel < 5e-6 and l2 < limit, 'the whole-tensor figures of the older tests do not'
    assert ew <= 1.0, 'nor does the worst-case elementwise bound'


def _live(kind, a, b, c):
    """the operands with one live channel (conv kinds: channel c of x) or one live cell column (weight gradients: columns = c mod 32 of g)"""
    if kind in ('wg_pair', 'wg_tap1'):
        live = (torch.arange(a.shape[-1]) % 32 == c).float()
        return a * live, b
    x = torch.zeros_like(b)
    x[:, c] = b[:, c]
    return a, x


def test_live_channel_bar_separates_intact_from_mutated(case):
    """the sweep: every channel (cell column) alive in turn; the intact restatement and torch's fp32 stay under the bar, each mutation
    applied to channel 3 only is over it there - and added to the dense result it passes the older whole-tensor figures"""
    c = case
    kind, a, b = c['kind'], c['a'], c['b']
    worst = {'split': 0.0, 'fp32': 0.0}
    for ch in range(32):
        la, lb = _live(kind, a, b, ch)
        ref = sr.reference(kind, la, lb)
        worst['split'] = max(worst['split'], sr.live_rms(sr.emulate(kind, la, lb), ref, c['groups'])[0])
        worst['fp32'] = max(worst['fp32'], sr.live_rms(sr.yardstick(kind, la, lb), ref, c['groups'])[0])
    print(f'{kind}: worst live rms / bar {worst["split"]:.3f} (fp32 {worst["fp32"]:.3f}); 2^{math.log2(worst["split"] * sr.LIVE_BAR):.1f}')
    assert worst['split'] <= 0.25 and worst['fp32'] <= 0.25           # intact: 2^-23 or better in every group, a quarter of the bar
    la, lb = _live(kind, a, b, 3)
    ref, intact = sr.reference(kind, la, lb), sr.emulate(kind, la, lb)
    # the dense launch of a kernel that loses the product for channel 3 only, at 64 channels (a second, independent half; the weight
    # gradients sum over 32 cell columns per row as they are): at 32 channels the row form's whole-tensor L2 sits at its limit
    if kind in ('wg_pair', 'wg_tap1'):
        a2, b2 = a, b
    else:
        a2 = torch.cat([a, a.flip(0)], 1) / math.sqrt(2)
        b2 = torch.cat([b, b.flip(1)], 1)
        intact_wide = sr.emulate(kind, *_live(kind, a2, b2, 3))
    ref2, yard2, got2 = sr.reference(kind, a2, b2), sr.yardstick(kind, a2, b2), sr.emulate(kind, a2, b2)
    for mutation in MUTATIONS:
        bad = sr.emulate(kind, la, lb, **mutation)
        r, n, where = sr.live_rms(bad, ref, c['groups'])
        if kind in ('wg_pair', 'wg_tap1'):
            dense = got2 + (bad - intact)
        else:
            dense = got2 + (sr.emulate(kind, *_live(kind, a2, b2, 3), **mutation) - intact_wide)
        g, _, _ = sr.grouped_rms(dense, yard2, ref2, c['groups'])
        rel, l2, limit = sr.whole_tensor_figures(dense, yard2, ref2)
        print(f'{kind} {mutation} for channel 3: live rms / bar {r:.2f} (2^{math.log2(r * sr.LIVE_BAR):.1f}); dense: group rms / limit {g:.3f}, '
              f'max err / max ref {rel:.2e}, l2 {l2:.2e} < {limit:.2e}')
        assert r > 4.0, 'the live channel must see it, four times over the bar'
        assert rel < 5e-6 and l2 < limit, 'the whole-tensor figures of the older tests do not'


def test_pooling_never_skips_a_group():
    cnt = torch.tensor([600, 100, 0, 100, 400, 512, 3])
    assert sr.pooled(cnt) == [[0], [1, 3, 4], [5, 6]]
    assert sr.pooled(torch.tensor([5, 7])) == [[0, 1]] and sr.pooled(torch.tensor([0, 0])) == []
    label = torch.tensor([0, 1, -1, 1]).view(1, 4)
    cnt, (s,) = sr.group_sums(label, (3, 4), None, [torch.ones(3, 4)])
    assert cnt.tolist() == [3, 6] and s.tolist() == [3.0, 6.0]
    keep = torch.tensor([[True, True, True, False]] * 3)
    cnt, (s,) = sr.group_sums(label, (3, 4), keep, [torch.full((3, 4), 2.0)])
    assert cnt.tolist() == [3, 3] and s.tolist() == [6.0, 6.0]


def test_split3_is_exact_and_ordered():
    v = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * torch.logspace(-20, 20, 4096)
    h, m, l = sr.split3(v)
    assert torch.equal(h + m + l, v) or float(((h.double() + m.double() + l.double() - v.double()).abs() / v.abs().double()).max()) <= 2.0 ** -24
    assert bool((m.abs() <= 2.0 ** -8 * v.abs()).all()) and bool((l.abs() <= 2.0 ** -16 * v.abs()).all())
    for p in (h, m, l):
        assert torch.equal(p.bfloat16().float(), p)


# ------------------------------------------------------------------------------------------------ the table against the queries
@pytest.mark.parametrize('entry', sf.TABLE, ids=IDS)
def test_entry_lands_on_its_key(entry):
    e = entry
    f = sf.check(e)
    for what, hv, scr, key in sf.twins(e):
        assert key != e.key or dict(hv) != dict(e.hooks), (e.name, what)
        sf.check(e, hv, scr, key)
    if isinstance(e, sf.Fwd):
        B, Kc, M, H, W = e.shape
        assert f['isc'] == e.isc and f['blocks'] * 1 >= f['ntiles'] * f['mblocks'] // max(1, f['tpb'] if f['lists'] else 1)
        assert f['mblocks'] == M // (128 if f['two_image'] else 64)
        if not f['lists']:
            assert f['blocks'] == -(-f['ntiles'] // 8) * 8 * f['mblocks'] and f['idle'] == f['blocks'] - f['ntiles'] * f['mblocks']
        if e.name not in sf.LARGE:
            assert B * M * max(H * W, 1) * (4 if e.kind == sf.T2 else 1) <= 6 << 20, 'a small entry'
    else:
        assert sf.chunk_masks(e).shape[0] == e.S


def test_idle_blocks_restated():
    """te_conv_split_form's idle count against split6_tile / split6_tile_list restated block by block (banded order)"""
    for e in sf.FWD:
        f = sf.answer(e)
        n, mb, lists = f['ntiles'], f['mblocks'], f['lists']
        slots = lists if lists else -(-n // 8)
        idle = 0
        for xcd in range(8):
            nb = (xcd + 1) * n // 8 - xcd * n // 8
            for q in range(slots):
                lo, hi = (q * nb // lists, (q + 1) * nb // lists) if lists else (q, q + 1 if q < nb else q)
                idle += mb * (lo >= hi)
        assert f['blocks'] == 8 * slots * mb and f['idle'] == idle, e.name


def test_table_covers_what_it_was_written_for():
    T = sf.FWD
    ans = {e: sf.answer(e) for e in T}
    some = lambda pred: [e for e in T if pred(e, ans[e])]
    w6, s2, t2, p1 = (lambda e, f, k=k: e.kind == k for k in (sf.W6, sf.S2, sf.T2, sf.P1))
    for isc in (0, 1):
        i = lambda e, f: e.isc == isc
        # 3X3W6
        pp = lambda e, f: w6(e, f) and i(e, f) and not f['two_image'] and not f['pair16']
        q = lambda e, f: w6(e, f) and i(e, f) and f['two_image']
        assert some(lambda e, f: pp(e, f) and f['ntiles'] == 1) and some(lambda e, f: pp(e, f) and f['ntiles'] > 1 and f['ntiles'] % 8)
        assert {e.shape[2] for e in some(pp)} >= {64, 192} and {e.shape[1] for e in some(pp)} >= {32, 160} and {e.shape[1] for e in some(q)} >= {32, 160}
        assert some(lambda e, f: w6(e, f) and i(e, f) and f['pair16'] and e.shape[0] % 2 == 0 and e.shape[4] == 16)
        assert some(lambda e, f: q(e, f) and f['lists'] == 0 and f['tpb'] == 1 and dict(e.hooks).get('wino6_tiles_per_block') == 1)
        assert {f['tpb'] for e, f in ((e, ans[e]) for e in some(q)) if f['lists']} >= {2, 3, 4}
        assert some(lambda e, f: q(e, f) and f['lists'] and f['idle'] > 0), 'XCDs with unequal run counts'
        assert some(lambda e, f: q(e, f) and f['lists'] and (f['ntiles'] // 8) % f['tpb']), 'a run that ends short'
        assert some(lambda e, f: q(e, f) and dict(e.hooks).get('wino6_tiles_per_block') == 0 and f['tpb'] == 1)
        assert some(lambda e, f: w6(e, f) and i(e, f) and e.shape[3:] == (8, 32)) and some(lambda e, f: w6(e, f) and i(e, f) and e.shape[3] >= 24 and e.shape[4] >= 96)
        for form in (pp, q):
            assert {(e.act, e.epi) for e in some(form)} >= {(0, 'none'), (3, 'none'), (4, 'none'), (0, 'res'), (3, 'both')}
            assert {e.adj for e in some(form)} == {0, 1}
        # S2S6
        for two in (0, 1):
            k = lambda e, f: s2(e, f) and i(e, f) and f['two_image'] == two
            assert some(lambda e, f: k(e, f) and f['ntiles'] == 1) and some(lambda e, f: k(e, f) and f['ntiles'] > 1 and f['ntiles'] % 8)
            assert {e.shape[1] for e in some(k)} >= {32, 48, 160} and {e.adj for e in some(k)} == {0, 1}
            assert {e.epi for e in some(k)} >= {'none', 'res', 'both'}
        assert {e.shape[2] for e in some(lambda e, f: s2(e, f) and i(e, f))} >= {64, 128, 192}
        # T2S6
        for two, ct, scr in itertools.product((0, 1), (2, 4), (0, 1)):
            assert some(lambda e, f: t2(e, f) and i(e, f) and (f['two_image'], f['edge_ct'], f['scratch']) == (two, ct, scr)), (isc, two, ct, scr)
        k = lambda e, f: t2(e, f) and i(e, f)
        assert {e.shape[1] for e in some(k)} >= {32, 48, 96} and {e.act for e in some(k)} == {0, 3, 4} and {e.adj for e in some(k)} == {0, 1}
        assert min(e.shape[3] * e.shape[4] for e in some(lambda e, f: k(e, f) and f['edge_ct'] == 4)) == 64 * 64
    assert some(lambda e, f: w6(e, f) and dict(e.hooks).get('wino6_tiles_per_block') is None and not e.hooks and f['two_image'] and f['tpb'] > 1), 'automatic runs'
    # 1X1S6
    tps = lambda e: e.shape[3] * e.shape[4] // 256
    assert {tps(e) == 1 for e in some(p1)} == {True, False} and {e.shape[2] for e in some(p1)} >= {128, 256} and {e.shape[1] for e in some(p1)} >= {64, 192, 128}
    assert {e.epi for e in some(p1)} == {'none', 'res'} and {e.adj for e in some(p1)} == {0, 1}
    assert some(lambda e, f: p1(e, f) and e.shape == (8, 64, 512, 32, 32) and f['blocks'] == 128) and some(lambda e, f: p1(e, f) and f['idle'])
    # the weight gradients
    G = sf.WG
    assert {e.key[1] for e in G} == set(_lib.WGRAD6_FORMS[1:])
    for form in _lib.WGRAD6_FORMS[1:]:
        mine = [e for e in G if e.key[1] == form]
        assert any(e.S == 1 for e in mine)
        if form not in ('t2masked',):
            assert any(e.H == 1 or form == 'w6pair' for e in mine) and any(e.H % 2 == 1 and e.H > 1 for e in mine), form
    for form in ('w6', 't2wide', 't2narrow', 'p1'):
        mine = [e for e in G if e.key[1] == form]
        assert any(e.NB > 1 for e in mine) and any(e.S > 1 and (e.NB * e.W // sf.WG_COLS[e.kind]) % e.S for e in mine), form
        blocks = {(-(-e.Co // (128 if form == 'p1' else 64)), -(-e.Ci // (128 if form in ('p1', 't2wide') else 64))) for e in mine}
        assert (1, 1) in blocks and any(max(b) >= 2 for b in blocks), form
    assert {e.B for e in G if e.key[1] == 'w6pair'} == {2, 6}
    assert {(e.Co % 64, e.Ci % 64) for e in G if e.key[1] == 't2masked'} >= {(32, 0), (0, 32)}


@pytest.fixture(scope='module')
def sweep():
    """{key: first grid point} of te_conv_split_form over host_plans' batches, channels and sizes, every value of the form hooks, the
    tile walk off / automatic / 2 / 3, with and without style scales and scratch; and of te_wgrad6_form under both values of its hook"""
    L = _lib.lib()
    buf = (C.c_int * len(_lib.CONV_SPLIT_FORM))()
    found, n = {}, 0
    with sf.hooks({}):
        for kind in (sf.W6, sf.S2, sf.T2, sf.P1):
            forms = (1, 2, 3) if kind == sf.W6 else ((0, 1, 2) if kind in sf.FORM_HOOK else (None,))
            for form, tpb in itertools.product(forms, (0, 1, 2, 3) if kind == sf.W6 else (None,)):
                if form is not None:
                    sf.HOOKS[sf.FORM_HOOK[kind]](form)
                if tpb is not None:
                    _lib.wino6_tiles_per_block(tpb)
                for B, Kc, M, (H, W), isc, scr in itertools.product(hp.BATCHES, hp.CHANNELS, hp.CHANNELS, hp.SIZES, (0, 1) if kind != sf.P1 else (0,),
                                                                   (0, 1) if kind == sf.T2 else (0,)):
                    rc = L.te_conv_split_form(sf.KIND[kind], B, Kc, M, H, W, isc, scr, buf)
                    n += 1
                    if rc:
                        assert rc == -3
                        continue
                    f = dict(zip(_lib.CONV_SPLIT_FORM, buf))
                    found.setdefault(sf.fwd_key(kind, f), (B, Kc, M, H, W, form, tpb))
        for wide, (kname, kind), B, (Co, Ci), (H, W), NB in itertools.product((0, 1), sf.WG_KIND.items(), hp.BATCHES, hp.WGRAD_CHANNELS, hp.SIZES, (1, 2)):
            _lib.wgrad_split(1)
            _lib.wgrad_t2_wide(wide)
            name = _lib.wgrad6_form(kind, B, Co, Ci, H, W, NB)
            n += 1
            if name != 'fp32':
                found.setdefault((kname, name), (B, Co, Ci, H, W, NB, wide))
    return found, n


def test_table_has_every_key_the_sweep_finds(sweep):
    found, n = sweep
    assert n > 100000
    have = {e.key for e in sf.TABLE}
    missing = {k: v for k, v in found.items() if k not in have}
    assert not missing, f'{len(missing)} keys without an entry: ' + '; '.join(f'{k} at {v}' for k, v in sorted(missing.items(), key=str))
    assert have == set(found), sorted(have - set(found), key=str)


def test_query_refuses_what_the_launch_refuses():
    """the query and te_conv_res_f32 answer bad arguments with the same code; a refusal leaves the output untouched.  The launch is
    called on stand-in pointers, so ONLY with arguments that the query has just refused: its planning half, the same code, refuses
    before anything touches a device.  (A shape that a kind takes is never launched here: with a GPU present that would be a real
    launch on host addresses.)"""
    L = _lib.lib()
    n = len(_lib.CONV_SPLIT_FORM)
    buf = (C.c_int * n)(*([-7] * n))
    stand_in = (C.c_float * 8)()
    x = C.addressof(stand_in)

    def both(kind, a, want):
        rc = L.te_conv_split_form(kind, *a, 0, 0, buf)
        assert rc == want and rc < 0 and list(buf) == [-7] * n, (kind, a, rc)
        assert L.te_conv_res_f32(x, None, x, x, None, None, None, None, None, 1.0, 0, kind, *a, None) == rc, (kind, a)

    supported = {sf.KIND[sf.W6]: _lib.wino6_ok, sf.KIND[sf.S2]: _lib.s2s6_ok, sf.KIND[sf.T2]: _lib.t2s6_ok, sf.KIND[sf.P1]: _lib.p1s6_ok}
    for kind in sf.KIND.values():
        for a in ((0, 32, 64, 8, 32), (1, 0, 64, 8, 32), (1, 32, -64, 8, 32), (1, 32, 64, 0, 32), (1, 32, 64, 8, 0)):
            both(kind, a, -2)
        refused = 0
        for a in ((1, 24, 64, 8, 32), (1, 32, 96, 8, 32), (1, 32, 128, 9, 32), (1, 64, 128, 8, 24), (1, 16, 128, 8, 32), (1, 64, 32, 8, 32)):
            if not supported[kind](*a):
                both(kind, a, -3)
                refused += 1
        assert refused >= 4, kind
        assert L.te_conv_split_form(kind, 1, 128, 128, 16, 32, 0, 0, None) == -1
    for kind in (_lib.CONV_3X3, _lib.CONV_T2, _lib.CONV_S2, _lib.CONV_1X1, _lib.CONV_3X3W):
        assert L.te_conv_split_form(kind, 8, 128, 128, 32, 32, 0, 0, buf) == -3
    assert L.te_conv_split_form(99, 8, 128, 128, 32, 32, 0, 0, buf) == -2 and L.te_conv_split_form(-1, 8, 128, 128, 32, 32, 0, 0, buf) == -2
    assert L.te_conv_split_form(sf.KIND[sf.P1], 8, 64, 512, 32, 32, 1, 0, buf) == -3               # 1X1S6 takes no style scales
    assert list(buf) == [-7] * n
    f = _lib.conv_split_form(_lib.CONV_T2S6, 1, 32, 64, 64, 64, True, False)
    assert (f['two_image'], f['edge_ct'], f['edge_line_tiles'], f['edge_blocks'], f['scratch'], f['isc'], f['ntiles'], f['idle']) == (0, 4, 3, 3, 0, 1, 32, 0)
    assert _lib.conv_split_form(_lib.CONV_3X3, 1, 32, 64, 8, 32) == -3


def test_query_follows_the_hooks():
    shape = (2, 32, 128, 8, 32)
    with sf.hooks({'wino6_form': 1}):
        assert _lib.conv_split_form(_lib.CONV_3X3W6, *shape)['two_image'] == 0
    with sf.hooks({'wino6_form': 2}):
        assert _lib.conv_split_form(_lib.CONV_3X3W6, *shape)['two_image'] == 0                     # 16 blocks: not every CU gets one
    for tpb, lists in ((1, 0), (2, 1), (0, 0)):
        with sf.hooks({'wino6_form': 3, 'wino6_tiles_per_block': tpb}):
            f = _lib.conv_split_form(_lib.CONV_3X3W6, *shape)
            assert (f['two_image'], f['lists'], f['mblocks']) == (1, lists, 1)
    for kind, hook in ((_lib.CONV_S2S6, 's2s6_form'), (_lib.CONV_T2S6, 't2s6_form')):
        for form, two in ((0, 0), (1, 0), (2, 1)):
            with sf.hooks({hook: form}):
                assert _lib.conv_split_form(kind, 2, 32, 128, 8, 16)['two_image'] == two, (hook, form)


# ------------------------------------------------------------------------------------------------ the references, alone
KINKED = [e for e in sf.FWD if e.act >= 3]


@pytest.mark.parametrize('entry', KINKED, ids=IDS)
def test_reference_leaves_out_at_most_half_the_cap(entry):
    """the fp64 reference alone, on the CPU: the share of the elements within their own bound of the kink"""
    with torch.no_grad():
        y, bound, keep = sf.reference(entry, sf.operands(entry))
    left = 1.0 - float(keep.double().mean())
    assert left <= KINK_CAP / 2, f'{entry.name}: {left:.2e} of the elements sit on the kink'
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())


def test_every_entry_without_activation_needs_no_kink():
    assert all(sf.reference(e, sf.operands(e))[2] is None for e in sf.FWD if e.act == 0 and e.name not in sf.LARGE and e.shape[0] * e.shape[2] <= 256)


@pytest.mark.parametrize('entry', sf.WG, ids=IDS)
def test_weight_gradient_reference_is_consistent(entry):
    """the chunks partition the cells, so the slabs of a group sum to torch's own weight gradient of the group's samples"""
    e = entry
    o = sf.operands(e)
    ref, bound = sf.wg_reference(e, o)
    nb = 1 if e.key[1] == 'w6pair' else e.NB
    taps = 1 if e.kind == sf.K1 else 9
    assert ref.shape == bound.shape == (e.B // nb, e.S, e.Co, e.Ci, taps)
    g, x = o['g'].double(), o['x'].double()
    for b0 in range(0, e.B, nb):
        gb, xb = g[b0:b0 + nb], x[b0:b0 + nb]
        if e.kind == sf.K3:
            want = torch.nn.grad.conv2d_weight(xb, (e.Co, e.Ci, 3, 3), gb, padding=1).reshape(e.Co, e.Ci, 9)
        elif e.kind == sf.KT:
            want = torch.nn.grad.conv2d_weight(gb, (e.Ci, e.Co, 3, 3), xb, stride=2).transpose(0, 1).reshape(e.Co, e.Ci, 9)
        else:
            want = torch.einsum('bohw,bihw->oi', gb, xb)[..., None]
        assert float((ref[b0 // nb].sum(0) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((bound[ref != 0] > 0).all()) and float(bound.max()) < 1e-2

"""The form table of the small dense kernel (tests/small_gemm_forms.py) against te_small_gemm_form, the library's own launch plan: every
entry lands on its declared key, the table has the cases it was written for, a sweep of the query finds no (entry point, key) pair and
no side of a threshold that the table lacks, and the fp64 reference of the GPU test keeps every leaky-ReLU entry off the kink.  No GPU:
the plan is host code."""
import ctypes as C
import dataclasses
import itertools

import pytest

import small_gemm_forms as sf
from transeditor_amd import _lib
from transeditor_amd.op import linear as oplin

IDS = lambda e: e.name
KS = (1, 16, 17, 64, 65, 256, 257, 511, 512, 513, 1024)          # both sides of every threshold of the NW rule
TILES2 = 512                                                      # 2 * kNumCU: K = 512 takes 8 waves from here on
NW_OF_K = {1: (1, 5, 8, 16), 2: (17, 18, 33, 64), 4: (65, 100, 256), 8: (257, 300, 511), 16: (513, 520, 1000, 1024)}
SINGLE = [e for e in sf.TABLE if e.ep == 'single']


def _tiles(e):
    return -(-e.I // 32) * -(-e.J // 32) * (1 if e.ep == 'single' else e.nz)


@pytest.mark.parametrize('entry', sf.TABLE, ids=IDS)
def test_entry_lands_on_its_key(entry):
    sf.check(entry)
    assert entry.ep in sf.EPS and entry.la in sf.LAYOUTS and entry.lb in sf.LAYOUTS and entry.act in (0, 1, 3)
    assert entry.name.startswith(f'{entry.ep}_nw{entry.key[0]}_a{entry.key[1]}b{entry.key[2]}_')
    if entry.act == 3:      # the recipe that keeps the pre-activations off the kink
        assert entry.bias and entry.beta == 1.0 and entry.alpha is None
    if entry.ep != 'single':
        assert not entry.rs, 'no row sums in the batched and split-K forms'
    if entry.ep in ('uniform', 'table'):
        assert not entry.pre and not entry.res
    if entry.name not in sf.LARGE:
        assert max(entry.I, entry.J) <= 100 and entry.K <= 8 * 1024, 'a small entry'


def _probe(ep, I, J, K, nz, la, lb, **kw):
    return sf.Entry('probe', ep, I, J, K, nz, la, lb, (), **kw)


@pytest.fixture(scope='module')
def sweep():
    """({(entry point, key): first grid point}, {(K, nw) of single launches at the threshold values of K}, number of answers) over shapes,
    the six layouts of A and of B (stride classes and the two alignments), and the z forms"""
    found, edges, n = {}, set(), 0

    def ask(p):
        nonlocal n
        ans = sf.answer(p)
        assert not isinstance(ans, int), (p, ans)
        n += 1
        found.setdefault((p.ep,) + ans[:3], p)
        return ans

    for (I, J), K, la, lb in itertools.product(((1, 1), (33, 65), (65, 33), (673, 705), (705, 705)), KS, sf.LAYOUTS, sf.LAYOUTS):
        ans = ask(_probe('single', I, J, K, 1, la, lb))
        edges.add((K, ans[0], ans[3] * ans[4] * ans[5] >= TILES2))
    for nz, K, la, lb, za_mode in itertools.product((1, 3, 16, 85, 86), KS, sf.LAYOUTS, sf.LAYOUTS, ('sep', 'odd', 'zero')):
        ask(_probe('uniform', 33, 65, K, nz, la, lb, za_mode=za_mode))
    for nz, K, la, lb, za_mode, odd in itertools.product((1, 3, 12, 13, 16), KS, sf.LAYOUTS, sf.LAYOUTS, ('sep', 'odd'), (-1, 0)):
        ask(_probe('table', 129, 225, K, nz, la, lb, za_mode=za_mode, tab_odd=odd))
    for S, Kc, (I, J), la, lb in itertools.product((1, 2, 3, 8), (8, 16, 24, 64, 72, 256, 264, 512, 520, 1024), ((5, 40), (225, 256), (256, 256)),
                                                   sf.LAYOUTS, sf.LAYOUTS):
        ask(_probe('splitk', I, J, S * Kc, S, la, lb))
    return found, edges, n


def test_table_has_every_key_the_sweep_finds(sweep):
    """a new form, or a form newly reachable from an entry point, fails here until the table gets an entry for it"""
    found, _, n = sweep
    assert n > 20000
    have = {(e.ep,) + e.key for e in sf.TABLE}
    missing = {k: v for k, v in found.items() if k not in have}
    assert not missing, f'{len(missing)} (entry point, nw, av, bv) without an entry: ' + '; '.join(f'{k} at {v}' for k, v in sorted(missing.items())[:8])
    assert len(found) == 80 and have == set(found)           # 4 entry points x 5 x 2 x 2


def test_table_has_both_sides_of_every_threshold(sweep):
    """what the sweep finds at the threshold values of K (and, at K = 512, on both sides of 2 * kNumCU tiles) has a single-launch entry
    with that K, that wave count and that side: a threshold that moves shows here as a pair the table lacks"""
    _, edges, _ = sweep
    have = {(e.K, e.key[0], _tiles(e) >= TILES2) for e in SINGLE}
    have_k = {p[:2] for p in have}                                  # (the tile count matters at K = 512 only)
    missing = sorted(p for p in edges if (p not in have if p[0] == 512 else p[:2] not in have_k))
    assert not missing, f'(K, nw, tiles >= {TILES2}) without a single-launch entry: {missing}'
    assert {(16, 1), (17, 2), (64, 2), (65, 4), (256, 4), (257, 8), (511, 8), (512, 8), (512, 16), (513, 16), (1024, 16)} == {p[:2] for p in edges if p[0] > 1}


def _some(pred, among=sf.TABLE):
    return [e for e in among if pred(e, sf.geom(e))]


def test_table_covers_what_it_was_written_for():
    # all 20 instantiations through te_small_gemm_f32, and through every other entry point
    for ep in sf.EPS:
        assert {e.key for e in sf.TABLE if e.ep == ep} == set(itertools.product((1, 2, 4, 8, 16), (0, 1), (0, 1))), ep
    # 8 waves two ways; the K = 512 one has the fewest tiles that do it: one tile row or column fewer is back at 16
    assert _some(lambda e, g: e.key[0] == 8 and 256 < e.K < 512, SINGLE)
    big = _some(lambda e, g: e.key[0] == 8 and e.K == 512, SINGLE)
    assert big and all(_tiles(e) >= TILES2 for e in big)
    for e in big:
        for less in (dataclasses.replace(e, I=e.I - 32), dataclasses.replace(e, J=e.J - 32)):
            assert sf.answer(less)[0] == 16 and _tiles(less) < TILES2
    # 16 waves three ways
    assert _some(lambda e, g: e.key[0] == 16 and e.K == 512 and _tiles(e) < 16, SINGLE)
    assert _some(lambda e, g: e.key[0] == 16 and e.K == 513, SINGLE) and _some(lambda e, g: e.key[0] == 16 and e.K == 1024, SINGLE)
    # K edges: each on a 16-byte form (with K % 4 != 0: rows at a stride >= K, % 4 == 0, for both operands) and on the scalar form
    for nw, Ks in NW_OF_K.items():
        for K in Ks:
            assert _some(lambda e, g: e.K == K and e.key == (nw, 1, 1) and g.sak == 1 and g.sbk == 1 and g.sai >= K and g.sbj >= K
                         and g.sai % 4 == 0 and g.sbj % 4 == 0, SINGLE), (nw, K)
            assert _some(lambda e, g: e.K == K and e.key == (nw, 0, 0), SINGLE), (nw, K)
    # tile edges
    for I, J in itertools.product((1, 31, 32, 33, 65), repeat=2):
        assert _some(lambda e, g: (e.I, e.J) == (I, J), SINGLE), (I, J)
    # layouts of A with a 16-byte B, of B with a 16-byte A
    want = {'dense': lambda s, k, off, K: (s, k, off) == (K, 1, 0), 'off4': lambda s, k, off, K: (s, k, off) == (K, 1, 1),
            'oddrow': lambda s, k, off, K: k == 1 and s % 4 != 0 and s > K and off == 0, 'padded': lambda s, k, off, K: k == 1 and s % 4 == 0 and s > K and off == 0,
            'every2': lambda s, k, off, K: k > 1 and s > 1}
    for lay, ok in want.items():
        assert _some(lambda e, g: ok(g.sai, g.sak, g.a_off, e.K) and e.la == lay and e.key[2] == 1, SINGLE), ('A', lay)
        assert _some(lambda e, g: ok(g.sbj, g.sbk, g.b_off, e.K) and e.lb == lay and e.key[1] == 1, SINGLE), ('B', lay)
    assert _some(lambda e, g: g.sak == e.I and g.sai == 1 and e.key[2] == 1, SINGLE) and _some(lambda e, g: g.sbk == e.J and g.sbj == 1 and e.key[1] == 1, SINGLE)
    for lay in ('dense', 'padded'):
        assert all(e.key[1] == 1 for e in sf.TABLE if e.la == lay and e.K % 4 == 0 and e.za_mode != 'odd')
    # an aligned twin for every 4-bytes-off entry (the GPU test compares their bits)
    for e in _some(lambda e, g: 'off4' in (e.la, e.lb)):
        twin = [t for t in sf.TABLE if (t.ep, t.I, t.J, t.K, t.key[0]) == (e.ep, e.I, e.J, e.K, e.key[0]) and 'off4' not in (t.la, t.lb)
                and t.la == e.la.replace('off4', 'dense') and t.lb == e.lb.replace('off4', 'dense')]
        assert twin, e.name
    # epilogue
    assert _some(lambda e, g: e.bias and e.beta != 1.0, SINGLE) and _some(lambda e, g: not e.bias, SINGLE)
    assert _some(lambda e, g: e.alpha not in (None, 1.0), SINGLE) and _some(lambda e, g: e.alpha == 1.0, SINGLE)
    for act, pre, res in itertools.product((0, 1, 3), (0, 1), (0, 1)):
        assert _some(lambda e, g: (e.act, e.pre, e.res) == (act, pre, res), SINGLE), (act, pre, res)
    for J in (1, 33, 65):
        assert _some(lambda e, g: e.rs not in (None, 1.0) and e.J == J and e.I % 32 != 0 and e.I > 32, SINGLE), J
    # batched
    for nz, ep in itertools.product((1, 3, 16), ('uniform', 'table')):
        for cl in ('dense', 'btd', 'bdt'):
            assert _some(lambda e, g: (e.ep, e.nz, e.cl) == (ep, nz, cl)), (ep, nz, cl)
    for e in _some(lambda e, g: e.ep == 'table'):
        g = sf.geom(e)
        assert len(g.b_tab) == e.nz and len(set(g.b_tab)) == e.nz
        assert (e.tab_odd >= 0) == any(t % 4 for t in g.b_tab) and sum(t % 4 != 0 for t in g.b_tab) <= 1
        if e.tab_odd >= 0:      # BV off by that one offset: the same entry without it has BV on
            assert e.key[2] == 0 and sf.answer(dataclasses.replace(e, tab_odd=-1))[2] == 1
    assert _some(lambda e, g: e.ep == 'table' and e.tab_odd >= 0 and e.nz == 16) and _some(lambda e, g: e.ep == 'table' and e.tab_odd < 0 and e.key[2] == 1)
    assert _some(lambda e, g: e.ep == 'table' and e.bias) and _some(lambda e, g: e.ep == 'table' and not e.bias)
    assert _some(lambda e, g: e.ep == 'uniform' and e.bias and g.zbias == e.J)
    odd = _some(lambda e, g: e.ep in ('uniform', 'table') and g.za % 4 != 0)
    assert odd and all(e.key[1] == 0 and sf.answer(dataclasses.replace(e, za_mode='sep'))[1] == 1 for e in odd)
    # split-K
    for S, Kc in itertools.product((1, 2, 3, 8), (8, 768, 1024)):
        assert _some(lambda e, g: e.ep == 'splitk' and e.nz == S and e.K == S * Kc and e.I % 32 and e.J % 32 and e.pre and e.bias and e.res and e.act in (1, 3)), (S, Kc)
    for act in (1, 3):
        assert _some(lambda e, g: e.ep == 'splitk' and e.act == act and e.pre and e.bias and e.res)
    assert _some(lambda e, g: (e.ep, e.I, e.K, e.J, e.nz) == ('splitk', 32, 8192, 512, 8)) and _some(lambda e, g: (e.ep, e.I, e.K, e.J, e.nz) == ('splitk', 5, 2304, 40, 3))
    assert all(n in sf.BY_NAME for n in sf.LARGE)


def test_query_refuses_what_the_launches_refuse():
    """bad arguments: the query and the launch answer with the same code (the launches check before they touch anything, so stand-in
    pointers do)"""
    L = _lib.lib()
    buf = (C.c_int * 6)(*([-7] * 6))
    tab = (C.c_int64 * 17)()
    x = C.addressof((C.c_float * 4)())
    form = lambda I, J, K, nz, b_tab=None, a16=0, b16=0, splitk=0, out=buf: L.te_small_gemm_form(I, J, K, nz, K, 1, 1, K, 0, 0, b_tab, a16, b16, splitk, out)
    single = lambda I, J, K: L.te_small_gemm_f32(x, None, x, x, None, None, None, 0.0, I, J, K, K, 1, 1, K, 1.0, 1.0, 0, None)
    batched = lambda I, J, K, nz, b_tab=None: L.te_small_gemm_batched_f32(x, x, x, None, nz, 0, 0, 0, 0, b_tab, None, I, J, K, K, 1, 1, K, J, 1, 1.0, 1.0, 0, None)
    splitk = lambda I, J, K, S: L.te_small_gemm_splitk_f32(x, None, x, S, x, x, None, None, I, J, K, K, 1, 1, K, 1.0, 1.0, 0, None)
    for I, J, K in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert form(I, J, K, 1) == single(I, J, K) == batched(I, J, K, 1) == splitk(I, J, K, 1) == -2, (I, J, K)
    assert form(4, 4, 4, 0) == batched(4, 4, 4, 0) == -2 and form(4, 4, 8, 0, splitk=1) == splitk(4, 4, 8, 0) == -2
    assert form(4, 4, 8, 17, tab) == batched(4, 4, 8, 17, tab) == -3 and b'16 table entries' in L.te_last_error_string()
    for K, S in ((24, 2), (100, 3), (8, 3), (4, 1)):
        assert form(4, 4, K, S, splitk=1) == splitk(4, 4, K, S) == -2, (K, S)
    assert form(4, 4, 16, 2, tab, splitk=1) == -3
    assert form(4, 4, 4, 1, out=None) == -1 and L.te_small_gemm_f32(None, None, x, x, None, None, None, 0.0, 4, 4, 4, 4, 1, 1, 4, 1.0, 1.0, 0, None) == -1
    for a16, b16 in ((-1, 0), (16, 0), (0, 16), (0, -4)):
        assert form(4, 4, 4, 1, a16=a16, b16=b16) == -2
    assert list(buf) == [-7] * 6                                       # a refusal leaves the output untouched
    assert form(4, 4, 4, 1) == 0 and list(buf) == [1, 1, 1, 1, 1, 1]
    assert _lib.small_gemm_form(4, 4, 0, 1, 4, 1, 1, 4) == -2 and _lib.small_gemm_form(33, 65, 1024, 1, 1024, 1, 1, 1024, b_mod16=4) == (16, 1, 0, 3, 2, 1)


@pytest.mark.parametrize('entry', [e for e in sf.TABLE if e.act == 3], ids=IDS)
def test_reference_stays_off_the_kink(entry):
    """the fp64 reference alone, on the CPU: elements whose pre-activation lies within its own bound of 0 are left out of the GPU
    comparison; at most KINK_CAP of an entry, none of an entry with fewer than 1000 outputs"""
    r = sf.reference(entry, sf.operands(entry), entry.key[0])
    left = sf.left_out(entry, r)
    assert sf.kink_ok(entry, r), f'{entry.name}: {left:.2e} of {r["pre"].numel()} outputs sit on the kink'


def test_ksplit_properties():
    """op/linear._ksplit for every K from 1025 to 65536: 0, or the smallest S with K % S == 0, (K / S) % 8 == 0 and K / S <= 1024; 0 only
    where no S <= 64 qualifies"""
    ok = lambda K, S: K % S == 0 and (K // S) % 8 == 0 and K // S <= oplin.MAX_K
    zeros = 0
    for K in range(1025, 65537):
        S = oplin._ksplit(K)
        if K % 8:
            assert S == 0, K
            zeros += 1
            continue
        first = next((s for s in range(1, 65) if ok(K, s)), 0)
        assert S == first, (K, S, first)
        zeros += S == 0
    assert oplin._ksplit(8192) == 8 and oplin._ksplit(2304) == 3 and oplin._ksplit(65536) == 64 and oplin._ksplit(1032) == 3 and zeros > 56000

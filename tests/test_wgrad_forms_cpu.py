"""The form table of the fp32 weight-gradient kernel (tests/wgrad_forms.py) against te_wgrad_form, the library's own launch plan: every
entry lands on its declared key and per-block facts, the table has the cases it was written for, a sweep of the query over the host-plan
grid finds no key (and no kstride under a key) that the table lacks, the query agrees with te_wgrad6_form and te_wgrad_pair_form and
refuses what the launch refuses, and the fp64 reference of the GPU test is consistent with itself.  No GPU: the plan is host code."""
import ctypes as C
import dataclasses
import itertools

import pytest
import torch

import host_plans as hp
import wgrad_forms as wf
from transeditor_amd import _lib

IDS = lambda e: e.name
K3, KT, K1 = wf.K3, wf.KT, wf.K1
KEYS = {K3: {wf.PV, wf.PS, wf.D4, wf.N2V, wf.N2}, KT: {wf.T4V, wf.D4, wf.N2V, wf.N2}, K1: {wf.P4V, wf.P4, wf.N2V, wf.N2}}
FORMS = {e: wf.answer(e) for e in wf.TABLE}           # (held to the declared keys by test_entry_lands_on_its_key)


def _nc(e):
    return FORMS[e]['TW'] * FORMS[e]['TH']


def _some(pred, among=wf.TABLE):
    return [e for e in among if pred(e, FORMS[e])]


@pytest.mark.parametrize('entry', wf.TABLE, ids=IDS)
def test_entry_lands_on_its_key(entry):
    e, f = entry, wf.check(entry)
    nwp, wino, vec, db = e.key[1:]
    assert e.name.startswith(f'{e.kind}_n{nwp}w{wino}v{vec}_') and e.off in (0, 4) and e.sw in (0, 1)
    assert len(e.trips) == e.S and sum(e.trips) == f['tiles_x'] * f['tiles_y'] * e.NB and len(e.ks) == f['grid_y'] * f['grid_z']
    assert db == int(e.kind != K1 and nwp == 4)
    # the cell tile by the rule of the table's docstring
    p2 = lambda n: 1 << (n - 1).bit_length()
    TW = max(2, min(32, p2(e.W)))
    assert (f['TW'], f['TH']) == (TW, max(1, min(p2(e.H), wf.NCELL[e.kind] // TW)))
    if e.name not in wf.LARGE:
        numel = e.B * max(e.Co * (2 * e.H + 1) * (2 * e.W + 1) if e.kind == KT else e.Co * e.H * e.W, e.Ci * e.H * e.W)
        assert 4 * numel < (1 << 20), 'a small entry: operands below a megabyte'


def test_names_and_large():
    assert len(wf.BY_NAME) == len(wf.TABLE) and len(wf.LARGE) <= 3 and all(n in wf.BY_NAME for n in wf.LARGE)
    assert {e.kind for e in wf.TABLE if e.name in wf.LARGE} == {K3, KT, K1}
    for e in wf.TABLE:
        if e.name in wf.LARGE:      # a full-size layer at batch 2 whose chunks hold several tiles, on the kernel's main form
            assert e.B == 2 and e.S == 4 and min(e.trips) >= 8 and e.key[3] == 1 and e.key[1] == 4


def test_table_covers_what_it_was_written_for():
    T = wf.TABLE
    # every key; each vec key also by an entry that the default routing takes
    assert {k: {e.key[1:] for e in T if e.kind == k} for k in KEYS} == KEYS
    for kind, keys in KEYS.items():
        for key in keys:
            if key[2]:
                assert _some(lambda e, f: e.kind == kind and e.key[1:] == key and e.sw == 1), (kind, key)
    # the smallest vec shapes
    assert _some(lambda e, f: e.kind == K3 and (e.H, e.W) == (2, 32) and f['vec']) and _some(lambda e, f: e.kind == K1 and (e.H, e.W) == (2, 32) and f['vec'])
    assert _some(lambda e, f: e.kind == KT and (e.H, e.W) == (1, 32) and f['vec'])
    # the switch is off exactly where the split kernel would take the aligned launch
    for e in T:
        with wf.switch(1):
            taken = _lib.wgrad6_form(wf.KIND[e.kind], e.B, e.Co, e.Ci, e.H, e.W, e.NB) != 'fp32'
        assert (e.sw == 0) == (taken and e.off == 0), e.name
    # direct form on the 4-wave tile of the 3x3 kind: NC = 2 only, 1x1 and 1x2 images
    d4 = _some(lambda e, f: e.kind == K3 and e.key[1:] == wf.D4)
    assert {(e.H, e.W) for e in d4} == {(1, 1), (1, 2)} and all(_nc(e) == 2 for e in d4)
    # trips of the tile loop: chunks of 0 .. 4 tiles with chunk boundaries inside a tile row, for a two-image and a single-image key of each kind
    for kind, db in ((K3, 1), (K3, 0), (KT, 1), (KT, 0), (K1, 0)):
        for vec in (0, 1):
            have = _some(lambda e, f: e.kind == kind and e.key[4] == db and e.key[3] == vec and f['tiles_x'] == 2 and e.NB == 1)
            assert {t for e in have for t in e.trips} >= {0, 1, 2, 3, 4}, (kind, db, vec)
            assert any(e.S > 1 and any(sum(e.trips[:s]) % 2 for s in range(1, e.S)) for e in have), (kind, db, vec)
    # k-step edges
    for kind in KEYS:
        assert _some(lambda e, f: e.kind == kind and _nc(e) == 2 and (e.H, e.W) == (1, 1))
    assert _some(lambda e, f: e.kind == K3 and _nc(e) == 4 and f['wino']) and _some(lambda e, f: e.kind == K3 and _nc(e) == 4 and f['nwp'] == 2)
    for H, W in ((3, 5), (9, 1)):
        for kind in (K3, K1):
            for nwp in (2, 4):
                assert _some(lambda e, f: (e.kind, e.H, e.W, f['nwp']) == (kind, H, W, nwp) and _nc(e) == 32 < wf.NCELL[kind]), (kind, H, W, nwp)
    assert _some(lambda e, f: e.kind == KT and (e.H, e.W) == (9, 1)) and _some(lambda e, f: e.kind == KT and (e.H, e.W) == (3, 5))
    for kind in (K3, K1):       # full NC, ragged tiles: vec off through H % TH alone, and a ragged last tile column
        assert _some(lambda e, f: e.kind == kind and (e.H, e.W) == (3, 32) and _nc(e) == 64 and not f['vec'] and e.off == 0)
    for kind in KEYS:
        assert _some(lambda e, f: e.kind == kind and e.W == 40 and f['tiles_x'] == 2 and not f['vec'])
        assert _some(lambda e, f: e.kind == kind and f['tiles_x'] == 2 and f['vec'])
    # the four K-split cases of the 2-wave tile and the channel tails inside them
    n2 = lambda kind, Co, Ci, k, vec=None: _some(lambda e, f: (e.kind, e.Co, e.Ci, e.ks) == (kind, Co, Ci, (k,)) and f['nwp'] == 2 and vec in (None, f['vec']))
    for (Co, Ci), k in (((64, 64), 1), ((32, 64), 2), ((64, 32), 2), ((32, 32), 4), ((48, 48), 1), ((33, 20), 2), ((8, 8), 4)):
        assert n2(K3, Co, Ci, k, 0) and n2(K3, Co, Ci, k, 1), (Co, Ci)
    for kind in (KT, K1):
        assert len({(e.Co, e.Ci) for e in _some(lambda e, f: e.kind == kind and f['nwp'] == 2 and e.ks[0] > 1)}) >= 2
        assert {e.ks[0] for e in _some(lambda e, f: e.kind == kind and f['nwp'] == 2)} == {1, 2, 4}
    assert n2(KT, 32, 64, 2) and n2(K3, 32, 64, 2)         # the roles swap: the one-block side is the shifted operand for T2, the plain one for 3x3
    for kind in KEYS:           # fewer k-steps than shares
        assert _some(lambda e, f: e.kind == kind and f['nwp'] == 2 and wf.facts(e, f)[2] < e.ks[0])
    assert _some(lambda e, f: (e.kind, e.Co, e.Ci, e.H, e.W) == (K3, 32, 32, 1, 1) and wf.facts(e, f)[2] == 1 and e.ks == (4,))
    # channel tails on the 4-wave tile, and grid y, z > 1
    for kind in KEYS:
        assert _some(lambda e, f: e.kind == kind and (e.Co, e.Ci) == (130, 66) and f['nwp'] == 4 and not f['vec'] and f['TW'] * f['TH'] > 2)
        assert _some(lambda e, f: e.kind == kind and (e.Co, e.Ci) == (96, 72) and f['vec'])
        assert _some(lambda e, f: e.kind == kind and f['grid_y'] > 1 and f['grid_z'] > 1 and e.Co % 128 == 0 and e.Ci % 128 == 0 and f['vec'])
    # groups
    for NB, S, vec in itertools.product((2, 4), (1, 2), (0, 1)):
        assert _some(lambda e, f: e.kind == K3 and (e.NB, e.S, f['vec']) == (NB, S, vec) and e.Co % 128 == 0 and e.Ci % 128 == 0), (NB, S, vec)
    for kind in KEYS:
        grp = _some(lambda e, f: e.kind == kind and e.NB > 1)
        assert {f['vec'] for f in map(FORMS.get, grp)} == {0, 1}
        tiles_1 = lambda e: FORMS[e]['tiles_x'] * FORMS[e]['tiles_y']
        cuts = lambda e: [sum(e.trips[:s]) for s in range(1, e.S)]
        assert any(c % tiles_1(e) == 0 for e in grp for c in cuts(e)), 'a chunk boundary between two samples'
        assert any(c % tiles_1(e) != 0 for e in grp for c in cuts(e)), 'a chunk boundary inside a sample'
    tails = _some(lambda e, f: e.NB > 1 and (e.Co % 128 or e.Ci % 128))
    assert all(f['vec'] and e.NB == 2 for e, f in ((e, FORMS[e]) for e in tails if e.Co % 64)) and _some(lambda e, f: e.NB == 2 and e.Co == 96 and f['vec'])
    # misalignment: a vec-eligible shape per kind, its key shows vec = 0, the aligned twin (switch off) is in the table with vec = 1, and
    # under the default switch a split kernel would have taken the aligned launch
    for kind in KEYS:
        off = _some(lambda e, f: e.kind == kind and e.off == 4)
        assert off and all(e.sw == 1 and e.key[3] == 0 for e in off)
        for e in off:
            twin = [t for t in wf.TABLE if t.off == 0 and dataclasses.replace(t, name='', key=(), off=4, sw=1) == dataclasses.replace(e, name='', key=())]
            assert len(twin) == 1 and twin[0].key[3] == 1 and twin[0].key[:3] == e.key[:3], e.name
        with wf.switch(1):
            assert any(_lib.wgrad_form(wf.KIND[e.kind], e.B, e.Co, e.Ci, e.H, e.W, e.S, e.NB)['form6'] != 0 for e in off), kind
    # S = 1 twins of the S > 1 trip entries, and batches of several samples with several chunks
    for e in _some(lambda e, f: e.name.endswith('_trips') and e.S == 3):
        assert _some(lambda t, f: (t.kind, t.B, t.Co, t.Ci, t.H, t.W, t.NB, t.S) == (e.kind, e.B, e.Co, e.Ci, e.H, e.W, 1, 1))
    for kind in KEYS:
        assert _some(lambda e, f: e.kind == kind and e.B > 2 and e.NB == 1 and e.S > 1 and max(e.trips) > 1)


def test_table_reaches_the_steady_state_of_both_tile_loops():
    """without `if (tl + 2 < t_end) issue(tl + 2)` only chunks of three or more tiles change: the table has them for the two-image branch
    and the single-image branch of every kind that has the branch (1x1: the single-image one only), on both staging paths"""
    for kind, db in ((K3, 1), (K3, 0), (KT, 1), (KT, 0), (K1, 0)):
        for vec in (0, 1):
            deep = _some(lambda e, f: e.kind == kind and f['db'] == db and f['vec'] == vec and max(wf.facts(e, f)[0]) >= 3)
            assert deep, (kind, db, vec)
            assert any(e.name not in wf.LARGE for e in deep)
    assert not _some(lambda e, f: e.kind == K1 and f['db'])


@pytest.fixture(scope='module')
def sweep():
    """({(kind, nwp, wino, vec, db): first grid point}, {(key, kstride of a 2-wave block)}, answers) over host_plans' batches, channels and sizes,
    both switch values, both alignments, S in {1, planner} and NB in {1, planner}; the answers are held to te_wgrad6_form, te_wgrad_pair_form
    and the zero rule on the way"""
    L = _lib.lib()
    buf = (C.c_int * len(_lib.WGRAD_FORM))()
    found, kfound, n = {}, set(), 0
    saved = L.te_wgrad_split_bf16(-1)
    try:
        for on, (kname, kind), B, (Co, Ci), (H, W) in itertools.product((0, 1), wf.KIND.items(), hp.BATCHES, hp.WGRAD_CHANNELS, hp.SIZES):
            L.te_wgrad_split_bf16(on)
            nb, sc = C.c_int(-1), C.c_int(-1)
            assert L.te_wgrad_group_plan(kind, B, Co, Ci, H, W, C.byref(nb), C.byref(sc)) == 0
            plans = {(1, 1), (L.te_wgrad_slab_count(kind, B, Co, Ci, H, W), 1), (1, nb.value), (sc.value, nb.value)}
            for (S, NB), off in itertools.product(sorted(plans), (0, 4)):
                assert L.te_wgrad_form(kind, B, Co, Ci, H, W, S, NB, off, off, buf) == 0, (kname, B, Co, Ci, H, W, S, NB)
                f = dict(zip(_lib.WGRAD_FORM, buf))
                n += 1
                where = (on, kname, B, Co, Ci, H, W, S, NB, off)
                assert f['form6'] == (0 if off else L.te_wgrad6_form(kind, B, Co, Ci, H, W, NB)), where
                if f['form6']:
                    assert not any(list(buf)[1:]), where
                    continue
                assert f['wino'] == L.te_wgrad_pair_form(kind, Co, Ci, H, W) and not (f['vec'] and off), where
                assert f['grid_x'] == B // NB * S and f['db'] == int(kname != K1 and f['nwp'] == 4), where
                key = (kname, f['nwp'], f['wino'], f['vec'], f['db'])
                found.setdefault(key, where)
                if f['nwp'] == 2:
                    assert f['grid_y'] == f['grid_z'] == 1
                    probe = wf.Entry('probe', kname, B, Co, Ci, H, W, S, NB, on, off, key, (), ())
                    kfound.add((key, wf.facts(probe, f)[1][0]))
    finally:
        L.te_wgrad_split_bf16(saved)
    return found, kfound, n


def test_table_has_every_key_the_sweep_finds(sweep):
    """a new instantiation, or a changed pick_nwp / pair_form_3x3 / vec rule, fails here (or in test_entry_lands_on_its_key, entry named)"""
    found, kfound, n = sweep
    assert n > 80000
    have = {e.key for e in wf.TABLE}
    missing = {k: v for k, v in found.items() if k not in have}
    assert not missing, f'{len(missing)} keys without an entry: ' + '; '.join(f'{k} at {v}' for k, v in sorted(missing.items()))
    assert len(found) == 13 and have == set(found)
    khave = {(e.key, k) for e in wf.TABLE if e.key[1] == 2 for k in e.ks}
    assert not kfound - khave, f'(key, kstride) without an entry: {sorted(kfound - khave)}'


def test_query_refuses_what_the_launch_refuses():
    """bad arguments: the query and the launches answer with the same code (the launches plan before they touch anything, so stand-in
    pointers do); a refusal leaves the output untouched.  (No image is too large for a cell tile: the tile is clamped to the stage.)"""
    L = _lib.lib()
    n = len(_lib.WGRAD_FORM)
    buf = (C.c_int * n)(*([-7] * n))
    x = C.addressof((C.c_float * 8)())
    k3 = _lib.CONV_3X3
    form = lambda kind, B, Co, Ci, H, W, S, NB=1, g16=0, x16=0, out=buf: L.te_wgrad_form(kind, B, Co, Ci, H, W, S, NB, g16, x16, out)
    one = lambda kind, B, Co, Ci, H, W, S: L.te_wgrad_f32(x, x, x, kind, B, Co, Ci, H, W, S, None)
    grp = lambda kind, B, Co, Ci, H, W, S, NB: L.te_wgrad_group_f32(x, x, x, kind, B, Co, Ci, H, W, S, NB, None)
    for on in (0, 1):
        with wf.switch(on):
            for a in ((0, 8, 8, 4, 4, 1), (2, 0, 8, 4, 4, 1), (2, 8, -1, 4, 4, 1), (2, 8, 8, 0, 4, 1), (2, 8, 8, 4, 0, 1), (2, 8, 8, 4, 4, 0)):
                assert form(k3, *a) == one(k3, *a) == grp(k3, *a, 1) == -2, a
            for NB in (0, -1, 3, 8):                                          # a group size that does not divide the batch
                assert form(k3, 4, 8, 8, 4, 4, 1, NB) == grp(k3, 4, 8, 8, 4, 4, 1, NB) == -2, NB
            big = (65536, 8, 8, 4, 4, 32768)                                  # B * S > 2^31 - 1
            assert form(k3, *big) == one(k3, *big) == -2 and b'grid too large' in L.te_last_error_string()
            wide = (1, 64 * 65535 + 1, 8, 1, 1, 1)                            # more than 65535 channel blocks
            assert form(k3, *wide) == one(k3, *wide) == -2
            for kind in wf.KIND.values():                                     # a sample, and a group of four, of 2 GiB
                huge = (1, 513, 3, 1024, 1024, 1)
                assert form(kind, *huge) == one(kind, *huge) == -3 and b'2 GiB' in L.te_last_error_string()
                g4 = (4, 128, 128, 1024, 1024, 1, 4)
                assert form(kind, *g4) == grp(kind, *g4) == -3
                assert isinstance(_lib.wgrad_form(kind, 4, 128, 128, 256, 1024, 1, 2), dict)
            assert form(99, 2, 8, 8, 4, 4, 1) == one(99, 2, 8, 8, 4, 4, 1) == -3
            assert form(k3, 2, 8, 8, 4, 4, 1, out=None) == -1 and L.te_wgrad_f32(None, x, x, k3, 2, 8, 8, 4, 4, 1, None) == -1
            for g16, x16 in ((-1, 0), (16, 0), (0, 16), (0, -4)):
                assert form(k3, 2, 8, 8, 4, 4, 1, 1, g16, x16) == -2
    assert list(buf) == [-7] * n
    assert form(k3, 2, 8, 8, 4, 4, 3) == 0 and list(buf)[:12] == [0, 2, 0, 0, 0, 4, 4, 1, 1, 6, 1, 1]
    assert _lib.wgrad_form(k3, 2, 8, 8, 0, 4, 1) == -2 and _lib.wgrad_form(k3, 1, 128, 64, 2, 32, 1, g_mod16=4)['vec'] == 0


def test_query_follows_the_switch_and_the_alignment():
    """a split-eligible shape: form6 names the split kernel only under the switch and with both operands aligned; else this kernel's plan"""
    k3 = _lib.CONV_3X3
    with wf.switch(1):
        f = _lib.wgrad_form(k3, 2, 128, 64, 2, 32, 1)
        assert f['form6'] == _lib.WGRAD6_FORMS.index('w6') and not any(v for k, v in f.items() if k != 'form6')
        for g16, x16 in ((4, 0), (0, 8), (12, 4)):
            f = _lib.wgrad_form(k3, 2, 128, 64, 2, 32, 1, 1, g16, x16)
            assert (f['form6'], f['nwp'], f['wino'], f['vec'], f['db']) == (0, 4, 1, 0, 1)
    with wf.switch(0):
        f = _lib.wgrad_form(k3, 2, 128, 64, 2, 32, 1)
        assert (f['form6'], f['nwp'], f['wino'], f['vec'], f['db'], f['TW'], f['TH']) == (0, 4, 1, 1, 1, 32, 2)
        assert f['lds'] == 2 * 4 * (128 * 65 + 64 * (4 * 34 | 1))


SMALL = [e for e in wf.TABLE if e.name.endswith(('_key', '_group', '_grouptail', '_tail')) or (e.name.endswith('_trips') and e.S == 3)]


@pytest.mark.parametrize('entry', SMALL, ids=IDS)
def test_reference_is_consistent(entry):
    """the fp64 reference alone, on the CPU: the chunks partition the cells, so the slabs of a group sum to torch's own weight gradient of
    the group's samples; the bound is positive wherever the reference is nonzero and an empty chunk has reference and bound 0"""
    e, f = entry, FORMS[entry]
    g, x = wf.operands(e)
    ref, bound = wf.reference(e, f, g, x)
    taps = 1 if e.kind == K1 else 9
    assert ref.shape == bound.shape == (e.B // e.NB, e.S, e.Co, e.Ci, taps)
    gd, xd = g.double(), x.double()
    if e.kind == K3:
        per = torch.stack([torch.nn.grad.conv2d_weight(xd[b:b + 1], (e.Co, e.Ci, 3, 3), gd[b:b + 1], padding=1).reshape(e.Co, e.Ci, 9) for b in range(e.B)])
    elif e.kind == KT:
        per = torch.stack([torch.nn.grad.conv2d_weight(gd[b:b + 1], (e.Ci, e.Co, 3, 3), xd[b:b + 1], stride=2).transpose(0, 1).reshape(e.Co, e.Ci, 9)
                           for b in range(e.B)])
    else:
        per = torch.einsum('bohw,bihw->boi', gd, xd)[..., None]
    want = per.view(e.B // e.NB, e.NB, e.Co, e.Ci, taps).sum(1)
    assert float((ref.sum(1) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((bound >= 0).all()) and bool((bound[ref != 0] > 0).all())
    for s, t in enumerate(e.trips):
        if t == 0:
            assert not bool(ref[:, s].any()) and not bool(bound[:, s].any())
    # the bound is a rounding bound: below 1e-4 of the magnitude sum it multiplies, far above fp64 noise
    assert float(bound.max()) < 1e-2

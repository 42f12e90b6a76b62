"""The form table of the fp32 direct convolution kernel (tests/conv_forms.py) against te_conv_form, the library's own launch plan:
every entry lands on its declared form, the table has the cases it was written for, and a sweep of the query finds no form that
the table lacks.  No GPU: the plan is host code."""
import ctypes as C
import itertools

import pytest

import conv_forms as cf
import host_plans as hp
from transeditor_amd import _lib

IDS = lambda e: e.name
SWEEP_SIZES = hp.SIZES + ((4, 3), (9, 3), (4, 5), (9, 5), (33, 3), (33, 5))


@pytest.mark.parametrize('entry', cf.TABLE, ids=IDS)
def test_entry_lands_on_its_form(entry):
    ans = cf.check(entry)
    B, K, M, H, W = entry.shape
    S = _lib.lib().te_conv_splitk_count(cf.KINDS[entry.kind], B, K, M, H, W)
    assert ans['ksplit'] == (S if entry.with_ws else 1)
    if S > 1:        # the same shape without workspace is not split, and with one it is
        assert cf.answer(entry.kind, entry.shape, entry.has_isc, entry.epi, 0)['ksplit'] == 1
        assert cf.answer(entry.kind, entry.shape, entry.has_isc, entry.epi, 1)['ksplit'] == S
    assert entry.name.startswith(cf.form_name(entry.kind, entry.has_isc, entry.epi, entry.form))
    assert entry.epi in cf.EPIS and entry.act in (0, 3, 4)


@pytest.fixture(scope='module')
def sweep():
    """{form key: first grid point} and the number of answers over BATCHES x CHANNELS x CHANNELS x SIZES of tests/host_plans.py plus widths 3
    and 5, both has_isc, with and without workspace, with and without an epilogue where the launch has one; ksplit is compared with
    te_conv_splitk_count on the way"""
    L = _lib.lib()
    found, n = {}, 0
    for kind, B, K, M, (H, W), isc, ws, epi in itertools.product(cf.KINDS, hp.BATCHES, hp.CHANNELS, hp.CHANNELS, SWEEP_SIZES, (0, 1), (0, 1), ('none', 'res')):
        ans = cf.answer(kind, (B, K, M, H, W), isc, epi, ws)
        refused = epi != 'none' and (isc or kind in ('S2', 'T2'))
        assert isinstance(ans, int) == bool(refused), (kind, B, K, M, H, W, isc, epi, ans)
        if refused:
            assert ans == -3
            continue
        n += 1
        S = L.te_conv_splitk_count(cf.KINDS[kind], B, K, M, H, W)
        assert ans['ksplit'] == (S if ws else 1), (kind, B, K, M, H, W, ans['ksplit'], S)
        found.setdefault(cf.key_of(kind, isc, epi, cf.form_of(ans)), (kind, (B, K, M, H, W), isc, epi, ws))
    return found, n


def test_table_has_every_form_the_sweep_finds(sweep):
    """a new form, or a threshold that moved, fails here until the table gets an entry for it"""
    found, n = sweep
    assert n > 100000
    have = {cf.key(e) for e in cf.TABLE}
    missing = {k: v for k, v in found.items() if k not in have}
    assert not missing, f'{len(missing)} forms without an entry, (kind, isc, epi) + {cf.FORM_FIELDS}: ' + '; '.join(
        f'{k} at {v}' for k, v in sorted(missing.items(), key=str)[:8])
    # and the table has no key of its own making: an entry's key is what the query says (test_entry_lands_on_its_form), so
    # every key is reachable; the ones beyond the sweep's grid are the shapes chosen for one rule (W = 2, the 8192 x 2 image, ...)
    assert len(have) >= len(found)


def _entries(pred):
    return [e for e in cf.TABLE if pred(dict(zip(cf.FORM_FIELDS, e.form)), e)]


def test_table_covers_what_it_was_written_for():
    """the list of the table's docstring, entry by entry of the list"""
    tcs = {'3X3': (0, 1, 2), 'S2': (0, 1, 2), 'T2': (0, 1, 2), '1X1': (0, 1, 2, 3)}
    for kind, classes in tcs.items():
        for tc in classes:
            here = lambda f, e: e.kind == kind and f['tc'] == tc
            fast = kind != '1X1' or tc == 3
            if fast:
                for isc in (0, 1):
                    assert _entries(lambda f, e: here(f, e) and f['fast'] and e.has_isc == isc), (kind, tc, 'fast', isc)
            if tc == 3:
                continue
            single = lambda f, e: here(f, e) and not f['fast'] and not f['multi']
            assert _entries(lambda f, e: single(f, e) and e.shape[1] == 12), (kind, tc, 'K = 12')
            if tc == (1 if kind == 'T2' else 0):
                assert _entries(lambda f, e: single(f, e) and e.shape[1] == 24), (kind, tc, 'K = 24')
            if (kind, tc) == ('T2', 0):
                continue                         # never multi-sample, never split (see the table's docstring)
            assert _entries(lambda f, e: here(f, e) and f['multi'] and f['ms'] and e.has_isc), (kind, tc, 'template MS')
            assert _entries(lambda f, e: here(f, e) and f['multi'] and not f['ms'] and not e.has_isc), (kind, tc, 'run-time multi-sample')
            assert _entries(lambda f, e: here(f, e) and f['split'] and not f['fast']), (kind, tc, 'general split')
            if fast:
                assert _entries(lambda f, e: here(f, e) and f['split'] and f['fast']), (kind, tc, 'FAST split')
                assert _entries(lambda f, e: here(f, e) and f['fast'] and f['th_cut']), (kind, tc, 'TH halved in FAST')
        if kind != '1X1':                        # (a 1x1 input tile is as large as its cells: it always fits the budget)
            assert _entries(lambda f, e: e.kind == kind and f['multi'] and f['nsv_cut']), (kind, 'NSv < NS')
        assert _entries(lambda f, e: e.kind == kind and e.shape[3:] == (1, 1)), (kind, '1 x 1 image')
    for e in cf.TABLE:
        if e.with_ws == 0:
            assert e.expect.get('ksplit') == 1 and _lib.lib().te_conv_splitk_count(cf.KINDS[e.kind], *e.shape) > 1, e.name
    assert len([e for e in cf.TABLE if e.with_ws == 0]) >= 4
    # tile-count edges of the banded mapping, both M block counts
    for nbody in (1, 7, 8, 9):
        assert _entries(lambda f, e: e.expect.get('nbody') == nbody and e.expect.get('mblocks') == 1)
    for nbody in (7, 9):
        assert _entries(lambda f, e: e.expect.get('nbody') == nbody and e.expect.get('mblocks') == 2 and e.shape[2] == 129)
    # geometry: partial tiles, odd width in FAST, W = 3, TW < 4
    assert _entries(lambda f, e: f['fast'] and e.shape[4] % 2 == 1 and e.shape[4] > 4)
    assert _entries(lambda f, e: e.shape[4] == 3) and _entries(lambda f, e: e.expect.get('r0_TW') == 2 and not f['fast'])
    assert _entries(lambda f, e: e.expect.get('r0_tiles_x') == 2) and _entries(lambda f, e: e.expect.get('r0_tiles_y') == 2)
    # T2 regions
    t2 = lambda f, e: e.kind == 'T2'
    assert _entries(lambda f, e: t2(f, e) and f['nreg'] == 1 and max(e.shape[3:]) + 1 <= 8)
    assert _entries(lambda f, e: t2(f, e) and f['nreg'] == 1 and e.shape[3] + 1 <= 8 < e.shape[4] + 1)
    assert _entries(lambda f, e: t2(f, e) and f['nreg'] == 1 and e.shape[4] + 1 <= 8 < e.shape[3] + 1)
    assert _entries(lambda f, e: t2(f, e) and f['nreg'] == 3 and e.expect.get('nbody') == 8)
    assert _entries(lambda f, e: t2(f, e) and f['nreg'] == 3 and e.expect.get('nbody') == 9)
    assert _entries(lambda f, e: t2(f, e) and f['tc'] == 1 and e.shape[2] >= 96)
    big = _entries(lambda f, e: t2(f, e) and f['tc'] == 0)
    assert len(big) == 4 and all(e.act == 0 for e in big)
    assert _entries(lambda f, e: t2(f, e) and not f['fast'] and e.expect.get('r1_TH', 0) < e.expect.get('r1_TH0', 0))
    # 1x1: the deep-stage class and its fallback
    assert _entries(lambda f, e: e.kind == '1X1' and f['tc'] == 3 and f['fast'])
    assert _entries(lambda f, e: e.kind == '1X1' and f['tc'] == 0 and not f['fast'] and e.shape[1] % 64 == 0 and e.expect.get('ksplit') == 1 and e.expect.get('r0_TW') == 2)
    # EPI: res, mask and both, FAST and general, single- and multi-sample, for both kinds that have it
    for kind in ('3X3', '1X1'):
        for epi in cf.EPIS[1:]:
            assert _entries(lambda f, e: e.kind == kind and e.epi == epi and f['fast']), (kind, epi, 'fast')
            assert _entries(lambda f, e: e.kind == kind and e.epi == epi and not f['fast'] and not f['multi']), (kind, epi, 'general')
            assert _entries(lambda f, e: e.kind == kind and e.epi == epi and f['multi'] and f['ms']), (kind, epi, 'multi-sample')
    # everything but the large entries stays far below a megabyte of operands
    for e in cf.TABLE:
        B, K, M, H, W = e.shape
        if e not in big and K * H * W < 2 ** 18:
            cin, cout = ((2 * H + 1) * (2 * W + 1) if e.kind == k else H * W for k in ('S2', 'T2'))
            assert (B * K * cin + B * M * cout + 9 * K * M) * 4 < 2 ** 20, e.name
    assert all(n in cf.BY_NAME for n in cf.DGRAD) and {cf.BY_NAME[n].kind for n in cf.DGRAD} == set(cf.KINDS)


def test_query_refuses_what_the_launch_refuses():
    L = _lib.lib()
    buf = (C.c_int * 35)(*([-7] * 35))
    for kind, shape, isc, epi in cf.REFUSED:
        assert cf.answer(kind, shape, isc, epi) == -3, (kind, shape, isc, epi)
    assert L.te_conv_form(0, 2, 16, 96, 9, 5, 1, 1, 1, buf) == -3 and b'unmodulated' in L.te_last_error_string()
    assert L.te_conv_form(0, 2, 16, 96, 9, 5, 0, 0, 1, None) == -1
    for bad in ((0, 0, 16, 96, 9, 5, 0, 0, 1), (0, 2, 0, 96, 9, 5, 0, 0, 1), (0, 2, 16, 96, 9, -1, 0, 0, 1), (-1, 2, 16, 96, 9, 5, 0, 0, 1),
                (9, 2, 16, 96, 9, 5, 0, 0, 1), (0, 2, 16, 96, 9, 5, 0, 4, 1), (0, 2, 16, 96, 9, 5, 0, -1, 1)):
        assert L.te_conv_form(*bad, buf) == -2, bad
    for kind in (_lib.CONV_3X3W, _lib.CONV_3X3W6, _lib.CONV_S2S6, _lib.CONV_T2S6, _lib.CONV_1X1S6):
        assert L.te_conv_form(kind, 2, 64, 128, 32, 32, 0, 0, 1, buf) == -3
    assert list(buf) == [-7] * 35                                      # a refusal leaves the output untouched
    assert L.te_conv_form(0, 2, 16, 96, 9, 5, 0, 0, 1, buf) == 0 and buf[0] == 0 and list(buf)[11 + 8:] == [0] * 16     # zeros past nreg

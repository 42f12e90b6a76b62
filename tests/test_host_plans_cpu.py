"""The host launch planners still give the recorded table (tests/host_plans.py), answer for answer.  No GPU: the planners are host code."""
import numpy as np
import pytest

import host_plans as hp
from transeditor_amd import _lib


@pytest.fixture(scope='module')
def tables():
    """(golden, current); the sweep flips te_wgrad_split_bf16 and has to leave it as it found it"""
    L = _lib.lib()
    before = L.te_wgrad_split_bf16(-1)
    current = hp.table(L)
    assert L.te_wgrad_split_bf16(-1) == before
    return dict(np.load(hp.GOLDEN)), current


def test_host_plans_match_golden(tables):
    golden, current = tables
    assert hp.answers(golden) == hp.answers(current) > 200000
    diff = hp.differences(golden, current)
    assert not diff, 'planner answers changed: ' + '; '.join(
        f'{name} rows {rows[:5].tolist()} ({len(rows)} rows): {golden[name][rows[0]].tolist()} -> {current[name][rows[0]].tolist()}'
        for name, rows in diff.items())


def test_refused_plans_stay_refused(tables):
    """the one permitted difference is the CODE of a refusal by the three FIR plans: the golden table does hold such rows, the same
    rows are refused now, and a refusal leaves the outputs untouched"""
    golden, current = tables
    for name in hp.REFUSAL_CODE_FREE:
        g, c = golden[name], current[name]
        assert (g[:, 0] < 0).any() and (g[:, 0] == 0).any()
        assert np.array_equal(g[:, 0] < 0, c[:, 0] < 0)
        assert (c[c[:, 0] < 0, 1:] == -1).all()

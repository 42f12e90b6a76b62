"""The route table of tests/conv_routes.py against the host-side predicates and planners (no GPU needed): every entry lands on the
routes it declares, and the table covers every route the selectors can take.  A predicate change that moves a shape to another
kernel, or a new route, fails here first, with the entry's name."""
import pytest

import conv_routes as cr


@pytest.mark.parametrize('route', cr.ROUTES, ids=lambda r: r.name)
def test_entry_lands_on_its_declared_routes(route):
    cr.check(route)


def test_switches_are_restored():
    from transeditor_amd import _lib
    from transeditor_amd.op import modconv as mc
    before = (mc.USE_WINOGRAD, mc.USE_SPLIT_BF16, mc.USE_SPLIT_S2, mc.USE_SPLIT_T2, mc.USE_SPLIT_1X1, mc.USE_CLOSED_MODCONV,
              _lib.wgrad_split())
    with pytest.raises(RuntimeError):
        with cr.switches(USE_WINOGRAD=False, split_bf16=False, USE_SPLIT_S2=False, USE_SPLIT_T2=False, USE_SPLIT_1X1=False,
                         USE_CLOSED_MODCONV=False):
            assert _lib.wgrad_split() == 0
            raise RuntimeError('leave the context by an exception')
    assert (mc.USE_WINOGRAD, mc.USE_SPLIT_BF16, mc.USE_SPLIT_S2, mc.USE_SPLIT_T2, mc.USE_SPLIT_1X1, mc.USE_CLOSED_MODCONV,
            _lib.wgrad_split()) == before


def test_table_covers_every_route_the_selectors_take():
    fwd, dgrad, plain, forms = cr.sweep()
    # the sweep finds exactly the routes the table module lists: a new selector branch fails here
    assert fwd == cr.ALL_FWD, f'forward routes changed: {sorted(fwd ^ cr.ALL_FWD)}'
    assert dgrad == cr.ALL_DGRAD, f'data-gradient routes changed: {sorted(dgrad ^ cr.ALL_DGRAD)}'
    assert plain == cr.ALL_PLAIN_1X1, f'plain 1x1 routes changed: {sorted(plain ^ cr.ALL_PLAIN_1X1)}'
    assert forms == set(cr.WGRAD_FORMS), f'weight-gradient forms changed: {sorted(forms ^ set(cr.WGRAD_FORMS))}'
    # ... and the table has an entry on each of them
    mod = [r for r in cr.ROUTES if r.op != 'skip']
    skip = [r for r in cr.ROUTES if r.op == 'skip']
    missing = {
        'fwd': cr.ALL_FWD - {r.fwd for r in mod},
        'dgrad': cr.ALL_DGRAD - {r.dgrad for r in mod},
        'plain 1x1': cr.ALL_PLAIN_1X1 - ({r.fwd for r in skip} | {r.dgrad for r in skip}),
        'wgrad form': set(cr.WGRAD_FORMS) - {r.wgrad[1] for r in cr.ROUTES},
        'wgrad split_supported': {0, 1, 2} - {r.wgrad[0] for r in cr.ROUTES},
        'wgrad plan': set(cr.WGRAD_PLANS) - {r.wgrad[2] for r in cr.ROUTES},
    }
    assert not any(missing.values()), f'routes without a table entry: { {k: v for k, v in missing.items() if v} }'
    # mixed routes: forward and data gradient on different arithmetic, both ways, for each op kind with a split form
    split = lambda pair: pair[1] in ('3X3W6', 'S2S6', 'T2S6', '1X1S6')
    for op in ('3x3', 'down', 'up', 'skip'):
        kinds = {(split(r.fwd), split(r.dgrad)) for r in cr.ROUTES if r.op == op and not r.switches}
        assert (True, False) in kinds, f'{op}: no entry with a split forward and an fp32 data gradient'
        assert (False, True) in kinds, f'{op}: no entry with an fp32 forward and a split data gradient'
    # every module switch has an entry that runs with it off
    for sw in ('USE_WINOGRAD', 'split_bf16', 'USE_SPLIT_S2', 'USE_SPLIT_T2', 'USE_SPLIT_1X1', 'USE_CLOSED_MODCONV'):
        assert any(sw in r.switches for r in cr.ROUTES), f'no entry runs with {sw} off'


@pytest.mark.parametrize('edge', sorted(cr.EDGES), ids=str)
def test_predicate_edges(edge):
    """each split predicate has an entry just inside and one just outside, which differ in one quantity only"""
    inside, outside = (cr.BY_NAME[n] for n in cr.EDGES[edge])
    assert inside.op == outside.op and not inside.switches and not outside.switches
    assert sum(a != b for a, b in zip(inside.shape, outside.shape)) == 1, (inside.shape, outside.shape)
    routes = lambda r: (r.fwd, r.dgrad, r.wgrad[1])
    assert routes(inside) != routes(outside), f'{edge}: {inside.name} and {outside.name} take the same routes'


def test_split_off_moves_every_split_route():
    """with the split-bf16 switch off no entry's shape reaches a split kernel (convolutions and weight gradients)"""
    split_kinds = {'3X3W6', 'S2S6', 'T2S6', '1X1S6'}
    with cr.switches(split_bf16=False):
        for r in cr.ROUTES:
            f, d = cr.conv_routes(r)
            assert f[1] not in split_kinds and d[1] not in split_kinds, r.name
            assert cr.wgrad_route(r)[1] == 'fp32', r.name

"""bench.py --full: a plain run measures its headline alone; every other leg (sub-benchmarks, live counters, CPU baseline,
communication evidence, the other sampling paths) runs only with --full (no GPU needed for the choice itself)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
    return bench.parse()


@pytest.mark.parametrize('workload', ['train', 'generator', 'sample'])
@pytest.mark.parametrize('world,dist_on', [(1, False), (1, True), (2, True)])
def test_plain_run_has_no_extra_legs(monkeypatch, workload, world, dist_on):
    args = _args(monkeypatch, '--gpus', str(world), '--steps', '20', '--warmup', '5', '--workload', workload)
    assert args.full is False
    assert not any(bench.extra_legs(args, world, dist_on).values())


def test_full_run_legs(monkeypatch):
    legs = bench.extra_legs(_args(monkeypatch, '--full'), 1, False)
    assert legs == {'sub_benchmarks': True, 'counters': True, 'cpu_baseline': True, 'comm': False, 'sampling_paths': False}
    legs = bench.extra_legs(_args(monkeypatch, '--full', '--gpus', '2'), 2, True)
    assert legs == {'sub_benchmarks': False, 'counters': False, 'cpu_baseline': False, 'comm': True, 'sampling_paths': False}
    assert bench.extra_legs(_args(monkeypatch, '--full'), 1, True)['comm']                  # the world-1 rehearsal of the N > 1 path
    legs = bench.extra_legs(_args(monkeypatch, '--full', '--workload', 'generator'), 1, False)
    assert legs == {'sub_benchmarks': False, 'counters': True, 'cpu_baseline': True, 'comm': False, 'sampling_paths': False}
    legs = bench.extra_legs(_args(monkeypatch, '--full', '--workload', 'sample'), 1, False)
    assert legs == {'sub_benchmarks': False, 'counters': False, 'cpu_baseline': False, 'comm': False, 'sampling_paths': True}


def test_no_switches_drop_single_legs_of_a_full_run(monkeypatch):
    legs = bench.extra_legs(_args(monkeypatch, '--full', '--no-cpu-baseline', '--no-sub'), 1, False)
    assert legs == {'sub_benchmarks': False, 'counters': True, 'cpu_baseline': False, 'comm': False, 'sampling_paths': False}

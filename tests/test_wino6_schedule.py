"""CPU tier: the per-tile phase schedule of wino6q_kernel's tile walk (transeditor_amd/csrc/wino6_schedule.h, the functions the kernel takes
its decisions from) is compiled for the host and replayed.  A barrier mismatch between the two wave groups of a block is a hang on
the GPU: this replay, not a GPU run, is what guards against it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'schedule_replay', 'wino6_schedule_check.cpp')


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++') if c and shutil.which(c)), None)
    assert cxx is not None, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('w6sched') / 'wino6_schedule_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-I', os.path.join(ROOT, 'transeditor_amd', 'csrc'), SRC, '-o', exe])
    return exe


@pytest.mark.parametrize('nstage', [2, 8])
@pytest.mark.parametrize('ntile', [1, 2, 3, 17])
def test_tile_walk_schedule_replay(checker, ntile, nstage):
    """equal barrier counts for the two groups (per block and per tile); no weight half read before the wait of its DMA or renewed
    while it can be read; no half tile read before the write_res that fills it or overwritten while its group can still read it"""
    r = subprocess.run([checker, str(ntile), str(nstage)], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout
    assert r.stdout.startswith('ok:')

"""bench.py --dump-outputs: what the timed path returned in its last step, written as .npy within a fixed byte budget (no GPU
needed for the writer itself; the GPU runs of bench.py call the same function)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _arrays():
    g = torch.Generator().manual_seed(5)
    return {'loss_g': torch.tensor(1.25), 'image': torch.randn(2, 3, 16, 16, generator=g),
            'generator_params': torch.randn(300_000, generator=g), 'g_ema_params': torch.randn(200_000, generator=g),
            'half': torch.randn(10, generator=g).half(), 'double': torch.randn(7, generator=g, dtype=torch.float64)}


def test_dump_outputs_budget_dtypes_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 1 << 20)
    arrs = _arrays()
    bench.dump_outputs(str(tmp_path / 'a'), arrs)
    bench.dump_outputs(str(tmp_path / 'b'), arrs)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(k + '.npy' for k in arrs)
    data = sum(np.load(tmp_path / 'a' / f).nbytes for f in files)
    assert data <= 1 << 20
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= (1 << 20) + 128 * len(files)
    for f in files:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    # small outputs whole and in their own shape and precision
    assert np.load(tmp_path / 'a' / 'loss_g.npy').shape == () and float(np.load(tmp_path / 'a' / 'loss_g.npy')) == 1.25
    assert np.array_equal(np.load(tmp_path / 'a' / 'image.npy'), arrs['image'].numpy())
    assert np.array_equal(np.load(tmp_path / 'a' / 'double.npy'), arrs['double'].numpy())
    assert np.array_equal(np.load(tmp_path / 'a' / 'half.npy'), arrs['half'].float().numpy())
    # the large ones: a sample of their own elements, as big as the budget allows
    for name in ('generator_params', 'g_ema_params'):
        s = np.load(tmp_path / 'a' / f'{name}.npy')
        assert s.ndim == 1 and 100_000 < s.size < arrs[name].numel()
        assert np.isin(s, arrs[name].numpy()).all()


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '3', '--dump-outputs', 'out'])
    args = bench.parse()
    assert args.steps == 3 and args.dump_outputs == 'out'

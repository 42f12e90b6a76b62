"""Writes tests/golden/ranger_ref.npz and tests/golden/RANGER_REPORT.txt from the reference's own Ranger class.  CPU only.

    python tools/ranger_golden.py --reference /path/to/the/reference/tree

The reference's pSp/training/ranger.py is imported from --reference (it runs on a current torch with deprecation warnings only)
and stepped 13 times in fp32 on the small shapes of tests/ranger_restated.py, in the two configurations defined there, with that
module's deterministic gradients.  The fixture holds, per configuration: the initial parameters, the parameters and the three
state tensors after steps 7 and 13, the reference's (N_sma, step_size) for every step, and the param_groups of its state_dict()
(as JSON).  The report holds the yardsticks: how far the reference's fp32 results are from the fp64 restatement.
"""
import argparse
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ranger_restated as RR  # noqa: E402


def reference_class(tree):
    path = os.path.join(tree, 'pSp', 'training', 'ranger.py')
    spec = importlib.util.spec_from_file_location('reference_ranger', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Ranger


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference tree (holds pSp/training/ranger.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    a = ap.parse_args()
    Ref = reference_class(a.reference)
    warnings.simplefilter('ignore')
    ids = RR.SMALL_IDS
    arrays, report = {}, []
    report.append('Ranger golden: the reference class (pSp/training/ranger.py) in fp32 against the fp64 restatement '
                  '(tests/ranger_restated.py)')
    report.append(f'torch {torch.__version__}; shapes ' + ' '.join(f'{t}:{RR.SHAPES[t]}' for t in ids))
    report.append('per tensor and quantity: max|x32 - x64|, max|x64|, their ratio in units of 2^-20 (the CPU test\'s bound is 1.0)')
    worst = {}
    for cfg in RR.CONFIGS:
        params = [torch.nn.Parameter(RR.param0(t).clone()) for t in ids]
        opt = RR.make_optimizer(Ref, params, ids, cfg)
        x64 = RR.run(ids, cfg, torch.float64)
        sched = np.zeros((RR.STEPS, 2))
        for t, p in zip(ids, params):
            arrays[f'{cfg}_p0_{t}'] = p.detach().numpy().copy()
        for step in range(1, RR.STEPS + 1):
            for t, p in zip(ids, params):
                p.grad = RR.grad(t, step).clone()
            opt.step()
            buf = opt.radam_buffer[step % 10]
            assert buf[0] == step
            sched[step - 1] = buf[1], buf[2]
            if step in RR.RECORD:
                report.append(f'configuration ({cfg}), step {step}')
                for t, p in zip(ids, params):
                    st = opt.state[p]
                    assert st['step'] == step and type(st['step']) is int
                    got = dict(p=p.detach(), **{k: st[k] for k in RR.STATE_KEYS})
                    for k, v in got.items():
                        arrays[f'{cfg}_s{step}_{t}_{k}'] = v.numpy().copy()
                        ref = x64[step][t][k]
                        err, mag = float((v.double() - ref).abs().max()), float(ref.abs().max())
                        ratio = err / (2.0 ** -20 * mag) if mag else 0.0
                        worst[(cfg, k)] = max(worst.get((cfg, k), 0.0), ratio)
                        report.append(f'  {t}:{str(RR.SHAPES[t]):14s} {k:11s} err {err:.3e}  max {mag:.3e}  ratio {ratio:.3f}')
                if step == RR.RECORD[0]:
                    arrays[f'{cfg}_param_groups'] = np.array(json.dumps(opt.state_dict()['param_groups']))
        arrays[f'{cfg}_schedule'] = sched
        c = RR.CONFIGS[cfg]
        mine = np.array([RR.schedule(s, *c['betas'], c['N_sma_threshhold'])[:2] for s in range(1, RR.STEPS + 1)])
        report.append(f'configuration ({cfg}) schedule: max relative difference restatement / reference '
                      f'{float(np.abs(mine / sched - 1).max()):.3e}; N_sma ' + ' '.join(f'{v:.3f}' for v in sched[:, 0]))
    report.append('worst ratio per configuration and quantity: ' + ', '.join(f'({c}) {k} {v:.3f}' for (c, k), v in sorted(worst.items())))
    os.makedirs(a.out, exist_ok=True)
    np.savez(os.path.join(a.out, 'ranger_ref.npz'), **arrays)
    with open(os.path.join(a.out, 'RANGER_REPORT.txt'), 'w') as f:
        f.write('\n'.join(report) + '\n')
    print('\n'.join(report))
    print(f'{os.path.getsize(os.path.join(a.out, "ranger_ref.npz"))} bytes')


if __name__ == '__main__':
    main()

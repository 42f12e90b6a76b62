"""Time of one Ranger step (transeditor_amd.optim.Ranger, te_mt_ranger_f32 in csrc/optim.hip) over the parameters of the true
dual-space pSp encoder on the MI355X.

    python tools/ranger_time.py [--reps 9] [--out profiles/ranger/time.json]

The workload is the encoder's parameter census: the shapes of GradualStyleEncoder's parameters (the key and shape list of
tests/golden/psp_encoder_ref.npz, which tests/test_psp_encoder_cpu.py holds equal to psp_encoder_restated.state_dict's; the batch
norm statistics are buffers and are left out), filled with random data.  Timed with HIP events around whole step() calls, the
median of --reps after eight untimed steps (so that RAdam is on its rectified branch, where it stays).  A step() is host work (the
checks and the pointer table over 571 tensors) followed by one launch; the events see both, because the device waits for the
launch.  For the two library optimisers the launch alone is timed too (events around the library call, --reps more steps), and
the bytes per second are the launch's:
  ranger_plain     : Ranger.step() on a step without lookahead                       7 floats moved per element
  ranger_lookahead : Ranger.step() on a lookahead step                                9 floats per element
  fused_adam       : FusedAdam.step() on the same list (te_mt_adam_f32), the streaming yardstick     7 floats per element
  torch_per_tensor : the reference's algorithm (pSp/training/ranger.py:79-165) as per-tensor torch ops on the device, written out
                     below with today's torch signatures; what a user runs without this kernel.  A step without lookahead.
GPU only.
"""
import argparse
import json
import sys

import torch

from net_timing import shares, timed, write_json

WARM = 8


def census():
    from conftest import load_golden
    z = load_golden('psp_encoder_ref')
    return [tuple(int(v) for v in str(s).split(',') if v) for k, s in zip(z['keys'], z['shapes'])
            if not str(k).endswith(('running_mean', 'running_var', 'num_batches_tracked'))]


def make_params(shapes, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    params = []
    for s in shapes:
        p = torch.nn.Parameter(torch.randn(s, device='cuda', generator=g) * 0.05)
        p.grad = torch.randn(s, device='cuda', generator=g) * 0.01 + 0.003
        params.append(p)
    return params


class TorchRanger:
    """ranger.py:79-165 restated op for op on the device (defaults; fp32, so its .float() copies are the identity)"""

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, betas=(.95, 0.999), eps=1e-5, threshold=5):
        self.params, self.lr, self.alpha, self.k, self.betas, self.eps, self.threshold = params, lr, alpha, k, betas, eps, threshold
        self.state = [dict(exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p), slow_buffer=p.detach().clone()) for p in params]
        self.steps = 0

    @torch.no_grad()
    def step(self):
        from transeditor_amd.optim import radam_schedule
        self.steps += 1
        beta1, beta2 = self.betas
        _, step_size, rectified = radam_schedule(self.steps, beta1, beta2, self.threshold)
        for p, st in zip(self.params, self.state):
            grad = p.grad
            if grad.dim() > 1:
                grad.add_(-grad.mean(dim=tuple(range(1, grad.dim())), keepdim=True))
            st['exp_avg_sq'].mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
            st['exp_avg'].mul_(beta1).add_(grad, alpha=1 - beta1)
            if rectified:
                denom = st['exp_avg_sq'].sqrt().add_(self.eps)
                p.addcdiv_(st['exp_avg'], denom, value=-step_size * self.lr)
            else:
                p.add_(st['exp_avg'], alpha=-step_size * self.lr)
            if self.steps % self.k == 0:
                st['slow_buffer'].add_(p - st['slow_buffer'], alpha=self.alpha)
                p.copy_(st['slow_buffer'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ranger_time.py needs a GPU')
    from transeditor_amd import _lib
    from transeditor_amd.optim import TILE, FusedAdam, Ranger, gc_row_len, row_groups
    shapes = census()
    numel = sum(torch.Size(s).numel() for s in shapes)
    work = row_groups([torch.Size(s).numel() for s in shapes], [gc_row_len(s) for s in shapes])
    res = {'command': ' '.join(['python tools/ranger_time.py'] + sys.argv[1:]), 'tensors': len(shapes), 'parameters': numel,
           'tile': TILE, 'blocks': int(work.shape[1]), 'reps': a.reps, 'untimed_steps': WARM}

    def case(name, make, floats, op=None):
        params = make_params(shapes, 11)
        opt = make(params)
        for _ in range(WARM - 1):                      # (timed() runs one more untimed call)
            opt.step()
        med, ts = timed(opt.step, a.reps)
        res[name] = {'ms_median': round(med, 4), 'ms_all': [round(t, 4) for t in ts]}
        if op:
            ks = sorted(shares(opt.step, [(_lib, op, 'launch')])['launch'][0] for _ in range(a.reps))
            res[name].update(launch_ms_median=round(ks[len(ks) // 2], 4), launch_ms_all=[round(t, 4) for t in ks], floats_per_element=floats,
                             launch_TB_per_s=round(numel * 4 * floats / (ks[len(ks) // 2] * 1e-3) / 1e12, 3))
        print(json.dumps({name: res[name]}), flush=True)
        del opt, params
        torch.cuda.empty_cache()

    case('ranger_plain', lambda p: Ranger(p, lr=1e-4, k=10 ** 9), 7, 'mt_ranger')
    case('ranger_lookahead', lambda p: Ranger(p, lr=1e-4, k=1), 9, 'mt_ranger')
    case('fused_adam', lambda p: FusedAdam(p, lr=1e-4), 7, 'mt_adam')
    case('torch_per_tensor', lambda p: TorchRanger(p, lr=1e-4, k=10 ** 9), 0)
    res['torch_per_tensor_over_ranger_plain'] = round(res['torch_per_tensor']['ms_median'] / res['ranger_plain']['ms_median'], 3)
    res['ranger_plain_over_fused_adam'] = round(res['ranger_plain']['ms_median'] / res['fused_adam']['ms_median'], 3)
    res['ranger_plain_launch_over_fused_adam_launch'] = round(res['ranger_plain']['launch_ms_median'] / res['fused_adam']['launch_ms_median'], 3)
    res['ranger_lookahead_over_ranger_plain'] = round(res['ranger_lookahead']['ms_median'] / res['ranger_plain']['ms_median'], 3)
    print(json.dumps({k: v for k, v in res.items() if '_over_' in k}), flush=True)
    write_json(res, a.out)


if __name__ == '__main__':
    main()

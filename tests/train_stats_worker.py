"""Helper of tests/test_gpu_train_stats.py, run as a child process so that CDRL_GUARD / CDRL_GRAPH are in the environment before the
library loads: a sequence of apply steps on injected gradients with the train-stats ring on; writes what it fetched as JSON.
usage: train_stats_worker.py <out.json> <ring rows> <apply steps>"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from carla_driving_rl_agent_amd.engine import LearnerEngine          # noqa: E402
from carla_driving_rl_agent_amd.init import init_engine_parameters   # noqa: E402

B, H, W = 4, 48, 64


def run_applies(eng, steps):
    """policy / value applies alternating on seeded gradients, hyper-parameters changing every step."""
    for k in range(steps):
        g = torch.randn(eng.grads_total, generator=torch.Generator().manual_seed(300 + k)) * 1e-3 * (k + 1)
        eng.grads.copy_(g.to(eng.grads.device))
        eng.set_hparams(policy_lr=1e-4 * (k + 1), value_lr=2e-4 * (k + 1), dynamics_lr=3e-4, clip_ratio=0.1 + 0.01 * k)
        if k % 2 == 0:
            eng.policy_apply()
        else:
            eng.value_apply()


def make_engine(rows, **kw):
    eng = LearnerEngine(B, device='cuda:0', H=H, W=W, train_stats=rows, **kw)
    init_engine_parameters(eng, seed=8)
    eng.reset_optimizer()
    return eng


if __name__ == '__main__':
    out, rows, steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    torch.cuda.set_device(0)
    eng = make_engine(rows)
    graphs_on = int(eng.lib.cdrl_learner_tail_offset(eng.h)) == eng.region('trunk', True)[1]
    run_applies(eng, steps)
    first = eng.train_stats()
    again = eng.train_stats()
    guards = eng.check_guards() if os.environ.get('CDRL_GUARD') == '1' else None
    eng.reset_optimizer()
    eng.params.copy_(make_engine(rows).params)
    run_applies(eng, steps)
    second = eng.train_stats()
    with open(out, 'w') as f:
        json.dump(dict(first=first, again=again, second=second, guards=guards, graphs_on=graphs_on), f)

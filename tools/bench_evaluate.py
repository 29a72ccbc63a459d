"""env-steps/s of CARLAgent.evaluate on FakeCARLAEnvironment: image stacks of 4 x 90 x 120 x 3, shards of E = 1 / 8 / 32 environments,
sampled and deterministic actions, in ONE process with one agent.  Every timed call runs one wave (trials = E) of `--timesteps`
steps (no episode length: every trial runs to the end), i.e. per step one observe() of E host observations, one inference forward
of the E-environment engine, one cdrl_beta_act launch, one device-to-host copy of the actions and E environment steps; per wave one
read of the device sums and one JSON file.  The synthetic environment draws every observation with numpy on the host, which is
part of the figure (the `env_only` row times that alone).  Configurations alternate per round; median (min, max) over the timed
rounds, one untimed round first (it builds the E-environment engine).

    python tools/bench_evaluate.py [--envs 1 8 32] [--timesteps 40] [--rounds 5] [--out profiles/r13_evaluate_bench.json]
"""
import argparse
import contextlib
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(values, digits=1):
    return dict(median=round(statistics.median(values), digits), min=round(min(values), digits), max=round(max(values), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='+', default=[1, 8, 32])
    ap.add_argument('--timesteps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=5, help='timed rounds per configuration (one untimed first)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r13_evaluate_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment

    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    torch.cuda.set_device(0)
    T, H, W = 4, 90, 120
    work = tempfile.mkdtemp(prefix='cdrl_bench_')
    shard = [FakeCARLAEnvironment(image_shape=(H, W, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=2,
                                  image_range=(0.0, 1.0), seed=100 + e) for e in range(max(args.envs))]
    agent = CARLAgent(shard[0], batch_size=64, log_mode=None, seed=5, aug_intensity=0.0, weights_dir=os.path.join(work, 'weights'),
                      evaluation_dir=os.path.join(work, 'evaluation'), name='bench_evaluate')
    configs = [(E, det) for E in args.envs for det in (False, True)]
    rates = {c: [] for c in configs}
    for k in range(args.rounds + 1):
        for E, det in configs[k % len(configs):] + configs[:k % len(configs)]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):      # evaluate() prints one line per trial
                results = agent.evaluate('bench', timesteps=args.timesteps, trials=E, envs=shard[:E], deterministic=det)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert results['timesteps'] == [args.timesteps] * E
            if k:
                rates[(E, det)].append(E * args.timesteps / dt)
    # the host environment alone: reset + `timesteps` steps of E environments, no agent
    env_only = {}
    for E in args.envs:
        vals = []
        for _ in range(3):
            t0 = time.perf_counter()
            for env in shard[:E]:
                env.reset()
                for _ in range(args.timesteps):
                    env.step(np.zeros(2, np.float32))
                env.reset_info()
            vals.append(E * args.timesteps / (time.perf_counter() - t0))
        env_only[E] = spread(vals)
    out = dict(metric='evaluate', stack=[T, H, W, 3], timesteps=args.timesteps, timed_rounds=args.rounds,
               clock='host perf_counter around one evaluate() call of one wave (trials = E), ending in a device synchronise; '
                     'env-steps/s = E * timesteps / seconds; median (min, max) over the timed rounds, configurations alternating',
               rows=[dict(envs=E, deterministic=det, env_steps_per_s=spread(rates[(E, det)])) for E, det in configs],
               env_only=[dict(envs=E, env_steps_per_s=env_only[E], what='reset + steps of the synthetic environments alone (host numpy)')
                         for E in args.envs])
    for row in out['rows'] + out['env_only']:
        print(json.dumps(row), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(dict(metric=out['metric'], written=os.path.relpath(args.out, ROOT))))


if __name__ == '__main__':
    main()

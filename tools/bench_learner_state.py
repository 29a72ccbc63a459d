"""Size on disk of one full learner state and wall time of CARLAgent.save_state / load_state (learner_state.py).

An agent at the default configuration (B samples of 4 x 90 x 120 x 3, Adam) saves its state into a temporary directory
--reps + 1 times and loads it as often; the first call of each is reported apart (directory creation, first page faults), the rest
by their median.  Times are host wall clock around the whole call, device synchronized before and (load) after.  Prints one JSON
line; `profiles/r12_learner_state.json` is that line.

    python tools/bench_learner_state.py [--batch 256] [--reps 5] [--optimizer adam]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5, help='timed calls behind the first one')
    ap.add_argument('--optimizer', default='adam')
    args = ap.parse_args()

    import torch
    from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment

    T, H, W = 4, 90, 120
    env = FakeCARLAEnvironment(image_shape=(H, W, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=2,
                               image_range=(0.0, 1.0))
    with tempfile.TemporaryDirectory() as tmp:
        agent = CARLAgent(env, batch_size=args.batch, log_mode=None, seed=3, weights_dir=tmp, name='m', optimizer=args.optimizer)
        eng = agent.network.engine
        save_s, load_s = [], []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.save_state()
            save_s.append(time.perf_counter() - t0)
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.load_state()
            torch.cuda.synchronize()
            load_s.append(time.perf_counter() - t0)
        base = agent.base_path
        stem = json.load(open(os.path.join(base, 'learner_state.json')))['checkpoint']
        one = {f: os.path.getsize(os.path.join(base, f)) for f in sorted(os.listdir(base))
               if f == 'learner_state.json' or f.startswith(stem + '.index') or f.startswith(stem + '.data-')}
    print(json.dumps(dict(
        what='size of one full learner state on disk and wall time of CARLAgent.save_state / load_state (first call, then median of '
             f'{args.reps})',
        config=dict(B=args.batch, T=T, H=H, W=W, optimizer=eng.optimizer), params_floats=eng.params_total, slot_floats=eng.grads_total,
        files_of_one_state=one, bytes_of_one_state=sum(one.values()),
        save_state_s=dict(first=save_s[0], median=statistics.median(save_s[1:]), all=save_s),
        load_state_s=dict(first=load_s[0], median=statistics.median(load_s[1:]), all=load_s))))


if __name__ == '__main__':
    main()

"""Augmentation of an environment shard's observations: the per-environment loop (CARLAgent(batch_augment=False): one
Augmenter.__call__ per environment = one host-to-device copy, one plan struct and up to six launches + a copy each, then one
torch.stack) against the batched path (batch_augment=True: one gather into page-locked memory, one copy, one packed-plan upload,
FIVE launches for any E), in ONE process.

Part 1 (one step): stacks of 4 x 90 x 120 x 3, E in {8, 32, 128}, starting from E host numpy stacks and ending in one (E, ...) device
tensor.  Both paths get the same plans: once E plans drawn at alpha = 1.0 (what a rollout sees: ops fire for some environments and
not for others), once the all-ops plan of tools/bench_rollout_rows.py for every environment (the most work a step can ask for).
    wall_ms    host clock from the host arrays to a device synchronise
    device_ms  event-to-event time on the stream for the same call with the images ALREADY on the device (launches, plan upload,
               the idle gaps between launches; no image copy)
Rounds alternate which path goes first; the median over the timed rounds is reported with (min, max) beside it.  The outputs of the
two paths are compared once per configuration (they must be equal).
Part 2 (rollout): env-steps/s of collect() on FakeCARLAEnvironment at E = 32 with aug_intensity 0, 1.0 (loop) and 1.0 (batched); the
three agents are rebuilt alike, the modes alternate per rollout.  The synthetic environment draws every observation with numpy on
the host, which is part of the figure.

    python tools/bench_augment_shard.py [--envs 8 32 128] [--rounds 20] [--out profiles/r11_augment_shard_bench.json]
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

LAUNCHES_PER_BATCH_CALL = 5         # channel mean, jitter, blur + noise, min/max, final (csrc/augment.hip::augment_images_batch)


def spread(values, digits=3):
    return dict(median=round(statistics.median(values), digits), min=round(min(values), digits), max=round(max(values), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='+', default=[8, 32, 128])
    ap.add_argument('--rounds', type=int, default=20, help='timed rounds per configuration (3 untimed ones first)')
    ap.add_argument('--collect-envs', type=int, default=32)
    ap.add_argument('--timesteps', type=int, default=16)
    ap.add_argument('--rollouts', type=int, default=5, help='timed rollouts per mode (one untimed first)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11_augment_shard_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.rl.augmentations import Augmenter, draw_plans, empty_plan

    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    torch.cuda.set_device(0)
    DEV = 'cuda:0'
    T, H, W = 4, 90, 120
    aug = Augmenter(DEV)

    def loop_path(stacks, plans):
        return torch.stack([aug(x, p) for x, p in zip(stacks, plans)], dim=0)

    def batch_path(stacks, plans):
        return aug.batch(stacks, plans)                      # a list of host stacks is gathered by the augmenter itself

    def timed(fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn(*a)
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    w3 = list(np.random.default_rng(9).normal(1.0, 0.25, 27).astype(np.float32)) + [0.0] * 48
    out = dict(metric='augment_shard', stack=[T, H, W, 3], timed_rounds=args.rounds, launches_per_batch_call=LAUNCHES_PER_BATCH_CALL,
               clock='wall_ms: host perf_counter from E host numpy stacks to a device synchronise; device_ms: event-to-event on the '
                     'stream, images already resident; median (min, max) over the timed rounds, paths alternating',
               step=[], collect=None)

    # ---- part 1: one step of E environments, both paths on the same inputs and plans
    for E in args.envs:
        host = [np.random.default_rng(1000 + e).uniform(0.0, 1.0, (T, H, W, 3)).astype(np.float32) for e in range(E)]
        resident = torch.as_tensor(np.stack(host, axis=0)).to(DEV)
        resident_list = list(resident)
        all_ops = []
        for e in range(E):
            p = empty_plan(seed=0x1234 + e, offset=5 + e)
            p.update(jitter=1, brightness=0.05, contrast=1.2, saturation=1.3, hue=0.07, blur_size=3, blur_kernel=w3, salt_pepper=1,
                     gauss_noise=1, normalize=1, cutout_size=6, cutout_cell=3, dropout_size=81)
            all_ops.append(p)
        for name, plans in (('drawn_alpha_1', draw_plans(1.0, np.random.default_rng(E), E, first_offset=1)), ('all_ops', all_ops)):
            assert torch.equal(loop_path(host, plans), batch_path(host, plans)), (E, name)
            t = dict(loop_wall=[], batch_wall=[], loop_dev=[], batch_dev=[])
            for k in range(args.rounds + 3):
                for mode in (('loop', 'batch') if k % 2 else ('batch', 'loop')):
                    fn = loop_path if mode == 'loop' else batch_path
                    wall, _ = timed(fn, host, plans)
                    _, dev = timed(fn, resident_list if mode == 'loop' else resident, plans)
                    if k >= 3:
                        t[mode + '_wall'].append(wall)
                        t[mode + '_dev'].append(dev)
            row = dict(envs=E, plans=name,
                       ops_fired={op: int(sum(1 for p in plans if p[op])) for op in ('jitter', 'blur_size', 'salt_pepper', 'gauss_noise',
                                                                                     'normalize', 'cutout_size', 'dropout_size')},
                       loop_wall_ms=spread(t['loop_wall']), batch_wall_ms=spread(t['batch_wall']),
                       loop_device_ms=spread(t['loop_dev']), batch_device_ms=spread(t['batch_dev']))
            row['wall_loop_over_batch'] = round(row['loop_wall_ms']['median'] / row['batch_wall_ms']['median'], 2)
            row['device_loop_over_batch'] = round(row['loop_device_ms']['median'] / row['batch_device_ms']['median'], 2)
            out['step'].append(row)
            print(json.dumps(row), flush=True)
        del resident, resident_list
        torch.cuda.empty_cache()

    # ---- part 2: collect() at E environments, aug_intensity 0 / 1.0 loop / 1.0 batched
    E = args.collect_envs
    weights = tempfile.mkdtemp(prefix='cdrl_bench_')
    modes = dict(aug_off=dict(aug_intensity=0.0), aug_loop=dict(aug_intensity=1.0, batch_augment=False),
                 aug_batch=dict(aug_intensity=1.0, batch_augment=True))
    agents, shards, rates = {}, {}, {m: [] for m in modes}
    for m, kw in modes.items():
        shards[m] = [FakeCARLAEnvironment(image_shape=(H, W, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=2,
                                          image_range=(0.0, 1.0), seed=100 + e) for e in range(E)]
        agents[m] = CARLAgent(shards[m][0], batch_size=64, log_mode=None, seed=5, weights_dir=weights, name='bench_augment_shard', **kw)
    order = list(modes)
    for k in range(args.rollouts + 1):
        for m in order[k % 3:] + order[:k % 3]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):      # collect() prints one line per closed trajectory
                rollout = agents[m].collect(shards[m], args.timesteps, episode=k)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert sum(rollout.length) == E * args.timesteps
            if k:
                rates[m].append(E * args.timesteps / dt)
            for env in shards[m]:
                env.reset_info()
    out['collect'] = dict(envs=E, timesteps=args.timesteps, timed_rollouts=args.rollouts,
                          what='env-steps/s of collect() (host clock, ends in a device synchronise); the synthetic environment draws '
                               'each observation with numpy on the host',
                          env_steps_per_s={m: spread(v, 1) for m, v in rates.items()})
    out['collect']['batch_over_loop'] = round(out['collect']['env_steps_per_s']['aug_batch']['median']
                                              / out['collect']['env_steps_per_s']['aug_loop']['median'], 3)
    print(json.dumps(out['collect']), flush=True)

    shutil.rmtree(weights, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(dict(metric=out['metric'], written=os.path.relpath(args.out, ROOT))))


if __name__ == '__main__':
    main()

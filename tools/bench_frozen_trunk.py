"""Frozen-trunk update-step (CARLAgent(update_dynamics=False), cdrl_config.freeze_trunk) against the full one, in ONE process.

Two learners over the same seeded weights and the same rollout minibatch (bench.py's inputs: B samples of 4 x 90 x 120 x 3, re-sampled
Beta-PPO policy loss, one policy + one value minibatch step per update-step through DataParallelLearner.update_step).  After warm-up,
blocks of full and frozen update-steps alternate; each block is timed with HIP events on the launch stream between two synchronizes,
as bench.py times its region.  Prints one JSON line: ms per update-step of both modes (median over the blocks) and their ratio, both
workspaces, and the frozen step's algorithmic bytes (one pass over every tower tensor's input + output per forward, two forwards per
update-step) with its fraction of 8 TB/s.

    python tools/bench_frozen_trunk.py [--batch 1024] [--dtype bf16s] [--blocks 6 --steps 10 --warmup 5]
    python tools/bench_frozen_trunk.py --only frozen --blocks 1     (one mode: for a kernel trace of the frozen step)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--dtype', choices=['f32', 'bf16', 'bf16s'], default='f32')
    ap.add_argument('--blocks', type=int, default=6, help='timed blocks per mode (alternating)')
    ap.add_argument('--steps', type=int, default=10, help='update-steps per block')
    ap.add_argument('--warmup', type=int, default=5, help='untimed update-steps per mode before the first block')
    ap.add_argument('--only', choices=['full', 'frozen'], default=None)
    args = ap.parse_args()

    import torch
    from bench import ALG_ELEMS_PER_FRAME
    from carla_driving_rl_agent_amd import synthetic
    from carla_driving_rl_agent_amd.engine import LearnerEngine, gae_returns
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    from carla_driving_rl_agent_amd.parallel import DataParallelLearner

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    B, T, H, W = args.batch, 4, 90, 120
    modes = [args.only] if args.only else ['full', 'frozen']
    dps, ws = {}, {}
    for mode in modes:
        eng = LearnerEngine(B, device=dev, T=T, H=H, W=W, compute=args.dtype, freeze_trunk=(mode == 'frozen'))
        init_engine_parameters(eng, seed=42)
        dps[mode] = DataParallelLearner(eng)
        ws[mode] = eng.workspace_bytes

    r = synthetic.make_rollout(B, T=T, H=H, W=W, seed=42)
    states = {k: torch.as_tensor(v).to(dev) for k, v in r['states'].items()}
    rewards = torch.cat([torch.as_tensor(r['reward']).to(dev), torch.zeros(1, device=dev)])
    values = torch.cat([torch.as_tensor(r['value']).to(dev), torch.zeros((1, 2), device=dev)])
    hp = synthetic.DEFAULT_HP
    _, returns_be, _, adv = gae_returns(rewards, values, hp['gamma'], hp['lambda_'], hp['advantage_scale'])
    speed = (torch.as_tensor(r['speed'][:, 0]) / 100.0).to(dev).contiguous()
    sim = torch.as_tensor(r['similarity'][:, 0]).to(dev).contiguous()
    pol = dict(states=states, advantages=adv.contiguous(), old_log_prob=torch.as_tensor(r['old_log_prob']).to(dev), speed=speed,
               similarity=sim, u=torch.as_tensor(r['action']).to(dev), du_da=None, du_db=None)
    val = dict(states=states, returns=returns_be.contiguous(), speed=speed, similarity=sim)

    step_no = {m: 0 for m in modes}

    def run(mode, n):
        for _ in range(n):
            step_no[mode] += 1
            dps[mode].update_step(pol, val, resample=(42, step_no[mode]))

    for mode in modes:
        run(mode, args.warmup)
    torch.cuda.synchronize()
    times = {m: [] for m in modes}
    for _ in range(args.blocks):
        for mode in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run(mode, args.steps)
            e1.record()
            torch.cuda.synchronize()
            times[mode].append(e0.elapsed_time(e1) / args.steps)
    for mode in modes:
        assert torch.isfinite(dps[mode].engine.params).all(), mode

    elem = 2 if args.dtype == 'bf16s' else 4
    frozen_bytes = 2 * elem * B * T * ALG_ELEMS_PER_FRAME[(H, W)]        # two forwards, one pass over in + out each
    out = dict(metric='frozen_trunk_update_step', batch=B, image=[T, H, W, 3], dtype=args.dtype, blocks=args.blocks,
               steps_per_block=args.steps, warmup=args.warmup)
    for mode in modes:
        out[f'{mode}_ms_per_update_step'] = round(statistics.median(times[mode]), 4)
        out[f'{mode}_ms_blocks'] = [round(t, 4) for t in times[mode]]
        out[f'{mode}_workspace_bytes'] = ws[mode]
    if 'frozen' in modes:
        ms = out['frozen_ms_per_update_step']
        out['frozen_alg_bytes_per_update_step'] = frozen_bytes
        out['frozen_floor_ms_at_8TBps'] = round(frozen_bytes / PEAK_BYTES_PER_S * 1e3, 4)
        out['frozen_frac_of_8TBps'] = round(frozen_bytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 4)
    if len(modes) == 2:
        out['ratio_frozen_over_full'] = round(out['frozen_ms_per_update_step'] / out['full_ms_per_update_step'], 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()

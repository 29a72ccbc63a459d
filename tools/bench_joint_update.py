"""Joint policy + value update-step (engine.joint_forward_backward_resample + joint_apply: one trunk forward and backward, one trunk
optimizer step) against the separate update-step (policy pass, apply, value pass, apply), in ONE process.

Per configuration two learners over the same seeded weights and the same rollout minibatch (bench.py's inputs: B samples of
4 x 90 x 120 x 3, re-sampled Beta-PPO policy loss): one runs DataParallelLearner.update_step, the other DataParallelLearner.joint_step.
After warm-up, blocks of separate and joint steps alternate; each block is timed with HIP events on the launch stream between two
synchronizes, as bench.py times its region.  Writes one JSON file: per configuration the per-block times, their medians and spread,
and the ratio joint / separate; the CDRL_* overrides in effect.  Refuses to run under a wrong-result diagnostic switch.

    python tools/bench_joint_update.py                                   (f32, B = 256)
    python tools/bench_joint_update.py --configs f32:256 bf16s:1024 f32:256:frozen
    python tools/bench_joint_update.py --only joint --blocks 1           (one mode: for a kernel trace of the joint step)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ('separate', 'joint')


def bench_config(spec, args):
    import torch
    from carla_driving_rl_agent_amd import synthetic
    from carla_driving_rl_agent_amd.engine import LearnerEngine, gae_returns
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    from carla_driving_rl_agent_amd.parallel import DataParallelLearner

    parts = spec.split(':')
    dtype, B, frozen = parts[0], int(parts[1]), len(parts) > 2 and parts[2] == 'frozen'
    dev = 'cuda:0'
    T, H, W = 4, 90, 120
    modes = [args.only] if args.only else list(MODES)
    dps = {}
    for mode in modes:
        eng = LearnerEngine(B, device=dev, T=T, H=H, W=W, compute=dtype, freeze_trunk=frozen)
        init_engine_parameters(eng, seed=42)
        dps[mode] = DataParallelLearner(eng)

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
    joint = dict(pol, returns=val['returns'])

    step_no = {m: 0 for m in modes}

    def run(mode, n):
        for _ in range(n):
            step_no[mode] += 1
            if mode == 'joint':
                dps[mode].joint_step(joint, resample=(42, step_no[mode]))
            else:
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

    out = dict(config=spec, batch=B, image=[T, H, W, 3], dtype=dtype, frozen_trunk=frozen)
    for mode in modes:
        out[f'{mode}_ms_per_step'] = round(statistics.median(times[mode]), 4)
        out[f'{mode}_ms_blocks'] = [round(t, 4) for t in times[mode]]
        out[f'{mode}_block_spread_ms'] = round(max(times[mode]) - min(times[mode]), 4)
    if len(modes) == 2:
        out['ratio_joint_over_separate'] = round(out['joint_ms_per_step'] / out['separate_ms_per_step'], 4)
        out['saved_ms_per_step'] = round(out['separate_ms_per_step'] - out['joint_ms_per_step'], 4)
        out['faster_by_more_than_the_separate_spread'] = bool(out['saved_ms_per_step'] > out['separate_block_spread_ms'])
    del dps
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', nargs='+', default=['f32:256'], metavar='DTYPE:BATCH[:frozen]',
                    help='e.g. f32:256 bf16s:1024 f32:256:frozen (each timed on its own, one after the other)')
    ap.add_argument('--blocks', type=int, default=6, help='timed blocks per mode (alternating)')
    ap.add_argument('--steps', type=int, default=10, help='update-steps per block')
    ap.add_argument('--warmup', type=int, default=5, help='untimed update-steps per mode before the first block')
    ap.add_argument('--only', choices=MODES, default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15_joint_update_bench.json'))
    args = ap.parse_args()

    import torch
    from carla_driving_rl_agent_amd import _lib
    if _lib.diag_active():
        raise SystemExit(f'[bench_joint_update] refusing to benchmark: wrong-result diagnostic switches are active ({_lib.env_overrides()})')
    if not torch.cuda.is_available():
        raise SystemExit('[bench_joint_update] needs a GPU')
    torch.cuda.set_device(0)
    out = dict(metric='joint_update_step_vs_separate', device=torch.cuda.get_device_name(0), blocks=args.blocks,
               steps_per_block=args.steps, warmup=args.warmup, env_overrides=_lib.env_overrides(),
               note='one process; blocks of the two modes alternate; ms per update-step (one minibatch through both losses); '
                    'HIP events between two synchronizes',
               results=[bench_config(spec, args) for spec in args.configs])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

"""Update-step time with the gradient gate (cdrl_config.clip_mode = global, skip_nonfinite) in ONE process.

Four learners over the same seeded weights and the same rollout minibatch (bench.py's inputs: B samples of 4 x 90 x 120 x 3, float32,
re-sampled Beta-PPO policy loss, one policy + one value minibatch step per update-step through DataParallelLearner.update_step):
default, clip_mode='global', skip_nonfinite, and both.  After warm-up, blocks of update-steps alternate over the configurations; each
block is timed with HIP events on the launch stream between two synchronizes, as bench.py times its region.  Then the apply steps
alone (policy_apply + value_apply on the gradients the last pass left) are timed the same way.  The default configuration's own block
spread is the noise floor of the run: a difference below it is not a difference.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_grad_gate.py [--batch 256] [--blocks 5 --steps 40 --warmup 3] [--out profiles/r14_grad_gate_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [('default', dict()), ('global', dict(clip_mode='global')), ('skip_nonfinite', dict(skip_nonfinite=True)),
           ('global_skip_nonfinite', dict(clip_mode='global', skip_nonfinite=True))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--blocks', type=int, default=5, help='timed blocks per configuration (alternating)')
    ap.add_argument('--steps', type=int, default=40, help='update-steps per block')
    ap.add_argument('--warmup', type=int, default=3, help='untimed update-steps per configuration before the first block')
    ap.add_argument('--apply-reps', type=int, default=50, help='apply pairs per block of the apply-only timing')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()

    import torch
    from carla_driving_rl_agent_amd import synthetic
    from carla_driving_rl_agent_amd.engine import LearnerEngine, gae_returns
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    from carla_driving_rl_agent_amd.parallel import DataParallelLearner

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    B, T, H, W = args.batch, 4, 90, 120
    tags = [t for t, _ in CONFIGS]
    dps = {}
    for tag, kw in CONFIGS:
        eng = LearnerEngine(B, device=dev, T=T, H=H, W=W, **kw)
        init_engine_parameters(eng, seed=42)
        # all three thresholds on: every list's norm is computed and every element multiplied by its list's scale (the kernels
        # multiply whether or not the scale is below 1, so the timing does not depend on how often a list is actually clipped)
        eng.set_hparams(clip_norm_policy=1.0, clip_norm_value=1.0, clip_norm_dynamics=1.0)
        dps[tag] = DataParallelLearner(eng)

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

    step_no = {t: 0 for t in tags}

    def run(tag, n):
        for _ in range(n):
            step_no[tag] += 1
            dps[tag].update_step(pol, val, resample=(42, step_no[tag]))

    def applies(tag, n):
        e = dps[tag].engine
        for _ in range(n):
            e.policy_apply()
            e.value_apply()

    def timed(fn, tag, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn(tag, n)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for tag in tags:
        run(tag, args.warmup)
    torch.cuda.synchronize()
    times = {t: [] for t in tags}
    for _ in range(args.blocks):
        for tag in tags:
            times[tag].append(timed(run, tag, args.steps))
    gate = {}
    for tag in tags:
        e = dps[tag].engine
        assert torch.isfinite(e.params).all(), tag
        if e.gated:
            st = e.gate_stats()
            assert st['policy']['skipped'] == 0 and st['value']['skipped'] == 0, (tag, st)
            gate[tag] = st
    apply_times = {t: [] for t in tags}
    for tag in tags:
        applies(tag, 2)
    for _ in range(args.blocks):
        for tag in tags:
            apply_times[tag].append(timed(applies, tag, args.apply_reps))

    out = dict(metric='grad_gate_update_step', batch=B, image=[T, H, W, 3], dtype='f32', blocks=args.blocks,
               steps_per_block=args.steps, warmup=args.warmup, apply_pairs_per_block=args.apply_reps, configs={})
    base = statistics.median(times['default'])
    base_apply = statistics.median(apply_times['default'])
    for tag, kw in CONFIGS:
        ms, ams = statistics.median(times[tag]), statistics.median(apply_times[tag])
        out['configs'][tag] = dict(
            options=kw, ms_per_update_step=round(ms, 4), ms_blocks=[round(t, 4) for t in times[tag]],
            block_spread_ms=round(max(times[tag]) - min(times[tag]), 4), ratio_over_default=round(ms / base, 4),
            apply_ms_per_update_step=round(ams, 4), apply_ms_blocks=[round(t, 4) for t in apply_times[tag]],
            apply_ms_over_default=round(ams - base_apply, 4), gate_stats=gate.get(tag))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

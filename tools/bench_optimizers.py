"""Update-step time of every optimizer of cdrl_config.optimizer (PPOAgent(optimizer=...)), and of Adam with polyak averaging, in ONE
process.

One learner per configuration over the same seeded weights and the same rollout minibatch (bench.py's inputs: B samples of
4 x 90 x 120 x 3, re-sampled Beta-PPO policy loss, one policy + one value minibatch step per update-step through
DataParallelLearner.update_step).  After warm-up, blocks of update-steps alternate over the configurations; each block is timed with
HIP events on the launch stream between two synchronizes, as bench.py times its region.  Then the apply steps alone (policy_apply +
value_apply on the gradients the last pass left, no forward or backward) are timed the same way, and set against the bytes the
optimizer kernels stream: per trainable element one read of the gradient, one read and write of the weight and of each slot the
optimizer keeps (12 B for SGD, 20 B for RMSprop / Adagrad, 28 B for the others); the trunk steps twice per update-step.  Prints one
JSON line.

    python tools/bench_optimizers.py [--batch 256] [--blocks 4 --steps 8 --warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8.0e12
CONFIGS = [('adam', 1.0), ('sgd', 1.0), ('rmsprop', 1.0), ('adagrad', 1.0), ('adadelta', 1.0), ('adamax', 1.0), ('nadam', 1.0),
           ('ftrl', 1.0), ('adam', 0.99)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--blocks', type=int, default=4, help='timed blocks per configuration (alternating)')
    ap.add_argument('--steps', type=int, default=8, help='update-steps per block')
    ap.add_argument('--warmup', type=int, default=3, help='untimed update-steps per configuration before the first block')
    ap.add_argument('--apply-reps', type=int, default=20, help='apply pairs per block of the apply-only timing')
    args = ap.parse_args()

    import torch
    from carla_driving_rl_agent_amd import _lib, synthetic
    from carla_driving_rl_agent_amd.engine import LearnerEngine, gae_returns
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    from carla_driving_rl_agent_amd.parallel import DataParallelLearner

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    B, T, H, W = args.batch, 4, 90, 120
    tags = [f'{o}' if pk == 1.0 else f'{o}_polyak{pk}' for o, pk in CONFIGS]
    dps = {}
    for tag, (opt, pk) in zip(tags, CONFIGS):
        eng = LearnerEngine(B, device=dev, T=T, H=H, W=W, optimizer=opt, polyak=pk)
        init_engine_parameters(eng, seed=42)
        dps[tag] = DataParallelLearner(eng)
    eng0 = dps[tags[0]].engine
    n_elems = {m: eng0.region(m, True)[1] for m in ('trunk', 'policy', 'value')}

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
    for tag in tags:
        assert torch.isfinite(dps[tag].engine.params).all(), tag
    apply_times = {t: [] for t in tags}
    for tag in tags:
        applies(tag, 2)
    for _ in range(args.blocks):
        for tag in tags:
            apply_times[tag].append(timed(applies, tag, args.apply_reps))

    out = dict(metric='optimizer_update_step', batch=B, image=[T, H, W, 3], dtype='f32', blocks=args.blocks,
               steps_per_block=args.steps, warmup=args.warmup, apply_pairs_per_block=args.apply_reps,
               trainable_elems=n_elems, configs={})
    elems_per_step = 2 * n_elems['trunk'] + n_elems['policy'] + n_elems['value']
    base = None
    for tag, (opt, pk) in zip(tags, CONFIGS):
        used = sum(s is not None for s in _lib.OPTIMIZER_SLOTS[opt])
        bpe = 12 + 8 * used
        ms = statistics.median(times[tag])
        ams = statistics.median(apply_times[tag])
        base = ms if base is None else base
        out['configs'][tag] = dict(
            optimizer=opt, polyak=pk, ms_per_update_step=round(ms, 4), ms_blocks=[round(t, 4) for t in times[tag]],
            ratio_over_adam=round(ms / base, 4), apply_ms_per_update_step=round(ams, 4),
            apply_bytes_per_trainable_elem=bpe, apply_bytes_per_update_step=bpe * elems_per_step,
            apply_frac_of_8TBps=round(bpe * elems_per_step / (ams * 1e-3) / PEAK_BYTES_PER_S, 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()

"""Update-step time with the trust-region guard (cdrl_config.trust, PPOAgent(target_kl=..., kl_penalty=...)) in ONE
process.

Three learners over the same seeded weights and the same rollout minibatch (bench.py's inputs: B samples of 4 x 90 x 120 x 3, float32,
re-sampled Beta-PPO policy loss, one policy + one value minibatch step per update-step through DataParallelLearner.update_step):
  off      -- no guard: the launches of the commit before the guard existed (the comparison base);
  target   -- trust = 1, anchors given, target_kl so high that the latch never sets, no penalty: the KL launch and the gated apply;
  penalty  -- the same with kl_penalty > 0: the KL launch also adds its gradient to the head's dlin.
After warm-up, blocks of update-steps alternate over the configurations; each block is timed with HIP events on the launch stream
between two synchronizes, as bench.py times its region.  The off configuration's own block spread is the noise floor of the run: a
difference below it is not a difference.  Then, timed the same way: the anchor sweep (CARLANetwork.distribution_and_value's work:
inference forwards of `--sweep-rows` rows in chunks of B through one engine over the same arenas) and cdrl_beta_kl alone on the
policy head's linear outputs.  The first measured pass's kl_last is the step-0 floor that the BatchNorm modes put between the acting
forward (moving statistics) and the training forward (batch statistics) of the SAME weights: target_kl values are meaningful only
above it.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_trust.py [--batch 256] [--blocks 5 --steps 40 --warmup 3] [--out profiles/r20_trust_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [('off', dict(), dict()), ('target', dict(trust=True), dict(target_kl=1e30, kl_coef=0.0)),
           ('penalty', dict(trust=True), dict(target_kl=1e30, kl_coef=0.01))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--blocks', type=int, default=5, help='timed blocks per configuration (alternating)')
    ap.add_argument('--steps', type=int, default=40, help='update-steps per block')
    ap.add_argument('--warmup', type=int, default=3, help='untimed update-steps per configuration before the first block')
    ap.add_argument('--sweep-rows', type=int, default=2048, help='rows of the timed anchor sweep')
    ap.add_argument('--kl-reps', type=int, default=200, help='launches per block of the kernel-only timing')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()

    import torch
    from carla_driving_rl_agent_amd import _lib, synthetic
    from carla_driving_rl_agent_amd.engine import LearnerEngine, beta_kl, gae_returns
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    from carla_driving_rl_agent_amd.parallel import DataParallelLearner

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    B, T, H, W = args.batch, 4, 90, 120
    tags = [t for t, _, _ in CONFIGS]

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

    dps, batches, floor = {}, {}, {}
    for tag, kw, trust_hp in CONFIGS:
        eng = LearnerEngine(B, device=dev, T=T, H=H, W=W, **kw)
        init_engine_parameters(eng, seed=42)
        if trust_hp:
            eng.set_hparams(**trust_hp)
            # the anchor as update() forms it: the acting network (old_policy, moving statistics) on the rows, before any step
            acting = LearnerEngine(B, device=dev, share_with=eng, T=T, H=H, W=W)
            out = acting.predict(states)
            batches[tag] = dict(pol, anchor=torch.stack([out['alpha'], out['beta']], dim=1).contiguous())
            eng.policy_forward_backward_resample(batches[tag], seed=42, offset=0)       # measured, not applied: the step-0 floor
            floor[tag] = eng.trust_stats()['kl_last']
            eng.trust_reset()
        else:
            batches[tag] = pol
        dps[tag] = DataParallelLearner(eng)

    step_no = {t: 0 for t in tags}

    def run(tag, n):
        for _ in range(n):
            step_no[tag] += 1
            dps[tag].update_step(batches[tag], val, resample=(42, step_no[tag]))

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
    trust = {}
    for tag in tags:
        e = dps[tag].engine
        assert torch.isfinite(e.params).all(), tag
        if e.trust:
            st = e.trust_stats()
            assert st['stop'] == 0 and st['skipped'] == 0 and st['passes'] == step_no[tag], (tag, st)
            trust[tag] = st

    # the anchor sweep: inference forwards in chunks of B through one engine over the arenas of the off learner
    sweep = LearnerEngine(B, device=dev, share_with=dps['off'].engine, T=T, H=H, W=W)
    chunks = max(1, (args.sweep_rows + B - 1) // B)

    def sweep_rows(_, n):
        for _ in range(n):
            for _ in range(chunks):
                sweep.predict(states)

    sweep_rows(None, 1)
    sweep_ms = [timed(sweep_rows, None, 3) for _ in range(args.blocks)]

    # the KL kernel alone, on the linear outputs the last pass left
    eng = dps['penalty'].engine
    lin = eng.buffer(_lib.BUF_LIN_P, (B, 2 * eng.cfg.A + 2)).clone()
    dlin = torch.zeros_like(lin)
    metrics = torch.empty(3, dtype=torch.float32, device=dev)
    anchor = batches['penalty']['anchor']

    def kl_only(coef, n):
        for _ in range(n):
            beta_kl(lin, anchor, coef, 1.0, dlin, metrics)

    kl_only(0.01, 5)
    kl_ms = {name: [timed(kl_only, coef, args.kl_reps) for _ in range(args.blocks)] for name, coef in (('measure', 0.0), ('penalty', 0.01))}

    out = dict(metric='trust_update_step', batch=B, image=[T, H, W, 3], dtype='f32', blocks=args.blocks, steps_per_block=args.steps,
               warmup=args.warmup, configs={}, kl_floor_step0={t: floor[t] for t in floor},
               anchor_sweep=dict(rows=chunks * B, chunk=B, ms=round(statistics.median(sweep_ms), 4), ms_blocks=[round(t, 4) for t in sweep_ms]),
               beta_kl_kernel_ms={k: dict(ms=round(statistics.median(v), 5), ms_blocks=[round(t, 5) for t in v]) for k, v in kl_ms.items()},
               beta_kl_kernel_note='back-to-back launches timed with events: launch-to-launch time, an upper bound of the device time')
    base = statistics.median(times['off'])
    for tag, kw, trust_hp in CONFIGS:
        ms = statistics.median(times[tag])
        out['configs'][tag] = dict(options=dict(kw, **trust_hp), ms_per_update_step=round(ms, 4), ms_blocks=[round(t, 4) for t in times[tag]],
                                   block_spread_ms=round(max(times[tag]) - min(times[tag]), 4), ms_over_off=round(ms - base, 4),
                                   ratio_over_off=round(ms / base, 4), trust_stats=trust.get(tag))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

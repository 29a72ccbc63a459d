"""Update-step time with the train-stats ring (cdrl_config.train_stats, LearnerEngine(train_stats=N)) off and on, in ONE process.

Two learners over the same seeded weights and the same rollout minibatch (bench.py's inputs: B samples of 4 x 90 x 120 x 3,
re-sampled Beta-PPO policy loss, one policy + one value minibatch step per update-step through DataParallelLearner.update_step),
one with the ring off, one with a ring of --rows rows.  After warm-up, blocks of update-steps alternate over the two; each block
is timed with HIP events on the launch stream between two synchronizes, as bench.py times its region.  Then the apply steps alone
(policy_apply + value_apply on the gradients the last pass left) are timed the same way.  The ring is emptied (no host copy)
between blocks, so the timed region holds no device-to-host transfer; one fetch at the end is timed on the host clock.
What the ring adds per update-step: one extra read of the trunk gradient per apply (2 x 4 B x trunk elements), the chunk
partials, and two rows.  Prints one JSON line.

    python tools/bench_train_stats.py [--batch 256] [--rows 256] [--blocks 4 --steps 8 --warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--rows', type=int, default=256, help='ring rows of the ring-on learner')
    ap.add_argument('--blocks', type=int, default=4, help='timed blocks per configuration (alternating)')
    ap.add_argument('--steps', type=int, default=8, help='update-steps per block')
    ap.add_argument('--warmup', type=int, default=3, help='untimed update-steps per configuration before the first block')
    ap.add_argument('--apply-reps', type=int, default=20, help='apply pairs per block of the apply-only timing')
    args = ap.parse_args()

    import torch
    from carla_driving_rl_agent_amd import synthetic
    from carla_driving_rl_agent_amd.engine import LearnerEngine, gae_returns
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    from carla_driving_rl_agent_amd.parallel import DataParallelLearner

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    B, T, H, W = args.batch, 4, 90, 120
    tags = ['ring_off', 'ring_on']
    dps = {}
    for tag, rows in zip(tags, (0, args.rows)):
        eng = LearnerEngine(B, device=dev, T=T, H=H, W=W, train_stats=rows)
        init_engine_parameters(eng, seed=42)
        dps[tag] = DataParallelLearner(eng)
    on = dps['ring_on'].engine
    n_elems = {m: on.region(m, True)[1] for m in ('trunk', 'policy', 'value')}
    lay = on.train_stats_layout

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
    # same seed, same inputs, same launch sequence up to the ring's own kernels: the two learners hold the same bits
    identical = all(torch.equal(getattr(dps['ring_off'].engine, a), getattr(on, a)) for a in ('params', 'grads', 'adam_m', 'adam_v'))
    times = {t: [] for t in tags}
    for _ in range(args.blocks):
        for tag in tags:
            times[tag].append(timed(run, tag, args.steps))
        on.train_stats_reset()
    for tag in tags:
        assert torch.isfinite(dps[tag].engine.params).all(), tag
    apply_times = {t: [] for t in tags}
    for tag in tags:
        applies(tag, 2)
    for _ in range(args.blocks):
        for tag in tags:
            apply_times[tag].append(timed(applies, tag, args.apply_reps))
        on.train_stats_reset()
    run('ring_on', 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = on.train_stats()
    fetch_ms = (time.perf_counter() - t0) * 1e3
    assert len(stats['rows']) == 4 and stats['dropped'] == 0, (len(stats['rows']), stats['dropped'])

    ms = {t: statistics.median(times[t]) for t in tags}
    ams = {t: statistics.median(apply_times[t]) for t in tags}
    extra_bytes = 2 * (4 * n_elems['trunk'] + 8 * ((n_elems['trunk'] + 1023) // 1024) + 4 * lay['width'])
    out = dict(metric='train_stats_update_step', batch=B, image=[T, H, W, 3], dtype='f32', ring_rows=args.rows, row_floats=lay['width'],
               blocks=args.blocks, steps_per_block=args.steps, warmup=args.warmup, apply_pairs_per_block=args.apply_reps,
               trainable_elems=n_elems, bit_identical_after_warmup=bool(identical),
               ms_per_update_step={t: round(ms[t], 4) for t in tags}, ms_blocks={t: [round(x, 4) for x in times[t]] for t in tags},
               ring_on_over_off=round(ms['ring_on'] / ms['ring_off'], 4),
               apply_ms_per_update_step={t: round(ams[t], 4) for t in tags},
               apply_ms_blocks={t: [round(x, 4) for x in apply_times[t]] for t in tags},
               apply_added_us_per_update_step=round((ams['ring_on'] - ams['ring_off']) * 1e3, 2),
               added_bytes_per_update_step=extra_bytes,
               added_bytes_at_measured_added_time_GBps=(round(extra_bytes / max((ams['ring_on'] - ams['ring_off']) * 1e-3, 1e-9) / 1e9, 1)
                                                        if ams['ring_on'] > ams['ring_off'] else None),
               fetch_and_decode_ms_host_clock=round(fetch_ms, 3))
    print(json.dumps(out))


if __name__ == '__main__':
    main()

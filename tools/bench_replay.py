"""What reusing kept rollouts costs (PPOAgent(replay_rollouts=K)), in ONE process:

 (a) cdrl_vtrace_segments against cdrl_gae_returns_segments, the closest kernel the project had, at the same (S, N): S equal
     trajectories, N rows in all, A = 3; both through the C entry points on preallocated buffers, so a time is launch + kernel.
 (b) the refresh of one kept period (CARLAgent.refresh_replay: inference forwards over its rows in chunks of batch_size, one more for
     the truncated trajectories' final observations, the padded layout, one V-trace launch) against the minibatch steps the period's
     rows add to the update (rows / batch_size policy steps and as many value steps, stored-action loss).

After warm-up, blocks of the two sides alternate; each block is timed with HIP events on the launch stream between two synchronizes;
the figure of a side is the median of its blocks.  Writes one JSON file.  Refuses to run under a wrong-result diagnostic switch.

    python tools/bench_replay.py
    python tools/bench_replay.py --sizes 8:512 --rows 512 --batch 64 --blocks 2        (a quick look)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed_blocks(sides, blocks, warmup):
    """sides: name -> callable running one block's work.  -> name -> list of block times in ms."""
    import torch
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(blocks):
        for name, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return times


def _summary(times, per):
    out = {}
    for name, ts in times.items():
        out[f'{name}_ms'] = round(statistics.median(ts) / per[name], 5)
        out[f'{name}_ms_blocks'] = [round(t / per[name], 5) for t in ts]
        out[f'{name}_block_spread_ms'] = round((max(ts) - min(ts)) / per[name], 5)
    return out


def bench_kernels(S, N, args):
    import numpy as np
    import torch
    from carla_driving_rl_agent_amd import _lib
    lib = _lib.load()
    A, dev = 3, 'cuda:0'
    n = N // S
    assert n * S == N, (S, N)
    rng = np.random.default_rng(S)
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    rewards = f(rng.uniform(0, 10, N + S))
    values_be = f(np.stack([rng.uniform(-1, 1, N + S), rng.uniform(0, 2, N + S)], 1))
    alpha, beta = f(rng.uniform(1, 6, (N, A))), f(rng.uniform(1, 6, (N, A)))
    actions = f(rng.uniform(0.01, 0.99, (N, A)))
    log_prob_old = f(rng.normal(0.0, 0.5, (N, A)))
    seg_off = torch.arange(0, N + 1, n, dtype=torch.int32, device=dev)
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    ret, ret_be, raw, adv, rho = e(N), e(N, 2), e(N), e(N), e(N)
    s_gae = torch.empty(int(lib.cdrl_gae_segments_scratch_doubles(N, S)), dtype=torch.float64, device=dev)
    s_vt = torch.empty(int(lib.cdrl_vtrace_segments_scratch_doubles(N, S)), dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = _lib.ptr

    def gae():
        for _ in range(args.launches):
            _lib.check(lib.cdrl_gae_returns_segments(p(rewards), p(values_be), p(seg_off), S, N, 0.9999, 0.999, 2.0, p(ret), p(ret_be),
                                                     p(raw), p(adv), p(s_gae), stream), 'gae')

    def vtrace():
        for _ in range(args.launches):
            _lib.check(lib.cdrl_vtrace_segments(p(rewards), p(values_be), p(alpha), p(beta), p(actions), p(log_prob_old), p(seg_off), S, N,
                                                A, 0.9999, 0.999, 1.0, 1.0, 2.0, p(ret), p(ret_be), p(raw), p(adv), p(rho), p(s_vt),
                                                stream), 'vtrace')

    times = _timed_blocks(dict(gae_segments=gae, vtrace_segments=vtrace), args.blocks, warmup=1)
    out = dict(S=S, N=N, A=A, rows_per_trajectory=n, launches_per_block=args.launches)
    out.update(_summary(times, dict(gae_segments=args.launches, vtrace_segments=args.launches)))
    out['ratio_vtrace_over_gae'] = round(out['vtrace_segments_ms'] / out['gae_segments_ms'], 3)
    assert torch.isfinite(adv).all() and torch.isfinite(ret).all()
    return out


def bench_refresh(args):
    import numpy as np
    import torch
    from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.rl.replay import ReplayPeriod
    T, H, W, rows, B = 4, 90, 120, args.rows, args.batch
    assert rows % B == 0
    env = FakeCARLAEnvironment(image_shape=(H, W, 3), time_horizon=T, num_actions=3)
    agent = CARLAgent(env, batch_size=B, log_mode=None, seed=42, aug_intensity=0.0, resample_actions=False, replay_rollouts=1,
                      weights_dir=os.path.join(args.scratch, 'weights'), name='bench_replay')
    dev = agent.device
    rng = np.random.default_rng(1)
    spec = agent.state_spec
    keys = ('state_image', 'state_road', 'state_vehicle', 'state_navigation')
    rand = lambda n, k: torch.as_tensor(rng.uniform(0, 1, (n, T) + tuple(spec[k])).astype(np.float32)).to(dev)
    trajectories = [(B, s % 2 == 0) for s in range(rows // B)]            # every second trajectory truncated
    truncated = sum(1 for _, terminal in trajectories if not terminal)
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    period = ReplayPeriod({k: rand(rows, k) for k in keys}, f(rng.uniform(0.05, 0.95, (rows, 3))), f(rng.normal(0.0, 0.3, (rows, 3))),
                          f(rng.uniform(0, 10, rows)), trajectories, {k: rand(truncated, k) for k in keys},
                          info=dict(speed=f(rng.uniform(0, 0.3, rows)), similarity=f(rng.uniform(-1, 1, rows))))
    agent.replay.add(period)
    agent.network.set_hparams(**agent.hyper_parameters())

    def refresh():
        agent.refresh_replay()

    def steps():
        t = period.targets
        for lo in range(0, rows, B):
            cut = lambda x: x[lo:lo + B]
            states = {k: cut(v) for k, v in period.states.items()}
            _, grads = agent.get_policy_gradients((states, cut(t['advantages']), cut(period.actions), cut(period.log_probs),
                                                   cut(period.info['speed']), cut(period.info['similarity'])))
            agent.update_policy(grads)
        for lo in range(0, rows, B):
            cut = lambda x: x[lo:lo + B]
            states = {k: cut(v) for k, v in period.states.items()}
            _, grads = agent.get_value_gradients((states, cut(t['returns_be']), cut(period.info['speed']), cut(period.info['similarity'])))
            agent.update_value(grads)

    refresh()                                                               # (the targets `steps` reads)
    times = _timed_blocks(dict(refresh=refresh, added_minibatch_steps=steps), args.blocks, warmup=2)
    out = dict(rows=rows, batch_size=B, image=[T, H, W, 3], trajectories=len(trajectories), truncated=truncated,
               minibatch_steps=dict(policy=rows // B, value=rows // B))
    out.update(_summary(times, dict(refresh=1, added_minibatch_steps=1)))
    out['refresh_share_of_added_work'] = round(out['refresh_ms'] / out['added_minibatch_steps_ms'], 4)
    assert torch.isfinite(agent.network.engine.params).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='+', default=['8:512', '32:2048', '128:8192'], metavar='S:N')
    ap.add_argument('--launches', type=int, default=500, help='kernel launches per timed block (part a)')
    ap.add_argument('--rows', type=int, default=2048, help='rows of the kept period (part b)')
    ap.add_argument('--batch', type=int, default=256, help='batch_size of the agent (part b)')
    ap.add_argument('--blocks', type=int, default=5, help='timed blocks per side (alternating)')
    ap.add_argument('--skip-refresh', action='store_true')
    ap.add_argument('--scratch', default=None, help='directory for the agent of part (b) (default: a temporary one)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r19_replay_bench.json'))
    args = ap.parse_args()

    import torch
    from carla_driving_rl_agent_amd import _lib
    if _lib.diag_active():
        raise SystemExit(f'[bench_replay] refusing to benchmark: wrong-result diagnostic switches are active ({_lib.env_overrides()})')
    if not torch.cuda.is_available():
        raise SystemExit('[bench_replay] needs a GPU')
    torch.cuda.set_device(0)
    out = dict(metric='rollout_reuse_cost', device=torch.cuda.get_device_name(0), blocks=args.blocks, env_overrides=_lib.env_overrides(),
               note='one process; blocks of the two sides alternate; medians of the blocks; HIP events between two synchronizes; '
                    'kernels: ms per launch through the C entry points; refresh: ms per refresh / per pass over the added minibatch steps',
               kernels=[bench_kernels(*(int(x) for x in size.split(':')), args) for size in args.sizes])
    if not args.skip_refresh:
        with tempfile.TemporaryDirectory() as tmp:
            args.scratch = args.scratch or tmp
            out['refresh'] = bench_refresh(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

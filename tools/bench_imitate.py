"""Behaviour-cloning minibatch step (engine.clone_step) against the existing step it shares everything but the loss launch with, in
ONE process on ONE engine (B = 256, 4 x 90 x 120 x 3, float32):

    clone          clone_forward_backward + policy_apply           vs   policy   policy_forward_backward (stored action) + policy_apply
    clone_returns  clone_forward_backward (returns) + joint_apply  vs   joint    joint_forward_backward (stored action) + joint_apply

After warm-up, blocks of the four modes alternate; each block is timed with HIP events on the launch stream between two
synchronizes, as bench.py times its region.  Also timed: what imitate() pays ONCE PER TRACE at N = 512 rows -- the upload of the
per-step rows and the windowing gather that stacks them over the time horizon (wall clock around a synchronize).  Writes one JSON
file; refuses to run under a wrong-result diagnostic switch.

    python tools/bench_imitate.py
    python tools/bench_imitate.py --blocks 8 --steps 10 --out profiles/r16_imitate_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ('policy', 'clone', 'joint', 'clone_returns')
PAIRS = (('clone', 'policy'), ('clone_returns', 'joint'))


def bench_steps(args):
    import torch
    from carla_driving_rl_agent_amd import synthetic
    from carla_driving_rl_agent_amd.engine import LearnerEngine, gae_returns
    from carla_driving_rl_agent_amd.init import init_engine_parameters

    dev = 'cuda:0'
    B, T, H, W = args.batch, 4, 90, 120
    eng = LearnerEngine(B, device=dev, T=T, H=H, W=W)
    init_engine_parameters(eng, seed=42)
    r = synthetic.make_rollout(B, T=T, H=H, W=W, seed=42)
    states = {k: torch.as_tensor(v).to(dev) for k, v in r['states'].items()}
    rewards = torch.cat([torch.as_tensor(r['reward']).to(dev), torch.zeros(1, device=dev)])
    values = torch.cat([torch.as_tensor(r['value']).to(dev), torch.zeros((1, 2), device=dev)])
    hp = synthetic.DEFAULT_HP
    _, returns_be, _, adv = gae_returns(rewards, values, hp['gamma'], hp['lambda_'], hp['advantage_scale'])
    speed = (torch.as_tensor(r['speed'][:, 0]) / 100.0).to(dev).contiguous()
    sim = torch.as_tensor(r['similarity'][:, 0]).to(dev).contiguous()
    u = torch.as_tensor(r['action']).to(dev)
    pol = dict(states=states, advantages=adv.contiguous(), old_log_prob=torch.as_tensor(r['old_log_prob']).to(dev), speed=speed,
               similarity=sim, u=u, du_da=None, du_db=None)
    joint = dict(pol, returns=returns_be.contiguous())
    clone = dict(states=states, u=u, speed=speed, similarity=sim)
    clone_returns = dict(clone, returns=joint['returns'])

    def run(mode, n):
        for _ in range(n):
            if mode == 'policy':
                eng.policy_step(pol)
            elif mode == 'joint':
                eng.joint_step(joint)
            elif mode == 'clone':
                eng.clone_step(clone)
            else:
                eng.clone_step(clone_returns, value_weight=0.5)

    for mode in MODES:
        run(mode, args.warmup)
    torch.cuda.synchronize()
    times = {m: [] for m in MODES}
    for _ in range(args.blocks):
        for mode in MODES:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run(mode, args.steps)
            e1.record()
            torch.cuda.synchronize()
            times[mode].append(e0.elapsed_time(e1) / args.steps)
    assert torch.isfinite(eng.params).all()
    out = dict(batch=B, image=[T, H, W, 3], dtype='f32')
    for mode in MODES:
        out[f'{mode}_ms_per_step'] = round(statistics.median(times[mode]), 4)
        out[f'{mode}_ms_blocks'] = [round(t, 4) for t in times[mode]]
        out[f'{mode}_block_spread_ms'] = round(max(times[mode]) - min(times[mode]), 4)
    for new, old in PAIRS:
        diff = out[f'{new}_ms_per_step'] - out[f'{old}_ms_per_step']
        out[f'{new}_minus_{old}_ms'] = round(diff, 4)
        out[f'{new}_inside_the_spread_of_{old}'] = bool(min(times[old]) <= out[f'{new}_ms_per_step'] <= max(times[old]))
    del eng
    torch.cuda.empty_cache()
    return out


def bench_trace(args):
    """Upload of N per-step rows of every state key plus one windowing gather per key (T = 4): the once-per-trace cost of imitate()."""
    import numpy as np
    import torch
    from carla_driving_rl_agent_amd import traces
    from carla_driving_rl_agent_amd.rl import utils

    dev = 'cuda:0'
    N, T, H, W = args.trace_rows, 4, 90, 120
    rng = np.random.default_rng(0)
    host = dict(state_image=rng.uniform(-1, 1, (N, H, W, 3)).astype(np.float32), state_road=rng.uniform(0, 1, (N, 9)).astype(np.float32),
                state_vehicle=rng.uniform(0, 1, (N, 5)).astype(np.float32), state_navigation=rng.uniform(0, 25, (N, 10)).astype(np.float32))
    upload, gather = [], []
    for _ in range(args.trace_repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        devs = {k: torch.as_tensor(v).to(dev) for k, v in host.items()}
        index = torch.as_tensor(traces.window_index(N, T)).to(dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        stacked = {k: utils.gather_rows(v, index).view((N, T) + tuple(v.shape[1:])) for k, v in devs.items()}
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        upload.append(1e3 * (t1 - t0))
        gather.append(1e3 * (t2 - t1))
        assert stacked['state_image'].shape == (N, T, H, W, 3)
        del devs, stacked
    upload, gather = upload[1:], gather[1:]         # (the first round pays the allocations)
    return dict(rows=N, time_horizon=T, image=[H, W, 3], host_megabytes=round(sum(v.nbytes for v in host.values()) / 2 ** 20, 1),
                upload_ms=round(statistics.median(upload), 3), window_gather_ms=round(statistics.median(gather), 3),
                upload_ms_runs=[round(t, 3) for t in upload], window_gather_ms_runs=[round(t, 3) for t in gather])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--blocks', type=int, default=6, help='timed blocks per mode (alternating)')
    ap.add_argument('--steps', type=int, default=10, help='minibatch steps per block')
    ap.add_argument('--warmup', type=int, default=5, help='untimed steps per mode before the first block')
    ap.add_argument('--trace-rows', type=int, default=512)
    ap.add_argument('--trace-repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_imitate_bench.json'))
    args = ap.parse_args()

    import torch
    from carla_driving_rl_agent_amd import _lib
    if _lib.diag_active():
        raise SystemExit(f'[bench_imitate] refusing to benchmark: wrong-result diagnostic switches are active ({_lib.env_overrides()})')
    if not torch.cuda.is_available():
        raise SystemExit('[bench_imitate] needs a GPU')
    torch.cuda.set_device(0)
    out = dict(metric='clone_step_vs_existing_step', device=torch.cuda.get_device_name(0), blocks=args.blocks, steps_per_block=args.steps,
               warmup=args.warmup, env_overrides=_lib.env_overrides(),
               note='one process, one engine; blocks of the four modes alternate; ms per minibatch step (pass + apply); HIP events '
                    'between two synchronizes; per_trace: wall clock around a synchronize',
               steps=bench_steps(args), per_trace=bench_trace(args))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

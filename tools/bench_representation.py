"""Representation minibatch step (engine.repr_step: trunk forward, NT-Xent, trunk backward, trunk-only apply) against the
stored-action policy step (engine.policy_step), which does everything the representation step does plus the policy head, in ONE
process:

    B = 256   float32     4 x 90 x 120 x 3
    B = 1024  bf16s       4 x 90 x 120 x 3

Per shape one engine; after warm-up, blocks of the two modes alternate; each block is timed with HIP events on the launch stream
between two synchronizes, as bench.py times its region.  Also timed: the device time of the NT-Xent launches alone
(cdrl_ntxent_loss on (B, 512) embeddings) at B = 256 and B = 2048.  Writes one JSON file; refuses to run under a wrong-result
diagnostic switch.

    python tools/bench_representation.py
    python tools/bench_representation.py --blocks 6 --steps 10 --out profiles/r17_representation_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ('policy', 'representation')
SHAPES = ((256, 'f32'), (1024, 'bf16s'))
LOSS_ROWS = (256, 2048)


def bench_steps(args, B, compute):
    import torch
    from carla_driving_rl_agent_amd import synthetic
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    from carla_driving_rl_agent_amd.init import init_engine_parameters

    dev = 'cuda:0'
    T, H, W = 4, 90, 120
    eng = LearnerEngine(B, device=dev, T=T, H=H, W=W, compute=compute)
    init_engine_parameters(eng, seed=42)
    r = synthetic.make_rollout(B // 2, T=T, H=H, W=W, seed=42)
    # two views: the rows stacked twice, the second copy's images darkened (the step's cost does not depend on the values)
    states = {k: torch.as_tensor(v).to(dev) for k, v in r['states'].items()}
    states = {k: torch.cat([v, 0.8 * v if k == 'state_image' else v], dim=0).contiguous() for k, v in states.items()}
    rep = lambda a: torch.cat([torch.as_tensor(a).to(dev)] * 2, dim=0).contiguous()
    pol = dict(states=states, advantages=rep(r['value'][:, 0]), old_log_prob=rep(r['old_log_prob']), speed=rep(r['speed'][:, 0]) / 100.0,
               similarity=rep(r['similarity'][:, 0]), u=rep(r['action']), du_da=None, du_db=None)

    def run(mode, n):
        for _ in range(n):
            if mode == 'policy':
                eng.policy_step(pol)
            else:
                eng.repr_step(states, args.temperature)

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
    out = dict(batch=B, image=[T, H, W, 3], compute=compute, representation_loss=round(eng.metrics('representation')['loss'], 6))
    for mode in MODES:
        out[f'{mode}_ms_per_step'] = round(statistics.median(times[mode]), 4)
        out[f'{mode}_ms_blocks'] = [round(t, 4) for t in times[mode]]
        out[f'{mode}_block_spread_ms'] = round(max(times[mode]) - min(times[mode]), 4)
    out['representation_minus_policy_ms'] = round(out['representation_ms_per_step'] - out['policy_ms_per_step'], 4)
    out['representation_not_slower_beyond_the_policy_spread'] = bool(out['representation_ms_per_step'] <= max(times['policy']))
    del eng
    torch.cuda.empty_cache()
    return out


def bench_loss(args, B, D=512):
    """Device time of the five NT-Xent launches on (B, D) embeddings: HIP events around `reps` calls, median over blocks."""
    import numpy as np
    import torch
    from carla_driving_rl_agent_amd import _lib
    import ctypes as C

    dev = 'cuda:0'
    lib = _lib.load()
    rng = np.random.default_rng(B)
    z = torch.as_tensor(rng.standard_normal((B, D)).astype(np.float32)).to(dev)
    ws = torch.empty(int(lib.cdrl_ntxent_workspace_floats(B, D)), device=dev)
    dz, metrics = torch.empty_like(z), torch.empty(16, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: _lib.check(lib.cdrl_ntxent_loss(_lib.ptr(z), B, D, args.temperature, 1.0, _lib.ptr(dz), _lib.ptr(metrics),
                                                   _lib.ptr(ws), stream), 'cdrl_ntxent_loss')
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    reps, blocks = 20, []
    for _ in range(args.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        blocks.append(e0.elapsed_time(e1) / reps)
    flop = 3 * 2.0 * B * B * D
    ms = statistics.median(blocks)
    return dict(rows=B, columns=D, workspace_megabytes=round(ws.numel() * 4 / 2 ** 20, 2), ms_per_call=round(ms, 4),
                ms_blocks=[round(t, 4) for t in blocks], gemm_shaped_gflop=round(flop / 1e9, 3),
                tflops=round(flop / (ms * 1e-3) / 1e12, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=6, help='timed blocks per mode (alternating)')
    ap.add_argument('--steps', type=int, default=10, help='minibatch steps per block')
    ap.add_argument('--warmup', type=int, default=5, help='untimed steps per mode before the first block')
    ap.add_argument('--temperature', type=float, default=0.1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r17_representation_bench.json'))
    args = ap.parse_args()

    import torch
    from carla_driving_rl_agent_amd import _lib
    if _lib.diag_active():
        raise SystemExit(f'[bench_representation] refusing to benchmark: wrong-result diagnostic switches are active ({_lib.env_overrides()})')
    if not torch.cuda.is_available():
        raise SystemExit('[bench_representation] needs a GPU')
    torch.cuda.set_device(0)
    out = dict(metric='repr_step_vs_policy_step', device=torch.cuda.get_device_name(0), blocks=args.blocks, steps_per_block=args.steps,
               warmup=args.warmup, temperature=args.temperature, env_overrides=_lib.env_overrides(),
               note='one process; per shape one engine, blocks of the two modes alternate; ms per minibatch step (pass + apply); HIP '
                    'events between two synchronizes; loss: the NT-Xent launches alone, 20 calls per block',
               steps=[bench_steps(args, B, compute) for B, compute in SHAPES], loss=[bench_loss(args, B) for B in LOSS_ROWS])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

"""Demonstration-augmented policy step (engine.demo_step) against what it stands next to and what it replaces, in ONE process on
engines over ONE set of parameter arenas (4 x 90 x 120 x 3, float32, stored actions):

    policy   (a) policy_forward_backward + policy_apply on B fresh rows                                     (B = 256)
    mixed    (b) demo_forward_backward + policy_apply on B - D fresh rows followed by D demonstration rows   (192 + 64)
    split    (c) policy step on B - D fresh rows, then clone_step on D demonstration rows: two trunk passes, two trunk optimizer
                 steps, two old_policy copies -- the only way to train on both kinds before the mixed pass existed

After warm-up, blocks of the three modes alternate; each block is timed with HIP events on the launch stream between two
synchronizes, as bench.py times its region.  Also timed: the loss launch alone, cdrl_beta_mixed_policy_loss against
cdrl_beta_ppo_loss on the same (B, 2A + 2) head outputs (both entries upload the same 64-byte hyper-parameter block in front of
their kernel).  Writes one JSON file; refuses to run under a wrong-result diagnostic switch.

    python tools/bench_demo.py
    python tools/bench_demo.py --blocks 8 --steps 10 --out profiles/r22_demo_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ('policy', 'mixed', 'split')


def _timed(torch, fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _summary(out, name, times):
    out[f'{name}_ms_per_step'] = round(statistics.median(times), 4)
    out[f'{name}_ms_blocks'] = [round(t, 4) for t in times]
    out[f'{name}_block_spread_ms'] = round(max(times) - min(times), 4)


def bench_steps(args):
    import torch
    from carla_driving_rl_agent_amd import synthetic
    from carla_driving_rl_agent_amd.engine import LearnerEngine, demo_block
    from carla_driving_rl_agent_amd.init import init_engine_parameters

    dev = 'cuda:0'
    B, D, T, H, W = args.batch, args.demo_rows, 4, 90, 120
    F = B - D
    eng = LearnerEngine(B, device=dev, T=T, H=H, W=W)
    init_engine_parameters(eng, seed=42)
    fresh_eng = LearnerEngine(F, device=dev, share_with=eng, T=T, H=H, W=W)
    demo_eng = LearnerEngine(D, device=dev, share_with=eng, T=T, H=H, W=W)
    r = synthetic.make_rollout(B, T=T, H=H, W=W, seed=42)
    g = torch.Generator().manual_seed(42)
    up = lambda a: torch.as_tensor(a).to(dev).contiguous()
    states = {k: up(v) for k, v in r['states'].items()}
    adv = up(torch.randn(B, generator=g))
    speed, sim = up(r['speed'][:, 0] / 100.0), up(r['similarity'][:, 0])
    u, old = up(r['action']), up(r['old_log_prob'])
    demo_w = torch.zeros(B, device=dev)
    demo_w[F:] = args.demo_weight
    pol = dict(states=states, advantages=adv, old_log_prob=old, speed=speed, similarity=sim, u=u, du_da=None, du_db=None)
    mixed = dict(pol, demo_u=u, demo_w=demo_w)
    rows = lambda t, s: t[s].contiguous()
    head, tail = slice(0, F), slice(F, B)
    pol_fresh = dict(states={k: rows(v, head) for k, v in states.items()}, advantages=rows(adv, head), old_log_prob=rows(old, head),
                     speed=rows(speed, head), similarity=rows(sim, head), u=rows(u, head), du_da=None, du_db=None)
    clone_demo = dict(states={k: rows(v, tail) for k, v in states.items()}, u=rows(u, tail), speed=rows(speed, tail),
                      similarity=rows(sim, tail), weight=rows(demo_w, tail))
    eng.set_demo_block(demo_block(dev))

    def split():
        fresh_eng.policy_step(pol_fresh)
        demo_eng.clone_step(clone_demo)

    step = dict(policy=lambda: eng.policy_step(pol), mixed=lambda: eng.demo_step(mixed), split=split)
    for mode in MODES:
        for _ in range(args.warmup):
            step[mode]()
    torch.cuda.synchronize()
    times = {m: [] for m in MODES}
    for _ in range(args.blocks):
        for mode in MODES:
            times[mode].append(_timed(torch, step[mode], args.steps))
    assert torch.isfinite(eng.params).all()
    out = dict(batch=B, fresh_rows=F, demo_rows=D, image=[T, H, W, 3], dtype='f32')
    for mode in MODES:
        _summary(out, mode, times[mode])
    out['mixed_minus_policy_ms'] = round(out['mixed_ms_per_step'] - out['policy_ms_per_step'], 4)
    out['mixed_inside_the_spread_of_policy'] = bool(min(times['policy']) <= out['mixed_ms_per_step'] <= max(times['policy']))
    out['mixed_over_split'] = round(out['mixed_ms_per_step'] / out['split_ms_per_step'], 4)
    del eng, fresh_eng, demo_eng
    torch.cuda.empty_cache()
    return out


def bench_loss(args):
    """The loss launch alone on random head outputs: the mixed loss with D demonstration rows, the mixed loss with none, and the
    policy loss."""
    import torch
    from carla_driving_rl_agent_amd import _lib

    lib = _lib.load()
    dev = 'cuda:0'
    B, D, A = args.batch, args.demo_rows, 2
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev).contiguous()
    uni = lambda *s: (torch.rand(*s, generator=g) * 0.98 + 0.01).to(dev).contiguous()
    lin, adv, old, speed, sim, u, demo_u = rnd(B, 2 * A + 2), rnd(B), rnd(B, A) * 0.3, uni(B), rnd(B).tanh(), uni(B, A), uni(B, A)
    demo_w, none = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    demo_w[B - D:] = args.demo_weight
    dlin, metrics, aux, hp = torch.empty_like(lin), torch.zeros(16, device=dev), torch.empty((B, 4 * A), device=dev), torch.zeros(16, device=dev)
    P = _lib.ptr
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (P(lin), P(adv), P(old), P(speed), P(sim), P(u), None, None)
    tail = (0.2, 0.01, B, A, 1.0, P(dlin), P(metrics), P(aux), P(hp))
    launch = dict(
        policy_loss=lambda: _lib.check(lib.cdrl_beta_ppo_loss(*head, *tail, stream())),
        mixed_loss=lambda: _lib.check(lib.cdrl_beta_mixed_policy_loss(*head, P(demo_u), P(demo_w), *tail, None, stream())),
        mixed_loss_no_demo_rows=lambda: _lib.check(lib.cdrl_beta_mixed_policy_loss(*head, P(demo_u), P(none), *tail, None, stream())))
    times = {k: [] for k in launch}
    for fn in launch.values():
        for _ in range(args.warmup):
            fn()
    for _ in range(args.blocks):
        for name, fn in launch.items():
            times[name].append(1e3 * _timed(torch, fn, args.loss_launches))
    out = dict(batch=B, demo_rows=D, actions=A, launches_per_block=args.loss_launches, unit='us per launch, back to back on one stream')
    for name in launch:
        out[f'{name}_us'] = round(statistics.median(times[name]), 2)
        out[f'{name}_us_blocks'] = [round(t, 2) for t in times[name]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--demo-rows', type=int, default=64, help='demonstration rows of the mixed minibatch (D)')
    ap.add_argument('--demo-weight', type=float, default=0.1)
    ap.add_argument('--blocks', type=int, default=6, help='timed blocks per mode (alternating)')
    ap.add_argument('--steps', type=int, default=10, help='minibatch steps per block')
    ap.add_argument('--warmup', type=int, default=5, help='untimed steps per mode before the first block')
    ap.add_argument('--loss-launches', type=int, default=200, help='loss launches per block')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r22_demo_bench.json'))
    args = ap.parse_args()
    if not 1 <= args.demo_rows < args.batch:
        raise SystemExit('[bench_demo] need 1 <= --demo-rows < --batch')

    import torch
    from carla_driving_rl_agent_amd import _lib
    if _lib.diag_active():
        raise SystemExit(f'[bench_demo] refusing to benchmark: wrong-result diagnostic switches are active ({_lib.env_overrides()})')
    if not torch.cuda.is_available():
        raise SystemExit('[bench_demo] needs a GPU')
    torch.cuda.set_device(0)
    out = dict(metric='demo_step_vs_policy_step_and_split_steps', device=torch.cuda.get_device_name(0), blocks=args.blocks,
               steps_per_block=args.steps, warmup=args.warmup, env_overrides=_lib.env_overrides(),
               note='one process, engines over one set of arenas; blocks of the three modes alternate; ms per minibatch step (pass + '
                    'apply); HIP events between two synchronizes.  Effect on learning or driving quality: not measured',
               steps=bench_steps(args), loss=bench_loss(args))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

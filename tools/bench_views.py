"""The two view builders of learn_representation() beside each other, in ONE process: view_pipeline 'agent' (draw_plans ->
Augmenter.batch on the rows stacked twice) and 'simclr' (draw_view_plans -> Augmenter.views).

Per view count (2N = 64 and 256 views of 4 x 90 x 120 x 3 by default) and per pipeline, after warm-up, in alternating blocks:
  host    drawing and packing one minibatch's plans (representation_plans + pack_plans / pack_view_plans): a host clock, no device work;
  device  the builder's device work with the plans already uploaded, enqueued back to back: 'agent' = the torch.cat of the image stacks +
          cdrl_augment_images_batch (five launches), 'simclr' = cdrl_views_batch (four launches); HIP events between two synchronizes;
  step    a whole learn_representation minibatch (plans, views, pass + trunk apply): a host clock around work that ends in a synchronize.
Each figure is the median of its blocks with the blocks' own spread (max - min).  For the new launches the achieved bytes/s against the
bytes they move (every launch reads and writes every view; the mean launch reads only the views that jitter) and against the least the
task needs (read the rows once, write the views once).  No ratio is asserted.  Refuses to run under a wrong-result diagnostic switch.

    python tools/bench_views.py
    python tools/bench_views.py --views 64 --blocks 3
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIPELINES = ('agent', 'simclr')
T, H, W = 4, 90, 120


def _summary(times):
    return dict(median_ms=round(statistics.median(times), 4), blocks_ms=[round(t, 4) for t in times],
                spread_ms=round(max(times) - min(times), 4))


def bench_views(V, args):
    import numpy as np
    import torch
    from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.rl import augmentations as aug

    dev = 'cuda:0'
    N = V // 2
    agents = {}
    for name in PIPELINES:
        env = FakeCARLAEnvironment(image_shape=(H, W, 3), time_horizon=T, image_range=(0.0, 1.0), seed=0)
        agents[name] = CARLAgent(env, batch_size=V, log_mode=None, seed=3, aug_intensity=0.0, name=f'bench_views_{name}',
                                 weights_dir=args.weights_dir, view_pipeline=name)
    gen = torch.Generator(device=dev).manual_seed(18)
    rows = {k: torch.rand((N, T) + tuple(agents['agent'].state_spec[k]), device=dev, generator=gen) for k in CARLAgent.STATE_KEYS}
    images = rows['state_image']
    n = T * H * W * 3
    rng = {name: np.random.default_rng(18) for name in PIPELINES}
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    lib = aug._lib.load()

    def host(name, steps):
        for _ in range(steps):
            plans = agents[name].representation_plans(1.0, rng[name], V, 1)
            packed = aug.pack_plans(plans) if name == 'agent' else aug.pack_view_plans(plans, H, W)
        return packed

    # fixed plans for the device figure, uploaded once
    packed = {name: host(name, 1) for name in PIPELINES}
    plans_dev = {name: torch.from_numpy(packed[name].view(np.uint8)).to(dev) for name in PIPELINES}
    ws = dict(agent=torch.empty(int(lib.cdrl_augment_batch_workspace_floats(V, T, H, W)), device=dev),
              simclr=torch.empty(int(lib.cdrl_views_workspace_floats(V, T, H, W)), device=dev))
    out = torch.empty((V, T, H, W, 3), device=dev)

    def device(name, steps):
        for _ in range(steps):
            if name == 'agent':
                twice = torch.cat([images, images], dim=0)
                aug._lib.check(lib.cdrl_augment_images_batch(ptr(twice), ptr(out), V, T, H, W, ptr(plans_dev[name]), ptr(ws[name]), stream()))
            else:
                aug._lib.check(lib.cdrl_views_batch(ptr(images), N, ptr(out), V, T, H, W, ptr(plans_dev[name]), ptr(ws[name]), stream()))

    def step(name, steps):
        agent = agents[name]
        for _ in range(steps):
            plans = agent.representation_plans(1.0, rng[name], V, 1)
            agent.representation_minibatch(agent.representation_views(rows, plans, 'zero'), 0.1)

    def timed_host(fn, name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(name, args.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    def timed_events(fn, name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn(name, args.steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    figures = dict(host=(host, timed_host), device=(device, timed_events), step=(step, timed_host))
    times = {(f, name): [] for f in figures for name in PIPELINES}
    for f, (fn, _) in figures.items():
        for name in PIPELINES:
            fn(name, args.warmup)
    torch.cuda.synchronize()
    for _ in range(args.blocks):
        for f, (fn, timer) in figures.items():
            for name in PIPELINES:
                times[(f, name)].append(timer(fn, name))
    for name in PIPELINES:
        assert torch.isfinite(agents[name].network.engine.params).all(), name

    res = dict(views=V, rows=N, image=[T, H, W, 3])
    for f in figures:
        for name in PIPELINES:
            res[f'{f}_{name}'] = _summary(times[(f, name)])
        res[f'{f}_simclr_minus_agent_ms'] = round(res[f'{f}_simclr']['median_ms'] - res[f'{f}_agent']['median_ms'], 4)
    jitter_share = float((packed['simclr']['jitter'] == 1).mean())
    moved = (6 + jitter_share) * V * n * 4            # launches 1, 3, 4 read and write every view; launch 2 reads the views that jitter
    least = (N + V) * n * 4
    secs = res['device_simclr']['median_ms'] * 1e-3
    res['simclr_launches'] = dict(launches=4, jitter_share_of_the_timed_plans=round(jitter_share, 4), bytes_moved=int(moved),
                                  bytes_least=int(least), achieved_TBps_of_bytes_moved=round(moved / secs / 1e12, 4),
                                  achieved_TBps_of_bytes_least=round(least / secs / 1e12, 4))
    res['agent_builder_doubled_copy_bytes'] = int(2 * V * n * 4)            # the torch.cat: reads N stacks twice, writes 2N
    del agents
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', nargs='+', type=int, default=[64, 256], help='views per minibatch (2N, even)')
    ap.add_argument('--blocks', type=int, default=5, help='timed blocks per figure and pipeline (alternating)')
    ap.add_argument('--steps', type=int, default=10, help='minibatches per block')
    ap.add_argument('--warmup', type=int, default=3, help='untimed minibatches per figure and pipeline before the first block')
    ap.add_argument('--weights-dir', default=os.path.join(ROOT, 'scratch', 'bench_views_weights'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r18_views_bench.json'))
    args = ap.parse_args()
    if any(v < 2 or v % 2 for v in args.views):
        raise SystemExit('[bench_views] --views: two views per row, so even and at least 2')

    import torch
    from carla_driving_rl_agent_amd import _lib
    if _lib.diag_active():
        raise SystemExit(f'[bench_views] refusing to benchmark: wrong-result diagnostic switches are active ({_lib.env_overrides()})')
    if not torch.cuda.is_available():
        raise SystemExit('[bench_views] needs a GPU')
    torch.cuda.set_device(0)
    out = dict(metric='representation_view_builders', device=torch.cuda.get_device_name(0), blocks=args.blocks,
               steps_per_block=args.steps, warmup=args.warmup, env_overrides=_lib.env_overrides(),
               note="one process; blocks of the two pipelines alternate; ms per minibatch; host: host clock, no device work; device: HIP "
                    "events between two synchronizes, plans uploaded beforehand ('agent' includes its torch.cat of the image stacks); "
                    "step: host clock around plans + views + representation pass and trunk apply, ending in a synchronize",
               results=[bench_views(v, args) for v in args.views])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

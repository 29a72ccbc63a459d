"""Time of one CARLAgent.explain() call on one 4 x 90 x 120 x 3 observation against the loop a user would write without it, in ONE
process with one agent.  Grids (6, 8) and (9, 12), per_frame off and on, chunk 32 and 64, modalities on: N = 1 + F*gh*gw + 4 rows in
ceil(N / chunk) inference forwards.

  explain     host clock around explain(...), ending in a device synchronise (the call's own host read of the four modality rows
              included)
  naive       per cell: clone the stack with torch, assign the baseline into the slice, one predict(deterministic=True) at E = 1,
              read alpha / beta / value on the host -- what explain() replaces; the unoccluded row and the four modality rows are
              run the same way, so both sides do N forwards' worth of rows
  launches    cdrl_occlusion_rows for one chunk, cdrl_occlusion_scores and cdrl_occlusion_maps alone: back-to-back launches between
              two device events (launch-to-launch time: an upper bound of the device time), and the bytes per second of the rows
              kernel from the bytes its algorithm moves (one read of the stack, `chunk` stacks written; the baseline is read only
              where a workgroup's span meets the cell, which is not counted)
  forwards    rollout_for(chunk).predict on a filled chunk alone, times ceil(N / chunk): what the call cannot avoid

Blocks alternate: every round times each configuration once, explain and naive in turn; one untimed round first (it builds the
engines for the chunk sizes and the chunk buffers).  Median (min, max) over the timed rounds.  Every block runs under its own time
limit (--limit seconds, SIGALRM).  The handler runs only when the interpreter has control again, so it ends a block that is slow, not
one that hangs inside a device call such as a synchronise: run the tool under an outer limit as well, as below.

    timeout -k 10 600 python tools/bench_explain.py [--rounds 5] [--naive-rounds 2] [--limit 120] [--out profiles/r21_explain_bench.json]
"""
import argparse
import json
import math
import os
import shutil
import signal
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(values, digits=3):
    return dict(median=round(statistics.median(values), digits), min=round(min(values), digits), max=round(max(values), digits))


class limit:
    """`with limit(seconds, what)`: the block raises TimeoutError when it runs longer."""

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _fire(self, *_):
        raise TimeoutError(f'{self.what}: longer than {self.seconds} s')

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5, help='timed rounds per explain configuration (one untimed first)')
    ap.add_argument('--naive-rounds', type=int, default=2, help='timed rounds of the per-cell loop (hundreds of forwards each)')
    ap.add_argument('--limit', type=int, default=120, help='seconds a single block may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_explain_bench.json'))
    args = ap.parse_args()

    import torch
    from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.engine import occlusion_baseline, occlusion_maps, occlusion_rows, occlusion_scores
    from carla_driving_rl_agent_amd.explain import occlusion_cells, occlusion_row_count

    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    torch.cuda.set_device(0)
    T, H, W = 4, 90, 120
    work = tempfile.mkdtemp(prefix='cdrl_bench_')
    env = FakeCARLAEnvironment(image_shape=(H, W, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=2,
                               image_range=(0.0, 1.0), seed=100)
    agent = CARLAgent(env, batch_size=64, log_mode=None, seed=5, aug_intensity=0.0, weights_dir=os.path.join(work, 'weights'),
                      evaluation_dir=os.path.join(work, 'evaluation'), name='bench_explain')
    state = agent.observe([env.reset()], agent.preprocess())
    keys = ('state_image', 'state_road', 'state_vehicle', 'state_navigation')
    one = {k: state[k][0].contiguous() for k in keys}
    A = agent.num_actions

    def run_explain(grid, per_frame, chunk):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = agent.explain(state, grid=grid, per_frame=per_frame, chunk=chunk)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def run_naive(grid, per_frame):
        """The per-cell loop: one E = 1 forward and one host read per row."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        base = state['state_image'][0].mean(dim=(1, 2), keepdim=True).expand(T, H, W, 3)
        rows = []

        def forward(st):
            _, mean, std, _, value = agent.predict(st, deterministic=True)
            rows.append([x.cpu().numpy() for x in (mean, std, value)])

        forward(state)
        for f in range(T if per_frame else 1):
            frames = slice(f, f + 1) if per_frame else slice(0, T)
            for (y0, y1, x0, x1) in occlusion_cells(H, W, grid[0], grid[1]):
                image = state['state_image'].clone()
                image[0, frames, y0:y1, x0:x1] = base[frames, y0:y1, x0:x1]
                forward(dict(state, state_image=image))
        forward(dict(state, state_image=base[None].contiguous()))
        for k in keys[1:]:
            forward(dict(state, **{k: torch.zeros_like(state[k])}))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, len(rows)

    def events(fn, reps):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    configs = [(grid, pf, chunk) for grid in ((6, 8), (9, 12)) for pf in (False, True) for chunk in (32, 64)]
    naive_configs = [(grid, pf) for grid in ((6, 8), (9, 12)) for pf in (False, True)]
    ms = {c: [] for c in configs}
    naive_ms = {c: [] for c in naive_configs}
    for k in range(args.rounds + 1):
        order = configs[k % len(configs):] + configs[:k % len(configs)]
        for i, (grid, pf, chunk) in enumerate(order):
            with limit(args.limit, f'explain {grid} per_frame={pf} chunk={chunk}'):
                dt, out = run_explain(grid, pf, chunk)
            assert tuple(out['scores'].shape) == ((T if pf else 1), grid[0], grid[1], 2 + A)
            if k:
                ms[(grid, pf, chunk)].append(dt)
            if k <= args.naive_rounds and i % 2 == 1:             # one naive block behind every second explain block
                nc = naive_configs[(i // 2) % len(naive_configs)]
                with limit(args.limit, f'naive {nc}'):
                    dt, n = run_naive(*nc)
                assert n == occlusion_row_count(T, nc[0][0], nc[0][1], nc[1], True)
                if k:
                    naive_ms[nc].append(dt)

    # the launches on their own
    base = occlusion_baseline(one['state_image'], 'mean')
    stack_bytes = T * H * W * 3 * 4
    launches = []
    with limit(args.limit, 'launches'):
        for chunk in (32, 64):
            bufs = {k: torch.empty((chunk,) + tuple(v.shape), device=agent.device) for k, v in one.items()}
            for grid, pf in naive_configs:
                t = [events(lambda: occlusion_rows(one['state_image'], base, one['state_road'], one['state_vehicle'],
                                                   one['state_navigation'], grid, pf, True, 1, bufs), 200) for _ in range(5)]
                moved = (chunk + 1) * stack_bytes
                launches.append(dict(kernel='occlusion_rows', grid=list(grid), per_frame=pf, chunk=chunk, ms=spread(t, 5),
                                     bytes=moved, gbytes_per_s=round(moved / (statistics.median(t) * 1e-3) / 1e9, 1),
                                     note='launch-to-launch time: where it does not grow with the bytes it is the launch floor, and '
                                          'gbytes_per_s a lower bound of the kernel\'s rate'))
            eng = agent.network.rollout_for(chunk)
            t = [events(lambda: eng.predict(bufs), 20) for _ in range(5)]
            launches.append(dict(kernel='inference forward', chunk=chunk, ms=spread(t, 4)))
        for grid, pf in naive_configs:
            F = T if pf else 1
            N = occlusion_row_count(T, grid[0], grid[1], pf, True)
            alpha, beta = (torch.rand((N, A), device=agent.device) * 20.0 + 1.01 for _ in range(2))
            value = torch.rand((N, 2), device=agent.device)
            scores = occlusion_scores(alpha, beta, value)
            t = [events(lambda: occlusion_scores(alpha, beta, value, out=scores), 200) for _ in range(5)]
            launches.append(dict(kernel='occlusion_scores', rows=N, ms=spread(t, 5)))
            for up in ('nearest', 'bilinear'):
                t = [events(lambda: occlusion_maps(scores, F, grid, (H, W), up, True), 200) for _ in range(5)]
                launches.append(dict(kernel='occlusion_maps', grid=list(grid), frames=F, upsample=up, ms=spread(t, 5),
                                     note='includes the allocation of the maps tensor by the wrapper'))

    forward_ms = {row['chunk']: row['ms']['median'] for row in launches if row['kernel'] == 'inference forward'}
    rows = []
    for grid, pf, chunk in configs:
        N = occlusion_row_count(T, grid[0], grid[1], pf, True)
        forwards = math.ceil(N / chunk)
        e = spread(ms[(grid, pf, chunk)])
        row = dict(grid=list(grid), per_frame=pf, chunk=chunk, rows=N, forwards=forwards, explain_ms=e,
                   forwards_alone_ms=round(forwards * forward_ms[chunk], 3),
                   share_of_forwards=round(forwards * forward_ms[chunk] / e['median'], 3))
        if naive_ms[(grid, pf)]:
            row['naive_ms'] = spread(naive_ms[(grid, pf)])
            row['speedup'] = round(row['naive_ms']['median'] / e['median'], 1)
        rows.append(row)
    chunk_bytes = {c: c * (stack_bytes + T * (9 + 4 + 5) * 4) for c in (32, 64)}
    out = dict(metric='explain', stack=[T, H, W, 3], timed_rounds=args.rounds, naive_rounds=args.naive_rounds,
               clock='host perf_counter around one call, ending in a device synchronise; launches: device events around back-to-back '
                     'launches; median (min, max), blocks alternating in one process',
               rows=rows, launches=launches,
               allocations=dict(chunk_buffers_bytes=chunk_bytes, per_call='alpha / beta / value (N, .), scores (N - 1, K) float64, '
                                'maps (K, F, H, W) float32, the baseline stack', first_use='one inference engine per chunk size '
                                '(rollout_for(chunk)) and the chunk buffers; both kept'))
    for row in rows + launches:
        print(json.dumps(row), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(dict(metric=out['metric'], written=os.path.relpath(args.out, ROOT))))


if __name__ == '__main__':
    main()

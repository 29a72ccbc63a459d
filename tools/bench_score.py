"""Time of scoring the acting policy on held-out rows (cdrl_beta_score, CARLAgent.score_traces), in ONE process with
one agent at 4 x 90 x 120 x 3, two actions.

  launch      cdrl_beta_score alone on the persistent predict outputs of rollout_for(chunk), chunk 32 and 256, with returns and
              auxiliary targets: back-to-back launches between two device events (launch-to-launch time: an upper bound of the
              device time), beside the same chunk's inference forward timed the same way, and their ratio
  score       host clock around score_traces(dir, aux=False) over 2048 rows in 8 trace files, ending in its one host read
  naive       the loop it replaces, on the same files: per trace distribution_and_value, three device-to-host copies, and the
              numpy / scipy restatement (tests/score_ref.py) on the host
  load        reading, checking and uploading the same files alone (what both sides share: numpy's decompression, the windowing
              gather, the returns launch)

Blocks alternate: every round times launch / forward per chunk and score / naive / load once each; one untimed round first (it builds
the engines).  Median (min, max) over the timed rounds.  Every block runs under its own time limit (--limit seconds, SIGALRM), which
ends a block that is slow, not one that hangs inside a device call: run the tool under an outer limit as well.

    timeout -k 10 600 python tools/bench_score.py [--rounds 5] [--rows 2048] [--limit 120] [--out profiles/r23_score_bench.json]
"""
import argparse
import json
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
    ap.add_argument('--rounds', type=int, default=5, help='timed rounds (one untimed first)')
    ap.add_argument('--rows', type=int, default=2048, help='rows of the held-out traces, in 8 files')
    ap.add_argument('--limit', type=int, default=120, help='seconds a single block may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r23_score_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    from carla_driving_rl_agent_amd import traces
    from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.engine import beta_score, score_block
    from tests import score_ref

    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    torch.cuda.set_device(0)
    T, H, W, A, CHUNK = 4, 90, 120, 2, 64
    work = tempfile.mkdtemp(prefix='cdrl_bench_')
    env = FakeCARLAEnvironment(image_shape=(H, W, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=A,
                               image_range=(0.0, 1.0), seed=100)
    agent = CARLAgent(env, batch_size=CHUNK, log_mode=None, seed=5, aug_intensity=0.0, weights_dir=os.path.join(work, 'weights'),
                      evaluation_dir=os.path.join(work, 'evaluation'), name='bench_score')
    net, dev = agent.network, agent.device
    rng = np.random.default_rng(7)

    # the held-out traces: per-step rows (the agent stacks the time_horizon axis on the device), images of 16 grey levels
    files, per = 8, args.rows // 8
    held = os.path.join(work, 'held_out')
    for k in range(files):
        image = (rng.integers(0, 16, (per, H, W, 3)) / 15.0).astype(np.float32)
        traces.write_trace(held, k + 1, dict(image=image, road=rng.random((per, 9), dtype=np.float32),
                                             vehicle=rng.random((per, 4), dtype=np.float32),
                                             navigation=rng.random((per, 5), dtype=np.float32)),
                           rng.uniform(-1.0, 1.0, (per, A)).astype(np.float32), rng.uniform(0.0, 1.0, per).astype(np.float32),
                           np.zeros(per, np.float32), dict(speed=rng.uniform(0.0, 30.0, per), similarity=rng.uniform(-1.0, 1.0, per)))

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

    def host(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def naive():
        prior = None
        for trace in traces.load_traces(held):
            data = agent._trace_tensors(trace, None, False, 1.0)
            alpha, beta, value = (x.cpu().numpy() for x in net.distribution_and_value(data['states'], chunk=CHUNK))
            value4 = np.concatenate([value, np.zeros_like(value)], axis=1)
            prior = score_ref.block(alpha, beta, value4, data['u'].cpu().numpy(), data['returns'].cpu().numpy(), prior=prior)
        return prior

    def load():
        for trace in traces.load_traces(held):
            agent._trace_tensors(trace, None, False, 1.0)

    chunks = {}
    for chunk in (32, 256):
        bufs = dict(state_image=torch.rand((chunk, T, H, W, 3), device=dev), state_road=torch.rand((chunk, T, 9), device=dev),
                    state_vehicle=torch.rand((chunk, T, 4), device=dev), state_navigation=torch.rand((chunk, T, 5), device=dev))
        eng = net.rollout_for(chunk)
        eng.predict(bufs)
        targets = dict(u=torch.rand((chunk, A), device=dev), returns=torch.rand((chunk, 2), device=dev),
                       speed=torch.rand(chunk, device=dev), similarity=torch.rand(chunk, device=dev))
        chunks[chunk] = (eng, bufs, targets, score_block(A, dev))

    launch_ms = {c: [] for c in chunks}
    forward_ms = {c: [] for c in chunks}
    score_ms, naive_ms, load_ms = [], [], []
    for k in range(args.rounds + 1):
        for chunk, (eng, bufs, t, block) in chunks.items():
            with limit(args.limit, f'launch {chunk}'):
                a = events(lambda: beta_score(eng._pred_out[0], eng._pred_out[1], t['u'], t['returns'], t['speed'], t['similarity'],
                                              block=block), 200)
                b = events(lambda: eng.predict(bufs), 20)
            if k:
                launch_ms[chunk].append(a)
                forward_ms[chunk].append(b)
        with limit(args.limit, 'score_traces'):
            dt_s, got = host(lambda: agent.score_traces(held, aux=False))
        with limit(args.limit, 'naive'):
            dt_n, want = host(naive)
        with limit(args.limit, 'load'):
            dt_l, _ = host(load)
        exact, err = score_ref.compare(got['block'], want, A)
        assert got['rows'] == files * per and exact and err < 1e-9, (got['rows'], exact, err)
        if k:
            score_ms.append(dt_s)
            naive_ms.append(dt_n)
            load_ms.append(dt_l)

    launches = []
    for chunk in chunks:
        a, b = spread(launch_ms[chunk], 5), spread(forward_ms[chunk], 4)
        launches.append(dict(kernel='beta_score', rows=chunk, actions=A, ms=a, forward_ms=b,
                             share_of_forward=round(a['median'] / b['median'], 4)))
    s, n, l = spread(score_ms), spread(naive_ms), spread(load_ms)
    sweep = dict(rows=files * per, files=files, chunk=CHUNK, score_traces_ms=s, naive_ms=n, load_ms=l,
                 speedup=round(n['median'] / s['median'], 2),
                 behind_the_load=dict(score_traces_ms=round(s['median'] - l['median'], 3), naive_ms=round(n['median'] - l['median'], 3)),
                 worst_sum_error=err, figures={k: got[k] for k in ('log_prob', 'rmse', 'coverage_90', 'value_rmse')})
    out = dict(metric='score', stack=[T, H, W, 3], timed_rounds=args.rounds,
               clock='launch / forward: device events around back-to-back launches; score / naive / load: host perf_counter around one '
                     'call, ending in a device synchronise; median (min, max), blocks alternating in one process',
               launches=launches, sweep=sweep,
               not_measured='any effect on learning or driving quality; nothing on the timed path of bench.py runs this code')
    for row in launches + [sweep]:
        print(json.dumps(row), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(dict(metric=out['metric'], written=os.path.relpath(args.out, ROOT))))


if __name__ == '__main__':
    main()

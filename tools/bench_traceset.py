"""Device-resident trace sets (rl/trace_set.py) against the file path they replace, in ONE process, alternating
blocks, medians with block spreads:

  (a) imitate() of `--epochs` epochs over `--rows` rows of 4 x 90 x 120 x 3 in 8 per-step files (images of the form q / 255), from
      the files -- every epoch reads, inflates and uploads every file -- against trace_set=; the set's build time is reported apart.
      Both start from the same weights and the same generator state and must end with the same bits.
  (b) ONE minibatch of `--batch` rows: the cdrl_traceset_batch launch against cdrl_gather_rows on the windowed float32 tensors
      (one call per key, what data_to_batches does), HIP events; bytes moved computed from the shapes, and achieved bandwidth.
  (c) device bytes per key and code.
Refuses to run under a wrong-result diagnostic switch.

    python tools/bench_traceset.py
    python tools/bench_traceset.py --rows 64 --height 48 --width 64 --epochs 1 --blocks 1 --out /tmp/x.json       # a tiny run
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs, digits=3):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits),
                blocks=[round(x, digits) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=2048, help='rows of the traces, in 8 files')
    ap.add_argument('--height', type=int, default=90)
    ap.add_argument('--width', type=int, default=120)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--blocks', type=int, default=3, help='timed blocks per side (alternating), one untimed first')
    ap.add_argument('--reps', type=int, default=50, help='minibatch assemblies per block of (b)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r24_traceset_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    from carla_driving_rl_agent_amd import _lib, traces
    from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.rl import utils

    if _lib.diag_active():
        raise SystemExit(f'[bench_traceset] refusing to benchmark: wrong-result diagnostic switches are active ({_lib.env_overrides()})')
    if not torch.cuda.is_available():
        raise SystemExit('[bench_traceset] needs a GPU')
    torch.cuda.set_device(0)
    T, H, W, A = 4, args.height, args.width, 2
    work = tempfile.mkdtemp(prefix='cdrl_bench_')
    try:
        env = FakeCARLAEnvironment(image_shape=(H, W, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=A,
                                   image_range=(0.0, 1.0), seed=100)
        agent = CARLAgent(env, batch_size=args.batch, log_mode=None, seed=5, aug_intensity=0.0, weights_dir=os.path.join(work, 'weights'),
                          name='bench_traceset')
        dev, eng = agent.device, agent.network.engine
        rng = np.random.default_rng(7)
        files, per = 8, args.rows // 8
        path = os.path.join(work, 'traces')
        for k in range(files):
            image = rng.integers(0, 256, (per, H, W, 3)).astype(np.float32) / np.float32(255.0)
            traces.write_trace(path, k + 1, dict(image=image, road=rng.integers(0, 2, (per, 9)).astype(np.float32),
                                                 vehicle=rng.random((per, 4), dtype=np.float32),
                                                 navigation=rng.random((per, 5), dtype=np.float32)),
                               rng.uniform(-1.0, 1.0, (per, A)).astype(np.float32), rng.uniform(0.0, 1.0, per).astype(np.float32),
                               np.zeros(per, np.float32), dict(speed=rng.uniform(0.0, 30.0, per), similarity=rng.uniform(-1.0, 1.0, per)))

        def host(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        build_ms, ts = host(lambda: agent.load_trace_set(path))
        arenas = ('params', 'adam_m', 'adam_v')
        start = {n: getattr(eng, n).clone() for n in arenas}
        steps = eng.named_buffer('hparams', dtype=torch.int32).clone()
        rng_state = agent.rng.bit_generator.state

        def imitate(**source):
            """From the same weights, optimizer state and generator state every time.  -> (ms, the arenas it leaves)."""
            for n in arenas:
                getattr(eng, n).copy_(start[n])
            eng.named_buffer('hparams', dtype=torch.int32).copy_(steps)
            agent.rng.bit_generator.state = rng_state
            stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
            try:
                ms, _ = host(lambda: agent.imitate(epochs=args.epochs, value_weight=0.5, close=False, **source))
            finally:
                sys.stdout.close()
                sys.stdout = stdout
            return ms, [getattr(eng, n).clone() for n in arenas]

        # ---- (a)
        times, same = dict(files=[], trace_set=[]), True
        for k in range(args.blocks + 1):
            ms_f, left_f = imitate(traces_dir=path)
            ms_s, left_s = imitate(trace_set=ts)
            same = same and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(left_f, left_s))
            if k:
                times['files'].append(ms_f)
                times['trace_set'].append(ms_s)
        part_a = dict(rows=ts.rows, files=files, epochs=args.epochs, batch=args.batch, image=[T, H, W, 3],
                      imitate_from_files_ms=spread(times['files'], 1), imitate_from_trace_set_ms=spread(times['trace_set'], 1),
                      trace_set_build_ms=round(build_ms, 1), same_bits=bool(same),
                      note='wall clock around a synchronize; the build (reading the files once, choosing and checking the codes on '
                           'the host, the upload) is paid once and is not part of imitate_from_trace_set_ms')

        # ---- (b)
        B = min(args.batch, ts.rows)
        order = np.random.default_rng(1).permutation(ts.rows).astype(np.int32)
        index = ts.upload_index(order)
        whole = {k: v for k, v in ts.batch(ts._dev['identity'], 0, min(ts.rows, 65535), ())['states'].items()}       # windowed float32
        pick = index[:B]

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

        new = lambda: ts.batch(index, 0, B, ())
        old = lambda: {k: utils.gather_rows(v, pick) for k, v in whole.items()}
        got, want = new()['states'], old()
        equal = all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in want)
        ms = dict(new=[], old=[])
        for k in range(args.blocks + 1):
            a, b = events(new, args.reps), events(old, args.reps)
            if k:
                ms['new'].append(a)
                ms['old'].append(b)
        written = sum(B * T * ts.row_elems[k] * 4 for k in ts.codes)
        item = dict(f32=4, f16=2, u8=1)
        # every frame of every row is fetched (neighbouring frames mostly from cache): an upper bound on what reaches memory
        read_new = sum(B * T * ts.row_elems[k] * item[ts.codes[k]] for k in ts.codes)
        moved = dict(new=read_new + written, old=2 * written)
        med = {k: statistics.median(v) for k, v in ms.items()}
        part_b = dict(rows=B, launch_ms=spread(ms['new'], 4), gather_rows_ms=spread(ms['old'], 4), same_bits=bool(equal),
                      bytes_written=written, bytes_read_launch=read_new, bytes_read_gather_rows=written,
                      launch_gbytes_per_s=round(moved['new'] / med['new'] / 1e6, 1),
                      gather_rows_gbytes_per_s=round(moved['old'] / med['old'] / 1e6, 1),
                      note='HIP events around `reps` assemblies including their output allocations; the launch decodes from the coded '
                           'slots, gather_rows copies rows of the windowed float32 tensors (one call per key); bytes from the shapes')

        # ---- (c)
        nbytes = ts.nbytes
        windowed = sum(ts.rows * T * ts.row_elems[k] * 4 for k in ts.codes)
        part_c = dict(nbytes=nbytes, windowed_float32_bytes=windowed, ratio=round(windowed / nbytes['total'], 2))

        out = dict(metric='trace_set_vs_files', device=torch.cuda.get_device_name(0), blocks=args.blocks, reps=args.reps,
                   env_overrides=_lib.env_overrides(), imitate=part_a, minibatch=part_b, storage=part_c,
                   not_measured='any effect of mixed minibatches (mix_traces=True) on learning; sets larger than the Infinity Cache')
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

"""Expert traces on disk: the `trace-*.npz` files the reference's CARLACollectWrapper writes from the privileged autopilot
(rl/environments/carla/environment.py:710-806) and PPOAgent.imitate learns from, their readers (rl/utils.py:502-565), and the host
side of the windowing that turns per-step rows into the learner's (time_horizon, ...) stacks.  Pure host code: numpy only.

Layout of one trace of N recorded steps:
  state_<key>      (N, ...) per observation key, float32; either per-step rows or rows that already carry the time_horizon axis
  action           (N, A)   in ENVIRONMENT units (action_space.low .. high)
  reward           (N + 1,) the step rewards and a trailing 0 for the state behind the last step
  done             (N,)
  info_speed       (N, 1)   km/h, info_similarity (N, 1): the targets of the auxiliary heads (optional)
File name trace-<episode>-<YYYYmmdd-HHMMSS>.npz (numpy compressed)."""
import os
import time
from typing import Optional

import numpy as np


def trace_files(dir_path: str, sort=True) -> list:
    """Names of the trace files (trace-*.npz) in a directory, sorted by name unless told otherwise."""
    names = [f for f in os.listdir(dir_path)
             if f.startswith('trace-') and f.endswith('.npz') and os.path.isfile(os.path.join(dir_path, f))]
    return sorted(names) if sort else names


def load_traces(traces_dir: str, max_amount: Optional[int] = None, shuffle=False, offset=0,
                rng: Optional[np.random.Generator] = None):
    """Generator over the opened traces of a directory: files [offset, max_amount) of the order, which is the sorted one or, with
    shuffle, a permutation of it drawn from `rng` (a fresh default generator when none is given) -- never from the global
    `random`, so a seeded agent reads its traces in a reproducible order."""
    if offset < 0:
        raise ValueError(f'load_traces: offset must not be negative, got {offset}')
    names = trace_files(traces_dir, sort=True)      # sorted first: the permutation does not depend on the directory's listing order
    if shuffle:
        rng = rng if rng is not None else np.random.default_rng()
        names = [names[i] for i in rng.permutation(len(names))]
    stop = len(names) if max_amount is None else min(len(names), int(max_amount))
    for name in names[offset:stop]:
        with np.load(os.path.join(traces_dir, name)) as f:
            yield {k: f[k] for k in f.keys()}


def unpack_trace(trace, unpack=True):
    """A loaded trace -> (state, action, reward, done), or with unpack=False the trace dict with its `state_<key>` / `action_<key>`
    entries folded into trace['state'] / trace['action'] (a dict of arrays when there are several, the array itself when there
    is one) and every other entry (reward, done, info_*) kept.  `done` is None when the trace has none."""
    keys = list(trace.keys())
    out = {k: trace[k] for k in keys}
    for name in ('state', 'action'):
        if sum(k.startswith(name) for k in keys) == 1:
            only = next(k for k in keys if k.startswith(name))
            out[name] = out[only]
            continue
        out[name] = {k: trace[k] for k in keys if k.startswith(name + '_')}
    out.setdefault('done', None)
    if unpack:
        return out['state'], out['action'], np.asarray(out['reward'], dtype=np.float32), out['done']
    for k in keys:
        if (k.startswith('state') or k.startswith('action')) and k not in ('state', 'action'):
            out.pop(k)
    return out


def window_index(n_rows: int, T: int) -> np.ndarray:
    """Row indices that stack T consecutive steps per row: int32 (n_rows * T,), entry n * T + t = max(n - (T - 1 - t), 0).  Slot
    T - 1 is the row's own step, the slots in front of it the steps before; at the start of a trace the first frame repeats.
    One call per trace, so a window never reaches into another trace."""
    if n_rows < 0 or T < 1:
        raise ValueError(f'window_index: need n_rows >= 0 and T >= 1, got {n_rows} and {T}')
    n = np.arange(n_rows, dtype=np.int64)[:, None]
    t = np.arange(T, dtype=np.int64)[None, :]
    return np.maximum(n - (T - 1 - t), 0).astype(np.int32).reshape(-1)


def unit_actions(actions, low, high) -> np.ndarray:
    """Environment actions -> the unit interval the Beta policy lives on: clip((a - low) / (high - low), 0, 1), float32.
    low / high: scalars or per-action arrays (the action space's bounds)."""
    a = np.asarray(actions, dtype=np.float32)
    low, high = np.asarray(low, dtype=np.float32), np.asarray(high, dtype=np.float32)
    if np.any(high <= low):
        raise ValueError('unit_actions: every action needs high > low')
    return np.clip((a - low) / (high - low), 0.0, 1.0).astype(np.float32)


def write_trace(dir_path: str, episode: int, states: dict, actions, rewards, done, info: Optional[dict] = None) -> str:
    """Writes one trace in the layout above and returns its path.  states: {key or state_key: (N, ...)}; actions (N, A) in
    environment units; rewards (N,) -- the trailing 0 is added here -- or (N + 1,) as they are; done (N,); info: {'speed': (N,) or
    (N, 1), 'similarity': ...} or None."""
    actions = np.asarray(actions, dtype=np.float32)
    n = actions.shape[0]
    actions = actions.reshape(n, -1)
    rewards = np.asarray(rewards, dtype=np.float32).reshape(-1)
    if rewards.shape[0] == n:
        rewards = np.concatenate([rewards, np.zeros(1, np.float32)])
    if rewards.shape[0] != n + 1:
        raise ValueError(f'write_trace: {n} steps need {n} or {n + 1} rewards, got {rewards.shape[0]}')
    buffer = dict(action=actions, reward=rewards, done=np.asarray(done, dtype=np.float32).reshape(-1))
    if buffer['done'].shape[0] != n:
        raise ValueError(f"write_trace: {n} steps need {n} done flags, got {buffer['done'].shape[0]}")
    for k, v in states.items():
        v = np.asarray(v, dtype=np.float32)
        if v.shape[0] != n:
            raise ValueError(f'write_trace: state {k} has {v.shape[0]} rows for {n} steps')
        buffer[k if k.startswith('state_') else f'state_{k}'] = v
    for k, v in (info or {}).items():
        v = np.asarray(v, dtype=np.float32).reshape(-1, 1)
        if v.shape[0] != n:
            raise ValueError(f'write_trace: info {k} has {v.shape[0]} rows for {n} steps')
        buffer[k if k.startswith('info_') else f'info_{k}'] = v
    os.makedirs(dir_path, exist_ok=True)
    base = f'trace-{episode}-{time.strftime("%Y%m%d-%H%M%S")}'
    path, k = os.path.join(dir_path, base + '.npz'), 0
    while os.path.exists(path):         # several traces of one episode within a second (an environment shard): keep them all
        k += 1
        path = os.path.join(dir_path, f'{base}-{k}.npz')
    np.savez_compressed(path, **buffer)
    return path

"""Expert demonstrations inside the PPO update (PPOAgent(demo_traces=...)): how a policy minibatch is cut into
fresh and demonstration rows, and the device-resident store the demonstration rows are drawn from.  The split and the draws are
pure host code (numpy); the store keeps its rows on the device and gathers there."""
from typing import Iterable

import numpy as np
import torch

from . import utils


def demo_split(batch_size: int, fraction: float) -> tuple:
    """-> (D, batch_size - D): demonstration and fresh rows of one policy minibatch, D = round(fraction * batch_size).
    ValueError unless 1 <= D < batch_size."""
    try:
        d = int(round(float(fraction) * int(batch_size)))
    except (TypeError, ValueError):
        raise ValueError(f'demo_fraction={fraction!r}: a number in (0, 1)') from None
    if not 1 <= d < batch_size:
        raise ValueError(f'demo_fraction={fraction!r} gives D = {d} demonstration rows in a minibatch of {batch_size}: it must leave '
                         f'at least one demonstration row and one fresh row (1 <= D < batch_size)')
    return d, int(batch_size) - d


def draw_rows(rng: np.random.Generator, rows: int, count: int) -> np.ndarray:
    """`count` distinct row indices of a store of `rows` rows, int32, in the order drawn."""
    return rng.choice(rows, size=count, replace=False).astype(np.int32)


class DemonstrationStore:
    """At most `cap` demonstration rows on the device: states (dict of (N, ...) tensors), u (N, A) unit actions, speed and
    similarity (N,) targets.  Built from per-trace tensor dicts (PPOAgent._trace_tensors with need_info) in the order given, cut
    at the cap; `left_out` counts the rows that did not fit.  ValueError when fewer than `need` rows came in."""

    KEYS = ('u', 'speed', 'similarity')

    def __init__(self, traces: Iterable[dict], cap: int, need: int):
        parts, rows, self.left_out, self.traces = [], 0, 0, 0
        for t in traces:
            n = int(t['u'].shape[0])
            take = max(0, min(n, int(cap) - rows))
            self.left_out += n - take
            if take:
                cut = (lambda x: x[:take].contiguous()) if take < n else (lambda x: x)
                parts.append(dict(states={k: cut(v) for k, v in t['states'].items()}, **{k: cut(t[k]) for k in self.KEYS}))
                rows += take
                self.traces += 1
        if rows < need:
            raise ValueError(f'the demonstration store holds {rows} rows, every policy minibatch needs {need}: give more traces, or a '
                             f'smaller demo_fraction / batch_size (demo_rows caps the store at {cap})')
        cat = lambda xs: xs[0] if len(xs) == 1 else torch.cat(xs, dim=0)
        self.states = {k: cat([p['states'][k] for p in parts]) for k in parts[0]['states']}
        self.u, self.speed, self.similarity = (cat([p[k] for p in parts]) for k in self.KEYS)
        self.rows = rows

    def gather(self, index: np.ndarray) -> dict:
        """The rows `index` as fresh device tensors: dict(states, u, speed, similarity)."""
        idx = torch.as_tensor(np.asarray(index, dtype=np.int32), device=self.u.device)
        return dict(states={k: utils.gather_rows(v, idx) for k, v in self.states.items()}, u=utils.gather_rows(self.u, idx),
                    speed=utils.gather_rows(self.speed, idx), similarity=utils.gather_rows(self.similarity, idx))

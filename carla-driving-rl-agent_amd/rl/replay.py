"""RolloutReplay: the most recent finished update-periods of a PPOAgent, kept on the device so that update() can train on their rows
again (PPOAgent(replay_rollouts=K)).  The rows are off-policy by the time they are reused: update() re-evaluates the
current policy and value head on them and corrects the targets with V-trace (utils.vtrace_segments, one launch for all kept periods).

This module is bookkeeping only -- what a period holds, in which order periods leave, and the index tables that lay a period's rows
out in the padded form of the trajectory kernels.  Everything is built from host-side counts: no device-to-host read anywhere."""
from collections import deque
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

States = Union[torch.Tensor, Dict[str, torch.Tensor]]


def _rows(states: States) -> int:
    return int((next(iter(states.values())) if isinstance(states, dict) else states).shape[0])


class ReplayPeriod:
    """One finished update-period: everything update() trained on between two optimizer phases.
    states / actions (N, A) / log_probs (N, A) / rewards (N,): the rows as the memory held them (behaviour log-probabilities, per-step
    rewards without bootstrap entries).  trajectories: [(rows, terminal), ...] in memory order.  finals: the observation behind the
    last step of every TRUNCATED trajectory, (K, ...) per state key in trajectory order, or None when all were terminal.
    info: dict of per-row auxiliary targets (CARLAgent: speed, similarity) or None.  targets: what the last refresh computed for the rows
    (advantages (N,), returns_be (N, 2)), None until then."""

    def __init__(self, states: States, actions: torch.Tensor, log_probs: torch.Tensor, rewards: torch.Tensor,
                 trajectories: Sequence[Tuple[int, bool]], finals: Optional[States], info: Optional[Dict[str, torch.Tensor]] = None):
        self.trajectories = [(int(n), bool(t)) for n, t in trajectories]
        self.rows = sum(n for n, _ in self.trajectories)
        truncated = sum(1 for _, t in self.trajectories if not t)
        if not self.trajectories or min(n for n, _ in self.trajectories) < 1:
            raise ValueError(f'ReplayPeriod: every trajectory needs at least one row (table {self.trajectories})')
        for name, have in (('states', _rows(states)), ('actions', int(actions.shape[0])), ('log_probs', int(log_probs.shape[0])),
                           ('rewards', int(rewards.shape[0]))):
            if have != self.rows:
                raise ValueError(f'ReplayPeriod: the trajectory table counts {self.rows} rows, {name} holds {have}')
        if (_rows(finals) if finals is not None else 0) != truncated:
            raise ValueError(f'ReplayPeriod: {truncated} truncated trajectories need as many final observations, got '
                             f'{_rows(finals) if finals is not None else 0}')
        if info is not None and any(int(t.shape[0]) != self.rows for t in info.values()):
            raise ValueError(f'ReplayPeriod: info targets must hold {self.rows} rows')
        self.states, self.actions, self.log_probs, self.rewards = states, actions, log_probs, rewards
        self.finals, self.info = finals, info
        self.targets: Optional[Dict[str, torch.Tensor]] = None

    @property
    def lengths(self) -> List[int]:
        return [n for n, _ in self.trajectories]

    @property
    def truncated(self) -> List[int]:
        """Indices (into the trajectory table) of the trajectories whose bootstrap value must be estimated."""
        return [s for s, (_, terminal) in enumerate(self.trajectories) if not terminal]

    def padded_index(self) -> Tuple[np.ndarray, np.ndarray]:
        """Where the period's rows and bootstrap entries sit in the padded layout of the trajectory kernels (every trajectory followed
        by its own bootstrap entry): -> (row_index (N,), bootstrap_index (S,)), int64, relative to the period's first padded entry."""
        lengths = np.asarray(self.lengths, dtype=np.int64)
        ends = np.cumsum(lengths)
        seg_of_row = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
        return np.arange(self.rows, dtype=np.int64) + seg_of_row, ends + np.arange(len(lengths), dtype=np.int64)


class RolloutReplay:
    """Holds the `capacity` most recent periods; adding to a full store evicts the oldest."""

    def __init__(self, capacity: int):
        if int(capacity) < 1:
            raise ValueError(f'RolloutReplay(capacity={capacity}): at least one period')
        self.capacity = int(capacity)
        self.periods: deque = deque()
        self.last_refresh: Optional[dict] = None     # inputs and outputs of the last V-trace launch (diagnostics, tests)

    def __len__(self) -> int:
        return len(self.periods)

    @property
    def rows(self) -> int:
        return sum(p.rows for p in self.periods)

    def add(self, period: ReplayPeriod) -> Optional[ReplayPeriod]:
        """-> the evicted period, or None."""
        evicted = self.periods.popleft() if len(self.periods) == self.capacity else None
        self.periods.append(period)
        return evicted

    def clear(self):
        self.periods.clear()
        self.last_refresh = None


class TrajectoryTable:
    """What trajectory_stored() collects between two update()s: per trajectory its row count, terminal flag and -- when truncated --
    the observation behind its last step."""

    def __init__(self):
        self.entries: List[Tuple[int, bool]] = []
        self.finals: List[States] = []

    def __len__(self) -> int:
        return len(self.entries)

    def record(self, rows: int, terminal: bool, final: Optional[States]):
        self.entries.append((int(rows), bool(terminal)))
        if not terminal:
            if final is None:
                raise ValueError('TrajectoryTable.record: a truncated trajectory needs the observation behind its last step')
            self.finals.append(final)

    def stacked_finals(self) -> Optional[States]:
        """(K, ...) per state key over the truncated trajectories (each recorded as a (1, ...) row), or None."""
        if not self.finals:
            return None
        if isinstance(self.finals[0], dict):
            return {k: torch.cat([f[k] for f in self.finals], dim=0) for k in self.finals[0]}
        return torch.cat(self.finals, dim=0)

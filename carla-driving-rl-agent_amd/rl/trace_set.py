"""Device-resident trace sets: a directory of `trace-*.npz` files (traces.py) read ONCE and kept on the device as
per-step rows in the most compact lossless code, and minibatches of time-stacked float32 rows assembled from it by one
cdrl_traceset_batch launch (csrc/traceset.hip) -- of one trace in order (what PPOAgent._trace_tensors uploads from a file, bit for
bit) or of arbitrary rows of the whole set.

Storage.  Every state key is an array of slots, one slot = one time step's row.  A trace recorded per step takes one slot per row; a
trace that carries the time_horizon axis on disk takes T slots per row.  Two int32 tables describe the rows of the set:
  slot[r]   the slot of row r's own, newest step
  lo[r]     the lowest slot its window may reach: the first slot of a per-step trace, slot[r] - (T - 1) for a stacked one
and frame t of row r is slot max(slot[r] - (T - 1 - t), lo[r]) -- traces.window_index within a per-step trace, the row's own T frames
for a stacked one, with one formula.
Codes, one per key: 'u8' a byte index into a palette of at most 256 float32 BIT PATTERNS (lossless for q / 255 camera bytes, 0 / 1
features and anything else with at most 256 distinct values; -0.0 and +0.0 are two entries), 'f16' IEEE half where every value
survives the round trip, 'f32' otherwise.  The choice is made on bit patterns and verified by decoding on the host before upload.
The per-row columns (unit actions, weights, speed, similarity, returns) live in one (N, W) float32 matrix.
Host code: numpy + torch; the device is touched by upload and by batch()."""
import ctypes as C
import os
import types

import numpy as np
import torch

from .. import _lib, traces

CODES = ('u8', 'f16', 'f32')        # smallest first
CODE_ID = dict(f32=_lib.TRACE_F32, f16=_lib.TRACE_F16, u8=_lib.TRACE_U8)
ITEM_BYTES = dict(f32=4, f16=2, u8=1)
COLUMNS = ('u', 'weight', 'speed', 'similarity', 'returns')
MAX_KEYS, MAX_ROWS, MAX_T = 8, 65535, 16


# ---------------------------------------------------------------------------------------------------------------- the three codes
def float_bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def half_bits_to_float_bits(h) -> np.ndarray:
    """uint16 half patterns -> the uint32 patterns of the same values, by bit operations alone (a NaN keeps sign and payload)."""
    h = np.asarray(h, dtype=np.uint16).astype(np.uint32)
    sign, e, m = (h & 0x8000) << 16, (h >> 10) & 0x1f, h & 0x3ff
    normal = sign | ((e + 112) << 23) | (m << 13)
    special = sign | np.uint32(0x7f800000) | (m << 13)
    sub = (m.astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32) | sign
    return np.where(e == 31, special, np.where(e == 0, sub, normal)).astype(np.uint32)


def encode_half(a) -> np.ndarray:
    """float32 -> uint16 half patterns, round to nearest even."""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.ascontiguousarray(a, dtype=np.float32).astype(np.float16).view(np.uint16)


def decode(code: str, coded: np.ndarray, palette=None) -> np.ndarray:
    """Coded slots -> float32 bit patterns (uint32), as the kernel decodes them."""
    if code == 'f32':
        return float_bits(coded)
    if code == 'f16':
        return half_bits_to_float_bits(coded)
    if code == 'u8':
        return np.asarray(palette, dtype=np.uint32)[coded]
    raise ValueError(f'unknown code {code!r}: one of {CODES}')


def find_palette(arrays, limit=256):
    """The sorted distinct float32 bit patterns of a list of arrays, or None when there are more than `limit`.  Looks at a small
    piece first, so data with many values is given up at once; after that only patterns the palette lacks are sorted."""
    pal = np.empty(0, np.uint32)
    for a in arrays:
        bits = float_bits(a).reshape(-1)
        start, size = 0, 4096
        while start < bits.size:
            piece = bits[start:start + size]
            if pal.size:
                at = np.minimum(np.searchsorted(pal, piece), pal.size - 1)
                piece = piece[pal[at] != piece]
            if piece.size:
                pal = np.union1d(pal, np.unique(piece))
                if pal.size > limit:
                    return None
            start, size = start + size, 1 << 22
    return pal


def choose_code(arrays, force=None):
    """The smallest code that reproduces every float32 bit of `arrays` (one key's rows, trace by trace).  force='f16': half whatever
    it loses.  -> (code, list of coded arrays, palette as 256 uint32 or None)."""
    if force not in (None, 'f16'):
        raise ValueError(f'force = {force!r}: None or f16')
    if force is None:
        pal = find_palette(arrays)
        if pal is not None:
            full = np.zeros(256, np.uint32)
            full[:pal.size] = pal
            return 'u8', [np.searchsorted(pal, float_bits(a)).astype(np.uint8) for a in arrays], full
    halves = [encode_half(a) for a in arrays]
    if force == 'f16' or all(np.array_equal(half_bits_to_float_bits(h), float_bits(a)) for h, a in zip(halves, arrays)):
        return 'f16', halves, None
    return 'f32', [np.ascontiguousarray(a, dtype=np.float32) for a in arrays], None


def build_tables(layout, T: int):
    """layout: per trace (rows, stacked).  -> slot, lo (int32, one entry per row of the set), first slot per trace, slots in all."""
    slot, lo, first, s0 = [], [], [], 0
    for n, stacked in layout:
        first.append(s0)
        local = np.arange(n, dtype=np.int64)
        if stacked:
            own = s0 + local * T + (T - 1)
            slot.append(own)
            lo.append(own - (T - 1))
            s0 += n * T
        else:
            slot.append(s0 + local)
            lo.append(np.full(n, s0, np.int64))
            s0 += n
    if s0 >= 2 ** 31:
        raise ValueError(f'{s0} slots do not fit the int32 tables')
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return cat(slot), cat(lo), first, s0


# ------------------------------------------------------------------------------------------------------------------------ the spec
class TraceSpec:
    """What a trace must fit, taken from an agent or given by hand: per-step state shapes, time_horizon, the action space, gamma, the
    device.  Carries the names PPOAgent._check_trace reads, so a set built from a spec refuses a trace in the agent's words."""

    def __init__(self, state_spec: dict, time_horizon: int, num_actions: int, action_low, action_high, gamma=0.99, device='cuda:0',
                 stacks_time=True):
        self.state_spec = {k: tuple(int(x) for x in v) for k, v in state_spec.items()}
        self.env = types.SimpleNamespace(time_horizon=int(time_horizon))
        self.num_actions, self.gamma, self.device = int(num_actions), float(gamma), device
        self.action_low, self.action_high = action_low, action_high
        self._stacks = bool(stacks_time)

    @classmethod
    def of(cls, agent) -> 'TraceSpec':
        if isinstance(agent, cls):
            return agent
        return cls({k: agent.state_spec[k] for k in agent.imitation_state_keys()}, getattr(agent.env, 'time_horizon', 1),
                   agent.num_actions, agent.action_low, agent.action_high, agent.gamma, agent.device, agent.stacks_time())

    def imitation_state_keys(self) -> list:
        return list(self.state_spec)

    def stacks_time(self) -> bool:
        return self._stacks

    def _check_trace_states(self, trace, n=None):
        from .agents.ppo import PPOAgent
        return PPOAgent._check_trace_states(self, trace, n)

    def check_trace(self, trace) -> int:
        from .agents.ppo import PPOAgent
        return PPOAgent._check_trace(self, trace, False, 0.0)

    @property
    def T(self) -> int:
        return self.env.time_horizon if self._stacks else 1


# ------------------------------------------------------------------------------------------------------------------------- the set
class TraceSet:
    """See the module text.  Made by from_dir (or agent.load_trace_set); read-only afterwards."""

    @classmethod
    def from_dir(cls, agent_or_spec, traces_dir: str, max_traces=None, storage='exact', weights=None, upload=True) -> 'TraceSet':
        """Reads the first `max_traces` (None: all) files of `traces_dir` in sorted order, each once.  storage: 'exact' (lossless, the
        smallest code per key) or 'f16' (state_image as half even where that loses bits; every other key exact).  weights:
        callable(trace dict) -> (N,) per-row weights, evaluated once per trace here.  upload=False keeps the set on the host (tables,
        codes, sizes and plans only: no batch).  ValueError, naming the file: a trace that does not fit; also an empty directory."""
        if storage not in ('exact', 'f16'):
            raise ValueError(f"storage = {storage!r}: 'exact' or 'f16'")
        spec = TraceSpec.of(agent_or_spec)
        T = spec.T
        if not 1 <= T <= MAX_T:
            raise ValueError(f'time_horizon {T}: a trace set stacks 1 to {MAX_T} frames')
        names = traces.trace_files(traces_dir, sort=True)
        names = names if max_traces is None else names[:int(max_traces)]
        if not names:
            raise ValueError(f'TraceSet: no trace-*.npz file in {traces_dir}')
        keys = spec.imitation_state_keys()
        per_key = {k: [] for k in keys}
        layout, u, w, speed, sim, rewards = [], [], [], [], [], []
        has_info = has_value = True
        for name in names:
            with np.load(os.path.join(traces_dir, name)) as f:
                trace = {k: f[k] for k in f.keys()}
            try:
                n = spec.check_trace(trace)
                if n < 1:
                    raise ValueError('the trace has no rows')
                wide = [k for k in keys if np.ndim(trace[k]) - 1 > len(spec.state_spec[k])]
                if wide and not spec.stacks_time():
                    raise ValueError(f'trace {wide[0]} carries a time axis, which this learner does not stack')
                stacked = bool(wide) and T >= 1
                for k in keys:
                    a = np.ascontiguousarray(trace[k], dtype=np.float32)
                    if stacked and k not in wide:           # a per-step key beside a stacked one: windowed here, once
                        a = a[traces.window_index(n, T).reshape(n, T)]
                    per_key[k].append(a.reshape((n * T if stacked else n, -1)))
                u.append(traces.unit_actions(np.asarray(trace['action']).reshape(n, -1), spec.action_low, spec.action_high))
                if weights is not None:
                    wt = np.asarray(weights(trace), dtype=np.float32).reshape(-1)
                    if wt.shape[0] != n:
                        raise ValueError(f'weights(trace) returned {wt.shape[0]} values for a trace of {n} rows')
                    w.append(wt)
            except ValueError as exc:
                raise ValueError(f'{os.path.join(traces_dir, name)}: {exc}') from None
            if has_info and 'info_speed' in trace and 'info_similarity' in trace and np.size(trace['info_speed']) == n \
                    and np.size(trace['info_similarity']) == n:
                speed.append(np.ascontiguousarray(np.reshape(trace['info_speed'], -1), dtype=np.float32))
                sim.append(np.ascontiguousarray(np.reshape(trace['info_similarity'], -1), dtype=np.float32))
            else:
                has_info = False
            if has_value and np.size(trace.get('reward', ())) == n + 1:
                rewards.append(np.ascontiguousarray(np.reshape(trace['reward'], -1), dtype=np.float32))
            else:
                has_value = False
            layout.append((n, stacked))
        self = cls()
        self.spec, self.dir, self.names, self.T, self.storage = spec, traces_dir, list(names), T, storage
        self.shapes = {k: spec.state_spec[k] for k in keys}
        self.row_elems = {k: int(np.prod(spec.state_spec[k], dtype=np.int64)) for k in keys}
        self.layout = layout
        self.slot, self.lo, self.first_slot, self.slots = build_tables(layout, T)
        bounds = np.concatenate([[0], np.cumsum([n for n, _ in layout])]).astype(np.int64)
        self.row_start, self.rows = bounds[:-1], int(bounds[-1])
        self.codes, self.coded, self.palettes = {}, {}, {}
        for k in keys:
            force = 'f16' if storage == 'f16' and k == 'state_image' else None
            code, parts, pal = choose_code(per_key[k], force)
            coded = np.concatenate(parts, axis=0)
            if force is None:       # the lossless promise, checked on what will be uploaded
                if not all(np.array_equal(decode(code, c, pal), float_bits(a)) for c, a in zip(parts, per_key[k])):
                    raise AssertionError(f'{k}: code {code} does not reproduce the rows')
            self.codes[k], self.coded[k], self.palettes[k] = code, coded, pal
            per_key[k] = None
        A = spec.num_actions
        self.column_ranges = dict(u=(0, A))
        for name, width, have in (('weight', 1, weights is not None), ('speed', 1, has_info), ('similarity', 1, has_info),
                                  ('returns', 2, has_value)):
            if have:
                at = max(hi for _, hi in self.column_ranges.values())
                self.column_ranges[name] = (at, at + width)
        self.width = max(hi for _, hi in self.column_ranges.values())
        host = np.zeros((self.rows, self.width), np.float32)
        host[:, :A] = np.concatenate(u, axis=0)
        for name, parts in (('weight', w), ('speed', speed), ('similarity', sim)):
            if name in self.column_ranges:
                host[:, self.column_ranges[name][0]] = np.concatenate(parts)
        self.host_columns, self.rewards, self.gamma = host, rewards if has_value else None, spec.gamma
        self.device, self._dev, self._matrices = None, None, {}
        if upload:
            self._upload(spec.device)
        return self

    # ---- bookkeeping
    @property
    def traces(self) -> int:
        return len(self.layout)

    @property
    def has_weight(self) -> bool:
        return 'weight' in self.column_ranges

    @property
    def has_info(self) -> bool:
        return 'speed' in self.column_ranges

    @property
    def has_value(self) -> bool:
        return 'returns' in self.column_ranges

    def trace_rows(self, i: int) -> tuple:
        """(first row, row count) of trace i."""
        return int(self.row_start[i]), int(self.layout[i][0])

    @property
    def nbytes(self) -> dict:
        """Device bytes: per key dict(code, bytes), then palettes, tables (slot, lo), columns, total."""
        out = {k: dict(code=self.codes[k], bytes=int(self.slots * self.row_elems[k] * ITEM_BYTES[self.codes[k]])) for k in self.codes}
        out['palettes'] = 1024 * sum(p is not None for p in self.palettes.values())
        out['tables'] = 2 * 4 * self.rows
        out['columns'] = 4 * self.rows * self.width
        out['total'] = sum(v['bytes'] for k, v in out.items() if isinstance(v, dict)) + out['palettes'] + out['tables'] + out['columns']
        return out

    def check_fits(self, agent):
        """ValueError when the set was not loaded for an agent like this one."""
        want, have = TraceSpec.of(agent), self.spec
        if want.state_spec != have.state_spec or want.T != self.T:
            raise ValueError(f'the trace set holds {have.state_spec} with {self.T} frames per row; the agent needs {want.state_spec} '
                             f'with {want.T}: load it with this agent (load_trace_set)')
        if want.num_actions != have.num_actions or not (np.array_equal(want.action_low, have.action_low) and
                                                        np.array_equal(want.action_high, have.action_high)):
            raise ValueError(f'the trace set holds unit actions of width {have.num_actions} scaled by another action space than the '
                             f"agent's ({want.num_actions} actions): load it with this agent (load_trace_set)")

    # ---- plans
    def epoch_order(self, rng: np.random.Generator, max_traces=None) -> list:
        """The traces of one epoch as traces.load_traces(shuffle=True) orders the sorted files: one rng.permutation, cut at max_traces."""
        order = rng.permutation(self.traces)
        stop = self.traces if max_traces is None else min(self.traces, int(max_traces))
        return [int(i) for i in order[:stop]]

    def plan_epoch(self, rng: np.random.Generator, batch_size: int, drop_remainder=False):
        """A full permutation of the rows cut into minibatches.  -> (order int32 (rows,), [(offset, rows of the minibatch), ...])."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f'plan_epoch: batch_size = {batch_size}, need at least 1')
        order = rng.permutation(self.rows).astype(np.int32)
        cuts = [(o, min(batch_size, self.rows - o)) for o in range(0, self.rows, batch_size)]
        if drop_remainder:
            cuts = [c for c in cuts if c[1] == batch_size]
        return order, cuts

    def check_index(self, index) -> np.ndarray:
        """Row numbers as a checked int32 host array; ValueError names the first one outside the set."""
        index = np.asarray(index)
        if index.ndim != 1 or not np.issubdtype(index.dtype, np.integer):
            raise ValueError(f'row index: a 1-D integer array, got {index.dtype} of shape {index.shape}')
        bad = np.nonzero((index < 0) | (index >= self.rows))[0]
        if bad.size:
            raise ValueError(f'row index {int(index[bad[0]])} at position {int(bad[0])} is outside 0..{self.rows - 1}')
        return np.ascontiguousarray(index, dtype=np.int32)

    def upload_index(self, index) -> torch.Tensor:
        """check_index, then ONE upload: an epoch's whole order; every minibatch is an (offset, rows) window of it."""
        self._need_device()
        return torch.as_tensor(self.check_index(index)).to(self.device)

    # ---- the device side
    def _need_device(self):
        if self._dev is None:
            raise RuntimeError('the trace set was loaded with upload=False: it has no device storage')

    def _upload(self, device):
        from . import utils
        up = lambda a: torch.as_tensor(a).to(device)
        dev = dict(slot=up(self.slot), lo=up(self.lo), identity=torch.arange(self.rows, dtype=torch.int32, device=device), coded={},
                   palette={})
        for k, coded in self.coded.items():
            dev['coded'][k] = up(coded.view(np.int16) if self.codes[k] == 'f16' else coded)
            if self.palettes[k] is not None:
                dev['palette'][k] = up(self.palettes[k].view(np.int32))
        matrix = up(self.host_columns)
        if self.has_info:       # as PPOAgent._trace_tensors: uploaded, then divided on the device
            at = self.column_ranges['speed'][0]
            matrix[:, at] = up(np.ascontiguousarray(self.host_columns[:, at])) / 100.0
        self.device, self._dev = device, dev
        self._matrices = {}
        if self.has_value:
            self._fill_returns(matrix, self.gamma, utils)
        self._matrices[self.gamma] = matrix
        self.coded = {k: None for k in self.coded}      # the device holds the rows now

    def _fill_returns(self, matrix, gamma, utils):
        lo, hi = self.column_ranges['returns']
        for i, reward in enumerate(self.rewards):       # per trace, the launch _trace_tensors makes
            start, n = self.trace_rows(i)
            zeros = torch.zeros((n + 1, 2), dtype=torch.float32, device=self.device)
            matrix[start:start + n, lo:hi] = utils.returns_and_advantages(reward, zeros, gamma, 0.0, 1.0, self.device)['returns_be']

    def _matrix(self, gamma) -> torch.Tensor:
        gamma = self.gamma if gamma is None else float(gamma)
        if gamma not in self._matrices:                 # another discount: the returns again, from the stored rewards
            from . import utils
            matrix = self._matrices[self.gamma].clone()
            if self.has_value:
                self._fill_returns(matrix, gamma, utils)
            self._matrices[gamma] = matrix
        return self._matrices[gamma]

    def batch(self, index_dev: torch.Tensor, offset: int, rows: int, columns=None, gamma=None) -> dict:
        """Rows index_dev[offset : offset + rows] of the set: dict(states={key: (rows, T) + shape}, u (rows, A), and of weight / speed /
        similarity (rows,) and returns (rows, 2) those in `columns` (None: all the set has; (): states alone) -- fresh contiguous
        float32 tensors, written by one cdrl_traceset_batch launch (two beyond 8 keys in all; one more per 65535 rows).
        index_dev: int32 on the device, made by upload_index (indices are checked THERE; the kernel cannot report one).
        gamma: discount of the returns (None: the one the set was loaded with)."""
        self._need_device()
        offset, rows = int(offset), int(rows)
        if index_dev.dtype != torch.int32 or index_dev.device != self._dev['slot'].device or not index_dev.is_contiguous():
            raise ValueError('batch: the index must be a contiguous int32 tensor on the device of the set (upload_index)')
        if rows < 1 or offset < 0 or offset + rows > index_dev.numel():
            raise ValueError(f'batch: rows [{offset}, {offset} + {rows}) of an index of {index_dev.numel()} entries')
        columns = tuple(c for c in COLUMNS if c in self.column_ranges) if columns is None else tuple(columns)
        lacking = [c for c in columns if c not in self.column_ranges]
        if lacking:
            raise ValueError(f'the trace set has no {lacking} column (it has {list(self.column_ranges)})')
        dev, out, keys = self._dev, dict(states={}), []
        empty = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        for k, code in self.codes.items():
            dst = out['states'][k] = empty(rows, *((self.T,) if self.spec.stacks_time() else ()), *self.shapes[k])
            pal = dev['palette'].get(k)
            keys.append((dev['coded'][k].data_ptr(), 0 if pal is None else pal.data_ptr(), dst, self.row_elems[k], self.row_elems[k],
                         CODE_ID[code], self.T, 0))
        if columns:
            matrix = self._matrix(gamma)
            for c in columns:
                lo, hi = self.column_ranges[c]
                dst = out[c] = empty(rows, hi - lo) if c in ('u', 'returns') else empty(rows)
                keys.append((matrix.data_ptr() + 4 * lo, 0, dst, hi - lo, self.width, CODE_ID['f32'], 1, 1))
        lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for k0 in range(0, len(keys), MAX_KEYS):
            group = keys[k0:k0 + MAX_KEYS]
            for r0 in range(0, rows, MAX_ROWS):
                arr = (_lib.TraceSetKey * len(group))()
                for j, (src, pal, dst, elems, stride, code, T, direct) in enumerate(group):
                    arr[j] = _lib.TraceSetKey(src, pal or None, dst.data_ptr() + 4 * r0 * T * elems, elems, stride, code, T, direct, 0)
                _lib.check(lib.cdrl_traceset_batch(arr, len(group), _lib.ptr(dev['slot']), _lib.ptr(dev['lo']), _lib.ptr(index_dev),
                                                   offset + r0, min(MAX_ROWS, rows - r0), self.rows, stream), 'cdrl_traceset_batch')
        return out

    def trace_tensors(self, i: int, columns=None, gamma=None) -> dict:
        """The rows of trace i in order: the dict PPOAgent._trace_tensors returns for its file, made by the kernel."""
        self._need_device()
        start, n = self.trace_rows(i)
        return self.batch(self._dev['identity'], start, n, columns, gamma)

    def trace_states(self, i: int) -> dict:
        """The state entries of trace i alone (PPOAgent._trace_states)."""
        return self.trace_tensors(i, ())['states']

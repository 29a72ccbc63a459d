"""LearnerEngine: thin Python owner of a `cdrl_learner` handle.

PyTorch is used for device memory (parameter arenas, Adam state, workspace), streams and
`torch.distributed` only; every arithmetic step of the learner runs in libcdrl_hip.so.
"""
import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import TRUNK, POLICY, VALUE, OLD_POLICY

MODEL_IDS = dict(trunk=TRUNK, policy=POLICY, value=VALUE, old_policy=OLD_POLICY)


def make_config(B, T=4, H=90, W=120, road=9, vehicle=4, navigation=5, A=2, **kw) -> _lib.Config:
    lib = _lib.load()
    cfg = _lib.Config()
    lib.cdrl_config_default(C.byref(cfg))
    cfg.B, cfg.T, cfg.H, cfg.W = B, T, H, W
    cfg.road, cfg.vehicle, cfg.navigation, cfg.A = road, vehicle, navigation, A
    for k, v in kw.items():
        if k == 'compute' and isinstance(v, str):
            # 'f32' | 'bf16' (bf16 MFMA operands in the tower's 1x1 convs, float32 tensors) | 'bf16s' (+ bf16 activation STORAGE in
            # the tower: configuration 3 in full)
            v = {'f32': _lib.COMPUTE_F32, 'bf16': _lib.COMPUTE_BF16_OPERANDS, 'bf16s': _lib.COMPUTE_BF16_STORAGE}[v]
        if k == 'freeze_trunk' and isinstance(v, bool):
            v = int(v)
        if k == 'optimizer' and isinstance(v, str):
            if v.lower() not in _lib.OPTIMIZERS:
                raise _lib.CdrlError(f'unknown optimizer {v!r}; select one of {_lib.OPTIMIZERS}')
            v = _lib.OPTIMIZERS.index(v.lower())
        if k == 'clip_mode' and isinstance(v, str):
            if v.lower() not in _lib.CLIP_MODES:
                raise ValueError(f'unknown clip_mode {v!r}; select one of {_lib.CLIP_MODES}')
            v = _lib.CLIP_MODES.index(v.lower())
        if k in ('skip_nonfinite', 'trust') and isinstance(v, bool):
            v = int(v)
        if k in ('stage_c', 'stage_n'):
            for i in range(3):
                getattr(cfg, k)[i] = v[i]
        else:
            setattr(cfg, k, v)
    return cfg


class ParamTable:
    """Variable inventory of one model (trunk / policy / value) as reported by the engine."""

    def __init__(self, lib, handle, model):
        self.entries = []
        n = lib.cdrl_learner_param_count(handle, model)
        for i in range(n):
            pi = _lib.ParamInfo()
            _lib.check(lib.cdrl_learner_param_info(handle, model, i, C.byref(pi)), 'param_info')
            self.entries.append(dict(name=pi.name.decode(), shape=tuple(pi.shape[:pi.ndim]), numel=int(pi.numel),
                                     trainable=bool(pi.trainable), offset=int(pi.offset)))
        self.by_name = {e['name']: e for e in self.entries}

    def spec(self):
        return [(e['name'], e['shape'], e['trainable']) for e in self.entries]


class LearnerEngine:
    def __init__(self, B, device: Optional[str] = 'cuda:0', share_with: 'LearnerEngine' = None, **cfg):
        """device=None -> host-only inspection (parameter tables, workspace size; no HIP calls).
        share_with -> reuse another engine's parameter arenas (e.g. a B=1 rollout engine); the new engine inherits its
        freeze_trunk, optimizer and polyak unless they are given.
        freeze_trunk=True -> the passes train the heads only on a fixed trunk (cdrl_config.freeze_trunk, include/cdrl.h).
        optimizer -> one of _lib.OPTIMIZERS, any letter case (the reference's get_optimizer_by_name), for the policy, value and
        dynamics optimizers; its slots live in the adam_m / adam_v arenas (optimizer_slots).  polyak in (0, 1]: < 1 averages the
        heads after each optimizer step (cdrl_config.optimizer / polyak, include/cdrl.h).
        train_stats=N > 0 -> every policy_apply / value_apply appends one row of update diagnostics to a device ring of N rows
        (cdrl_config.train_stats); train_stats() fetches them.  Not inherited through share_with (rollout engines have no use for
        it); an engine that is given it appends to the ring of the engine it shares with, when that one has a ring too.
        clip_mode -> 'tensor' (default: tf.clip_by_norm per tensor of the two heads, the trunk unclipped, as the reference does)
        or 'global' (every optimizer's gradient list clipped by its global norm: the heads with clip_norm_policy / clip_norm_value,
        the trunk with clip_norm_dynamics); an unknown name raises ValueError.  skip_nonfinite=True -> an apply step whose
        gradients hold a NaN or an Inf writes nothing and is counted (gate_stats).  Both are cdrl_config fields (include/cdrl.h,
        gradient gate), off by default, and inherited through share_with (a different value there is refused by the library).
        trust=True -> the trust-region guard of the policy steps (cdrl_config.trust, include/cdrl.h): policy batches
        may carry an 'anchor' (B, 2, A), whose Beta KL to the pass's policy is measured on the device; policy_apply obeys the
        block's latch (set_hparams(target_kl=, kl_stop_factor=, kl_coef=), trust_stats, trust_reset).  Off by default, inherited
        through share_with like the gate's options."""
        self.lib = _lib.load()
        if share_with is not None:
            cfg.setdefault('freeze_trunk', share_with.frozen)
            cfg.setdefault('optimizer', share_with.optimizer)
            cfg.setdefault('polyak', share_with.polyak)
            cfg.setdefault('clip_mode', share_with.clip_mode)
            cfg.setdefault('skip_nonfinite', share_with.skip_nonfinite)
            cfg.setdefault('trust', share_with.trust)
        self.cfg = make_config(B, **cfg)
        h = C.c_void_p()
        _lib.check(self.lib.cdrl_learner_create(C.byref(self.cfg), C.byref(h)), 'cdrl_learner_create')
        self.h = h
        self.frozen = bool(self.cfg.freeze_trunk)
        self.optimizer = _lib.OPTIMIZERS[self.cfg.optimizer]
        self.polyak = float(self.cfg.polyak)
        self.clip_mode = _lib.CLIP_MODES[self.cfg.clip_mode]
        self.skip_nonfinite = bool(self.cfg.skip_nonfinite)
        self.gated = self.clip_mode == 'global' or self.skip_nonfinite     # the apply steps run the gated sequence
        self.trust = bool(self.cfg.trust)       # policy_apply runs the gated sequence and obeys the trust-region latch
        used, init = (C.c_int32 * 2)(), (C.c_float * 2)()
        _lib.check(self.lib.cdrl_optimizer_slots(self.cfg.optimizer, used, init), 'cdrl_optimizer_slots')
        self.slot_init = (float(init[0]), float(init[1]))       # initial value of the adam_m / adam_v arena's slot
        lay = _lib.TrainStatsLayout()
        _lib.check(self.lib.cdrl_learner_train_stats_layout(h, C.byref(lay)), 'cdrl_learner_train_stats_layout')
        self.train_stats_layout = {n: int(getattr(lay, n)) for n, _ in lay._fields_}      # rows == 0: the ring is off
        self.tables = {m: ParamTable(self.lib, h, mid) for m, mid in (('trunk', TRUNK), ('policy', POLICY), ('value', VALUE))}
        self.params_total = int(self.lib.cdrl_learner_params_total(h))
        self.grads_total = int(self.lib.cdrl_learner_grads_total(h))
        self.workspace_bytes = int(self.lib.cdrl_learner_workspace_bytes(h))
        self.device = device
        self.hp = dict(policy_lr=3e-4, value_lr=3e-4, dynamics_lr=3e-4, clip_ratio=0.2, entropy_coef=1.0,
                       clip_norm_policy=1.0, clip_norm_value=1.0, beta1=0.9, beta2=0.999, eps=1e-7, clip_norm_dynamics=0.0)
        if self.trust:
            self.hp.update(target_kl=0.0, kl_stop_factor=1.5, kl_coef=0.0)
        self._keep = []
        self._keep_stage = {}
        self._pred_out = None
        if device is None:
            return
        dev = torch.device(device)
        if dev.type == 'cuda' and dev.index is not None and dev.index != torch.cuda.current_device():
            # one process per GPU: the engine creates its HIP streams on the CURRENT device and every entry point runs there
            raise ValueError(f'LearnerEngine(device={device!r}): call torch.cuda.set_device({dev.index}) first '
                             f'(current device is {torch.cuda.current_device()})')
        if share_with is not None:
            self.params, self.grads = share_with.params, share_with.grads
            self.adam_m, self.adam_v = share_with.adam_m, share_with.adam_v
        else:
            self.params = torch.zeros(self.params_total, dtype=torch.float32, device=dev)
            self.grads = torch.zeros(self.grads_total, dtype=torch.float32, device=dev)
            self.adam_m = torch.full((self.grads_total,), self.slot_init[0], dtype=torch.float32, device=dev)
            self.adam_v = torch.full((self.grads_total,), self.slot_init[1], dtype=torch.float32, device=dev)
        self.workspace = torch.zeros(self.workspace_bytes, dtype=torch.uint8, device=dev)
        _lib.check(self.lib.cdrl_learner_bind(h, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.adam_m),
                                              _lib.ptr(self.adam_v), _lib.ptr(self.workspace), self.workspace_bytes),
                   'cdrl_learner_bind')
        if share_with is not None and share_with.device is not None:
            # one optimizer: learning rates, clip and the Adam step counters live in the owner's device block
            _lib.check(self.lib.cdrl_learner_share_hparams(h, share_with.h), 'cdrl_learner_share_hparams')
            self.hp = share_with.hp
            self._hp_owner = share_with
        else:
            self._hp_owner = None
            self.set_hparams()

    def __del__(self):
        try:
            if getattr(self, 'h', None):
                self.lib.cdrl_learner_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def region(self, model: str, trainable: bool):
        mid = MODEL_IDS[model]
        off = int(self.lib.cdrl_learner_region_offset(self.h, mid, 1 if trainable else 0))
        n = int(self.lib.cdrl_learner_region_elems(self.h, mid, 1 if trainable else 0))
        return off, n

    def _view(self, flat, model, e, grad=False):
        off, _ = self.region(model, e['trainable'])
        if grad and model == 'old_policy':
            raise KeyError('old_policy has no gradients')
        return flat[off + e['offset']: off + e['offset'] + e['numel']].view(e['shape'])

    def param_views(self, model: str) -> Dict[str, torch.Tensor]:
        table = self.tables['policy' if model == 'old_policy' else model]
        return {e['name']: self._view(self.params, model, e) for e in table.entries}

    def grad_views(self, model: str) -> Dict[str, torch.Tensor]:
        return {e['name']: self._view(self.grads, model, e, True) for e in self.tables[model].entries if e['trainable']}

    def adam_views(self, model: str):
        t = self.tables[model]
        return ({e['name']: self._view(self.adam_m, model, e) for e in t.entries if e['trainable']},
                {e['name']: self._view(self.adam_v, model, e) for e in t.entries if e['trainable']})

    def optimizer_slots(self, model: str) -> Dict[str, Dict[str, torch.Tensor]]:
        """{Keras slot name: {tensor name: view}} of the optimizer's slots for `model`'s trainable tensors (e.g. rmsprop:
        {'rms': ...}; sgd: {}).  The views alias adam_m / adam_v, as adam_views does."""
        out = {}
        for slot, flat in zip(_lib.OPTIMIZER_SLOTS[self.optimizer], (self.adam_m, self.adam_v)):
            if slot is not None:
                out[slot] = {e['name']: self._view(flat, model, e) for e in self.tables[model].entries if e['trainable']}
        return out

    def load_params(self, model: str, values: Dict[str, np.ndarray]):
        views = self.param_views(model)
        for name, v in views.items():
            v.copy_(torch.as_tensor(np.asarray(values[name], dtype=np.float32)).reshape(v.shape))

    def export_params(self, model: str) -> Dict[str, np.ndarray]:
        return {k: v.detach().cpu().numpy().copy() for k, v in self.param_views(model).items()}

    def set_hparams(self, **kw):
        """Hyper-parameters of the following steps (cdrl_hparams).  clip_norm_* <= 0 or None: that clip is off.
        clip_norm_dynamics is the trunk's threshold with clip_mode='global'; with 'tensor' it is accepted and ignored (the trunk
        is never clipped there, as in the reference).  target_kl / kl_stop_factor / kl_coef: the trust-region block's head
        (cdrl_trust_params), on an engine built with trust=True only; target_kl None or 0: measure, never stop."""
        if getattr(self, '_hp_owner', None) is not None:
            return self._hp_owner.set_hparams(**kw)
        if not self.trust:
            for k in TRUST_PARAMS:
                if k in kw:
                    raise _lib.CdrlError(f'set_hparams({k}=...): this engine was built without trust=True')
        self.hp.update(kw)
        hp = _lib.HParams()
        for k in ('policy_lr', 'value_lr', 'dynamics_lr', 'clip_ratio', 'entropy_coef', 'beta1', 'beta2', 'eps'):
            setattr(hp, k, float(self.hp[k]))
        hp.clip_norm_policy = float(self.hp['clip_norm_policy'] or 0.0)
        hp.clip_norm_value = float(self.hp['clip_norm_value'] or 0.0)
        hp.clip_norm_dynamics = float(self.hp.get('clip_norm_dynamics') or 0.0)
        _lib.check(self.lib.cdrl_learner_set_hparams(self.h, C.byref(hp), self._stream()), 'set_hparams')
        if self.trust:
            tp = _lib.TrustParams(*(float(self.hp[k] or 0.0) for k in TRUST_PARAMS))
            _lib.check(self.lib.cdrl_learner_set_trust_params(self.h, C.byref(tp), self._stream()), 'set_trust_params')

    def set_comm_stream(self, stream: Optional['torch.cuda.Stream']):
        """See cdrl_learner_set_comm_stream (data-parallel overlap); None switches it off."""
        self._comm_stream = stream      # keep it alive: the engine holds the raw handle
        _lib.check(self.lib.cdrl_learner_set_comm_stream(self.h, C.c_void_p(stream.cuda_stream) if stream is not None else None),
                   'set_comm_stream')

    def tail_offset(self) -> int:
        """See cdrl_learner_tail_offset: first trunk-gradient element that is final when the communication stream is released."""
        off = int(self.lib.cdrl_learner_tail_offset(self.h))
        if off < 0:
            raise _lib.CdrlError('cdrl_learner_tail_offset failed')
        return off

    def reset_optimizer(self):
        """A fresh optimizer: every slot at its initial value (0; adagrad / ftrl accumulators 0.1), step counters 0."""
        self.adam_m.fill_(self.slot_init[0])
        self.adam_v.fill_(self.slot_init[1])
        _lib.check(self.lib.cdrl_learner_reset_optimizer_steps(self.h, self._stream()), 'reset_optimizer_steps')

    # ------------------------------------------------------------------ full state (learner_state.py)
    OPTIMIZER_SCALARS = ('t_policy', 't_value', 't_dynamics', 'm_cache_policy', 'm_cache_value', 'm_cache_dynamics')

    def _need_device(self, what):
        if self.device is None:
            raise _lib.CdrlError(f'{what}: this engine was built with device=None (host-only inspection): it has no arenas and no '
                                 f'device block to read or write')

    def get_optimizer_state(self) -> dict:
        """The three step counters (int) and the three Nadam m_caches (float32 values) of the device block this engine steps with
        (the owner's under share_with): one small device-to-host copy behind everything on the current stream."""
        self._need_device('get_optimizer_state')
        st = _lib.OptimizerState()
        _lib.check(self.lib.cdrl_learner_get_optimizer_state(self.h, C.byref(st), self._stream()), 'get_optimizer_state')
        return {k: (int if k.startswith('t_') else float)(getattr(st, k)) for k in self.OPTIMIZER_SCALARS}

    def set_optimizer_state(self, **values):
        """Writes the six scalars (all of them: see OPTIMIZER_SCALARS), enqueued on the current stream with no host sync.  A
        negative counter or an m_cache that is not finite and positive raises CdrlError and nothing is written."""
        self._need_device('set_optimizer_state')
        if set(values) != set(self.OPTIMIZER_SCALARS):
            raise _lib.CdrlError(f'set_optimizer_state takes exactly {self.OPTIMIZER_SCALARS}, got {sorted(values)}')
        st = _lib.OptimizerState()
        for k in self.OPTIMIZER_SCALARS:
            setattr(st, k, int(values[k]) if k.startswith('t_') else float(values[k]))
        _lib.check(self.lib.cdrl_learner_set_optimizer_state(self.h, C.byref(st), self._stream()), 'set_optimizer_state')

    def manifest(self) -> dict:
        """What a saved state must agree with to fit this engine (learner_state.make_manifest): optimizer, polyak, parameter
        tables.  Host only."""
        from . import learner_state
        return learner_state.make_manifest(self.optimizer, self.polyak, self.tables)

    def export_state(self) -> dict:
        """Everything the learner carries from one step to the next, as host copies: dict(params=, adam_m=, adam_v= flat float32
        numpy arrays -- `params` is the whole arena: every model's trainable and state regions, old_policy and the BatchNorm moving
        statistics included --, optimizer=the six scalars of get_optimizer_state, manifest=manifest()).  Three arena copies and
        one small read; an engine built with share_with exports the owner's state (the same arenas and block)."""
        self._need_device('export_state')
        owner = getattr(self, '_hp_owner', None)
        if owner is not None:
            return owner.export_state()
        opt = self.get_optimizer_state()            # (waits for the current stream: the arena copies below see finished steps)
        return dict(params=self.params.detach().cpu().numpy().copy(), adam_m=self.adam_m.detach().cpu().numpy().copy(),
                    adam_v=self.adam_v.detach().cpu().numpy().copy(), optimizer=opt, manifest=self.manifest())

    def import_state(self, state: dict):
        """Inverse of export_state.  Validates first and writes afterwards: a state whose optimizer or parameter tables differ
        from this engine's, whose arenas have another size or type, or whose scalars the library would refuse raises CdrlError
        naming the first difference, and no arena byte or counter has changed.  Batch size, compute mode, freeze_trunk and
        train_stats of the exporting engine are free (the tables and region offsets do not depend on them)."""
        self._need_device('import_state')
        owner = getattr(self, '_hp_owner', None)
        if owner is not None:
            return owner.import_state(state)
        from . import learner_state
        diff = learner_state.manifest_difference(state.get('manifest', {}), self.manifest())
        if diff is not None:
            raise _lib.CdrlError(f'import_state: the state does not fit this engine -- {diff}')
        arrays = {}
        for name, dst in (('params', self.params), ('adam_m', self.adam_m), ('adam_v', self.adam_v)):
            a = state.get(name)
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.shape != (dst.numel(),):
                raise _lib.CdrlError(f'import_state: {name} must be a flat float32 array of {dst.numel()} elements, got '
                                     f'{type(a).__name__} {getattr(a, "dtype", "")} {getattr(a, "shape", "")}')
            arrays[name] = a
        opt = state.get('optimizer', {})
        if set(opt) != set(self.OPTIMIZER_SCALARS):
            raise _lib.CdrlError(f'import_state: optimizer scalars {sorted(opt)} are not {sorted(self.OPTIMIZER_SCALARS)}')
        for k in self.OPTIMIZER_SCALARS:            # the library's own rule, checked here so that the arenas are not written first
            v = opt[k]
            if k.startswith('t_') and not (isinstance(v, (int, np.integer)) and 0 <= int(v) < 2 ** 31):
                raise _lib.CdrlError(f'import_state: {k} = {v!r} is not a step count')
            if k.startswith('m_') and not (np.isfinite(np.float32(v)) and np.float32(v) > 0):
                raise _lib.CdrlError(f'import_state: {k} = {v!r} is not a finite positive number')
        for name, dst in (('params', self.params), ('adam_m', self.adam_m), ('adam_v', self.adam_v)):
            dst.copy_(torch.from_numpy(arrays[name]))
        self.set_optimizer_state(**opt)

    def gate_stats(self) -> dict:
        """Counters and last norms / scales of the gradient gate (cdrl_gate_stats; the owner's block under share_with): per head
        ('policy', 'value') dict(skipped=, applied= apply steps since create or gate_reset, norm=, scale= of the head's list and
        norm_dynamics=, scale_dynamics= of the trunk's at that head's last apply; a norm that was not needed reads 0).  ONE
        device-to-host copy behind everything on the current stream.  CdrlError when neither option is on."""
        self._need_device('gate_stats')
        gs = _lib.GateStats()
        _lib.check(self.lib.cdrl_learner_gate_stats(self.h, C.byref(gs), self._stream()), 'gate_stats')
        return {head: dict(skipped=int(gs.skipped[i]), applied=int(gs.applied[i]), norm=float(gs.norm[i]), scale=float(gs.scale[i]),
                           norm_dynamics=float(gs.norm_dynamics[i]), scale_dynamics=float(gs.scale_dynamics[i]))
                for i, head in enumerate(('policy', 'value'))}

    def gate_reset(self):
        """Skip / apply counters of the gradient gate to zero (enqueued on the current stream)."""
        self._need_device('gate_reset')
        _lib.check(self.lib.cdrl_learner_gate_reset(self.h, self._stream()), 'gate_reset')

    def trust_stats(self) -> dict:
        """The trust-region block (cdrl_trust_stats; the owner's under share_with): target_kl, kl_stop_factor, kl_coef as set;
        kl_last, kl_max, kl_sum, passes of the measured passes since trust_reset; stop (the latch), stop_pass (-1 before), armed,
        skipped (policy applies the latch left out).  ONE device-to-host copy behind everything on the current stream."""
        self._need_device('trust_stats')
        ts = _lib.TrustStats()
        _lib.check(self.lib.cdrl_learner_trust_stats(self.h, C.byref(ts), self._stream()), 'trust_stats')
        return {n: (float if t in (C.c_float, C.c_double) else int)(getattr(ts, n)) for n, t in ts._fields_}

    def trust_reset(self):
        """Latch, counters and sums of the trust-region block to their initial values (enqueued on the current stream)."""
        self._need_device('trust_reset')
        _lib.check(self.lib.cdrl_learner_trust_reset(self.h, self._stream()), 'trust_reset')

    def _stats_owner(self):
        owner = getattr(self, '_hp_owner', None)
        return owner if owner is not None and owner.train_stats_layout['rows'] > 0 else self

    def train_stats_reset(self):
        """Empties the train-stats ring without reading it (enqueued on the current stream)."""
        _lib.check(self.lib.cdrl_learner_train_stats_reset(self.h, self._stream()), 'train_stats_reset')

    def train_stats(self):
        """The update diagnostics written by the apply steps since the last call (this engine's and those of the engines sharing
        its ring), oldest first: dict(rows=[...], dropped=rows lost to a full ring); see train_stats.decode for a row.  ONE
        device-to-host copy, then the ring is reset.  None when the ring is off (train_stats=0)."""
        if self.train_stats_layout['rows'] <= 0:
            return None
        from . import train_stats as ts
        own = self._stats_owner()           # the ring lives in the workspace of the engine whose hyper-parameters are shared
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(self.lib.cdrl_learner_train_stats_buffer(self.h, C.byref(p), C.byref(n)), 'train_stats_buffer')
        off = p.value - own.workspace.data_ptr()
        if off < 0 or off + n.value > own.workspace.numel():
            raise _lib.CdrlError('train-stats ring outside the workspace')
        block = own.workspace[off: off + n.value].view(torch.float32).cpu().numpy()
        self.train_stats_reset()
        names = {m: [e['name'] for e in self.tables[m].entries if e['trainable']] for m in ('policy', 'value', 'trunk')}
        return ts.decode(block, self.train_stats_layout, names)

    def buffer(self, which: int, shape=None) -> torch.Tensor:
        """Zero-copy torch view of an engine-owned workspace buffer."""
        p = C.c_void_p()
        n = C.c_int64()
        _lib.check(self.lib.cdrl_learner_get_buffer(self.h, which, C.byref(p), C.byref(n)), 'get_buffer')
        base = self.workspace.data_ptr()
        off = p.value - base
        t = self.workspace[off: off + 4 * n.value].view(torch.float32)
        return t.view(shape) if shape is not None else t

    def check_guards(self):
        """(bands that lost their pattern, workspace byte offset of the first one or -1): the out-of-bounds canaries behind every
        workspace tensor of a learner created with CDRL_GUARD=1 in the environment (cdrl_learner_check_guards)."""
        bad, first = C.c_int64(0), C.c_int64(-1)
        _lib.check(self.lib.cdrl_learner_check_guards(self.h, self._stream(), C.byref(bad), C.byref(first)), 'check_guards')
        return int(bad.value), int(first.value)

    def named_buffer(self, name: str, dtype=torch.float32, shape=None) -> torch.Tensor:
        """Zero-copy view of a named internal tensor (cdrl_learner_named_buffer; parity tests)."""
        p = C.c_void_p()
        n = C.c_int64()
        _lib.check(self.lib.cdrl_learner_named_buffer(self.h, name.encode(), C.byref(p), C.byref(n)), f'named_buffer({name})')
        off = p.value - self.workspace.data_ptr()
        t = self.workspace[off: off + n.value].view(dtype)
        return t.view(shape) if shape is not None else t

    # ------------------------------------------------------------------ staging
    def stage(self, batch: dict, slot: str) -> dict:
        """Copies a (nested) batch into persistent device buffers owned by the engine and returns those.
        The step entry points are replayed from captured hipGraphs keyed on their pointer arguments, so
        minibatches that live in fresh tensors every time (tf.data-style gathers) go through fixed
        staging buffers (one D2D copy, ~0.05 ms for a 256x4x90x120x3 minibatch)."""
        store = self._keep_stage.setdefault(slot, {})
        # hipGraph replay is opt-in (CDRL_GRAPH=1; eager launches are faster on this stack): without it the
        # entry points take any contiguous device tensor, and the staging copy (a 133 MB D2D copy per B = 256 pass) is skipped
        direct = os.environ.get('CDRL_GRAPH', '0') in ('', '0')

        def put(key, t):
            if t is None:
                return None
            if direct and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous():
                return t
            buf = store.get(key)
            if buf is None or buf.shape != t.shape:
                buf = torch.empty_like(t, memory_format=torch.contiguous_format)
                store[key] = buf
            buf.copy_(t)
            return buf
        out = {}
        for k, v in batch.items():
            out[k] = {kk: put(f'{k}/{kk}', vv) for kk, vv in v.items()} if isinstance(v, dict) else put(k, v)
        return out

    # ------------------------------------------------------------------ steps
    def _states(self, batch):
        st = batch['states'] if 'states' in batch else batch
        return st['state_image'], st['state_road'], st['state_vehicle'], st['state_navigation']

    @staticmethod
    def _chk(t, shape, name):
        if t is None:
            return
        if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f'{name}: expected contiguous float32 cuda tensor of shape {tuple(shape)}, '
                             f'got {tuple(t.shape)} {t.dtype} contiguous={t.is_contiguous()} cuda={t.is_cuda}')

    def _check_states(self, img, road, veh, nav):
        c = self.cfg
        self._chk(img, (c.B, c.T, c.H, c.W, 3), 'state_image')
        self._chk(road, (c.B, c.T, c.road), 'state_road')
        self._chk(veh, (c.B, c.T, c.vehicle), 'state_vehicle')
        self._chk(nav, (c.B, c.T, c.navigation), 'state_navigation')

    def policy_forward_backward(self, batch, grad_scale=1.0):
        pb = self._policy_batch(batch)
        _lib.check(self.lib.cdrl_learner_policy_forward_backward(self.h, C.byref(pb), float(grad_scale), self._stream()),
                   'policy_forward_backward')

    def _policy_batch(self, batch, resample=False):
        """The checked cdrl_policy_batch of a batch dict.  resample: the entry point draws u on the device and ignores the batch's,
        so a batch without one gets a placeholder."""
        c = self.cfg
        if resample and 'u' not in batch:
            batch = dict(batch, u=batch['old_log_prob'])
        img, road, veh, nav = self._states(batch)
        self._check_states(img, road, veh, nav)
        self._chk(batch['advantages'], (c.B,), 'advantages')
        for k in ('old_log_prob', 'u', 'du_da', 'du_db'):
            self._chk(batch.get(k), (c.B, c.A), k)
        for k in ('speed', 'similarity'):
            if batch[k].numel() != c.B:
                raise ValueError(f'{k}: expected {c.B} elements')
        self._chk(batch.get('anchor'), (c.B, 2, c.A), 'anchor')
        return _lib.PolicyBatch(anchor=batch['anchor'].data_ptr() if batch.get('anchor') is not None else None,
                                image=img.data_ptr(), road=road.data_ptr(), vehicle=veh.data_ptr(),
                                navigation=nav.data_ptr(), advantages=batch['advantages'].data_ptr(),
                                old_log_prob=batch['old_log_prob'].data_ptr(), speed=batch['speed'].data_ptr(),
                                similarity=batch['similarity'].data_ptr(), u=batch['u'].data_ptr(),
                                du_dalpha=batch['du_da'].data_ptr() if batch.get('du_da') is not None else None,
                                du_dbeta=batch['du_db'].data_ptr() if batch.get('du_db') is not None else None)

    def policy_forward(self, states):
        """train-mode forward of trunk + policy head; returns (alpha, beta) views (B, A) of the current policy."""
        img, road, veh, nav = self._states(states)
        self._check_states(img, road, veh, nav)
        _lib.check(self.lib.cdrl_learner_policy_forward(self.h, _lib.ptr(img), _lib.ptr(road), _lib.ptr(veh),
                                                        _lib.ptr(nav), self._stream()), 'policy_forward')
        aux = self.buffer(_lib.BUF_AUX_P, (self.cfg.B, 4, self.cfg.A))
        return aux[:, 0], aux[:, 1]

    def policy_backward(self, batch, grad_scale=1.0):
        pb = self._policy_batch(batch)
        _lib.check(self.lib.cdrl_learner_policy_backward(self.h, C.byref(pb), float(grad_scale), self._stream()),
                   'policy_backward')

    def policy_forward_backward_resample(self, batch, seed: int, offset: int, grad_scale=1.0):
        """F8-faithful step with the Beta re-sampling done on the device (no torch.distributions)."""
        pb = self._policy_batch(batch, resample=True)
        _lib.check(self.lib.cdrl_learner_policy_forward_backward_resample(self.h, C.byref(pb), int(seed), int(offset),
                                                                         float(grad_scale), self._stream()),
                   'policy_forward_backward_resample')

    def policy_apply(self):
        _lib.check(self.lib.cdrl_learner_policy_apply(self.h, self._stream()), 'policy_apply')

    def value_forward_backward(self, batch, grad_scale=1.0):
        c = self.cfg
        img, road, veh, nav = self._states(batch)
        self._check_states(img, road, veh, nav)
        self._chk(batch['returns'], (c.B, 2), 'returns')
        vb = _lib.ValueBatch(image=img.data_ptr(), road=road.data_ptr(), vehicle=veh.data_ptr(),
                             navigation=nav.data_ptr(), returns=batch['returns'].data_ptr(),
                             speed=batch['speed'].data_ptr(), similarity=batch['similarity'].data_ptr())
        _lib.check(self.lib.cdrl_learner_value_forward_backward(self.h, C.byref(vb), float(grad_scale), self._stream()),
                   'value_forward_backward')

    def value_apply(self):
        _lib.check(self.lib.cdrl_learner_value_apply(self.h, self._stream()), 'value_apply')

    # Joint policy + value update (opt-in, include/cdrl.h): one trunk forward and one trunk backward per minibatch.  `batch` is the
    # policy batch dict plus 'returns' (B, 2); the value loss takes the batch's speed / similarity.
    def _joint_batch(self, batch, resample=False):
        self._chk(batch['returns'], (self.cfg.B, 2), 'returns')
        return self._policy_batch(batch, resample)

    def joint_forward_backward(self, batch, grad_scale=1.0):
        """Stored-action / injected-Jacobian policy loss + value loss on ONE train-mode trunk forward, one trunk backward."""
        pb = self._joint_batch(batch)
        _lib.check(self.lib.cdrl_learner_joint_forward_backward(self.h, C.byref(pb), _lib.ptr(batch['returns']), float(grad_scale),
                                                                self._stream()), 'joint_forward_backward')

    def joint_forward_backward_resample(self, batch, seed: int, offset: int, grad_scale=1.0):
        """The joint pass with the Beta re-sampling done on the device (as policy_forward_backward_resample)."""
        pb = self._joint_batch(batch, resample=True)
        _lib.check(self.lib.cdrl_learner_joint_forward_backward_resample(self.h, C.byref(pb), _lib.ptr(batch['returns']), int(seed),
                                                                         int(offset), float(grad_scale), self._stream()),
                   'joint_forward_backward_resample')

    def joint_apply(self):
        """Trunk step ONCE, then the policy head (old_policy <- policy in front), then the value head."""
        _lib.check(self.lib.cdrl_learner_joint_apply(self.h, self._stream()), 'joint_apply')

    def joint_step(self, batch):
        with self.sequence():
            self.joint_forward_backward(batch)
            self.joint_apply()

    # Behaviour cloning (include/cdrl.h).  `batch`: states, 'u' (B, A) expert actions in the unit interval, optional
    # 'weight' (B), optional 'speed' / 'similarity' (B each, together), optional 'returns' (B, 2; needs the two targets).
    def _clone_batch(self, batch):
        c = self.cfg
        img, road, veh, nav = self._states(batch)
        self._check_states(img, road, veh, nav)
        if batch.get('u') is None:
            raise ValueError('u: a clone batch needs the expert actions, shape (B, A) in the unit interval')
        self._chk(batch['u'], (c.B, c.A), 'u')
        self._chk(batch.get('weight'), (c.B,), 'weight')
        self._chk(batch.get('returns'), (c.B, 2), 'returns')
        targets = [batch.get(k) for k in ('speed', 'similarity')]
        if (targets[0] is None) != (targets[1] is None):
            raise ValueError('speed and similarity targets come together: give both, or neither')
        if batch.get('returns') is not None and targets[0] is None:
            raise ValueError('returns: the value loss needs the speed and similarity targets as well')
        for k, t in zip(('speed', 'similarity'), targets):
            self._chk(t, (c.B,), k)
        p = lambda t: t.data_ptr() if t is not None else None
        return _lib.CloneBatch(image=img.data_ptr(), road=road.data_ptr(), vehicle=veh.data_ptr(), navigation=nav.data_ptr(),
                               u=batch['u'].data_ptr(), weight=p(batch.get('weight')), speed=p(targets[0]), similarity=p(targets[1]),
                               returns=p(batch.get('returns')))

    def clone_forward_backward(self, batch, policy_weight=1.0, value_weight=0.0, aux_weight=1.0, grad_scale=1.0):
        """Behaviour-cloning pass: the clone loss in the place of the policy loss; with batch['returns'] also the value loss, on one
        trunk forward and backward like the joint pass.  The weights scale gradients only (metrics stay unscaled)."""
        cb = self._clone_batch(batch)
        _lib.check(self.lib.cdrl_learner_clone_forward_backward(self.h, C.byref(cb), float(policy_weight), float(value_weight),
                                                                float(aux_weight), float(grad_scale), self._stream()),
                   'clone_forward_backward')

    def clone_step(self, batch, policy_weight=1.0, value_weight=0.0, aux_weight=1.0):
        """Clone pass, then the matching apply: policy_apply, or joint_apply when the batch carries returns."""
        with self.sequence():
            self.clone_forward_backward(batch, policy_weight, value_weight, aux_weight)
            if batch.get('returns') is not None:
                self.joint_apply()
            else:
                self.policy_apply()

    # Expert demonstrations inside the PPO update (include/cdrl.h).  `batch`: a policy batch dict plus 'demo_u' (B, A)
    # expert actions in the unit interval and 'demo_w' (B): rows with demo_w > 0 are demonstration rows, the others PPO rows.
    def _demo_batch(self, batch, resample=False):
        c = self.cfg
        for k, shape in (('demo_u', (c.B, c.A)), ('demo_w', (c.B,))):
            if batch.get(k) is None:
                raise ValueError(f'{k}: a demonstration batch needs it, shape {shape}')
            self._chk(batch[k], shape, k)
        if batch.get('anchor') is not None:
            raise ValueError('anchor: a demonstration batch carries none (the trust-region sweep has no demonstration rows)')
        return self._policy_batch(batch, resample)

    def demo_forward_backward(self, batch, grad_scale=1.0):
        """The policy pass with the mixed loss (stored actions / injected Jacobians on the PPO rows)."""
        pb = self._demo_batch(batch)
        _lib.check(self.lib.cdrl_learner_demo_forward_backward(self.h, C.byref(pb), _lib.ptr(batch['demo_u']), _lib.ptr(batch['demo_w']),
                                                               float(grad_scale), self._stream()), 'demo_forward_backward')

    def demo_forward_backward_resample(self, batch, seed: int, offset: int, grad_scale=1.0):
        """... with the Beta re-sampling on the device: u is drawn for all B rows as in policy_forward_backward_resample, the draw
        of a demonstration row is ignored."""
        pb = self._demo_batch(batch, resample=True)
        _lib.check(self.lib.cdrl_learner_demo_forward_backward_resample(self.h, C.byref(pb), _lib.ptr(batch['demo_u']),
                                                                        _lib.ptr(batch['demo_w']), int(seed), int(offset),
                                                                        float(grad_scale), self._stream()),
                   'demo_forward_backward_resample')

    def demo_step(self, batch):
        with self.sequence():
            self.demo_forward_backward(batch)
            self.policy_apply()

    def set_demo_block(self, block: Optional[torch.Tensor]):
        """block: a zeroed float64 device tensor of DEMO_BLOCK_DOUBLES elements (cdrl_demo_stats) that every later demonstration pass
        of this engine adds to, or None.  Engines of several minibatch sizes may share one."""
        self._need_device('set_demo_block')
        if block is not None and (block.dtype != torch.float64 or block.numel() != DEMO_BLOCK_DOUBLES or not block.is_cuda
                                  or not block.is_contiguous()):
            raise ValueError(f'set_demo_block: a contiguous float64 device tensor of {DEMO_BLOCK_DOUBLES} elements, got '
                             f'{tuple(block.shape)} {block.dtype}')
        self._demo_block = block        # (kept alive: the library holds its address)
        _lib.check(self.lib.cdrl_learner_set_demo_block(self.h, _lib.ptr(block)), 'set_demo_block')

    # Contrastive pre-training of the trunk (include/cdrl.h).  `states`: the four state tensors of B = 2N rows, rows
    # i and i + N being two views of one observation.
    def repr_forward_backward(self, states, temperature=0.1, grad_scale=1.0):
        """Representation pass: train-mode trunk forward, NT-Xent on the trunk's output, trunk backward.  No head runs."""
        img, road, veh, nav = self._states(states)
        self._check_states(img, road, veh, nav)
        _lib.check(self.lib.cdrl_learner_repr_forward_backward(self.h, _lib.ptr(img), _lib.ptr(road), _lib.ptr(veh), _lib.ptr(nav),
                                                               float(temperature), float(grad_scale), self._stream()),
                   'repr_forward_backward')

    def trunk_apply(self):
        """The trunk's optimizer step alone (dynamics_lr, unclipped) and one tick of its step counter."""
        _lib.check(self.lib.cdrl_learner_trunk_apply(self.h, self._stream()), 'trunk_apply')

    def repr_step(self, states, temperature=0.1):
        with self.sequence():
            self.repr_forward_backward(states, temperature)
            self.trunk_apply()

    def sequence(self):
        """Context manager around a run of learner calls on the current stream with nothing of the caller's own between them (one
        minibatch on one GPU: policy pass, apply, value pass, apply): the hand-overs between the caller's stream and the engine's
        happen once, around the whole run (`cdrl_learner_sequence_begin / _end`).  Not for runs with collectives in between."""
        eng = self

        class _Seq:
            def __enter__(self_inner):          # (re-entrant on the Python side: only the outermost level brackets)
                depth = getattr(eng, '_seq_depth', 0)
                if depth == 0:
                    _lib.check(eng.lib.cdrl_learner_sequence_begin(eng.h, eng._stream()), 'sequence_begin')
                eng._seq_depth = depth + 1
                return eng

            def __exit__(self_inner, *exc):
                eng._seq_depth -= 1
                if eng._seq_depth == 0:
                    _lib.check(eng.lib.cdrl_learner_sequence_end(eng.h, eng._stream()), 'sequence_end')
                return False

        return _Seq()

    def policy_step(self, batch):
        with self.sequence():
            self.policy_forward_backward(batch)
            self.policy_apply()

    def value_step(self, batch):
        with self.sequence():
            self.value_forward_backward(batch)
            self.value_apply()

    def update_old_policy(self):
        _lib.check(self.lib.cdrl_learner_update_old_policy(self.h, self._stream()), 'update_old_policy')

    def trunk_forward_train(self, states):
        img, road, veh, nav = self._states(states)
        self._check_states(img, road, veh, nav)
        _lib.check(self.lib.cdrl_learner_trunk_forward_train(self.h, _lib.ptr(img), _lib.ptr(road), _lib.ptr(veh),
                                                             _lib.ptr(nav), self._stream()), 'trunk_forward_train')
        return self.buffer(_lib.BUF_DYNAMICS, (self.cfg.B, self.cfg.dyn))

    def predict(self, states):
        c = self.cfg
        st = states['states'] if 'states' in states else states
        staged = self.stage({k: st[k] for k in ('state_image', 'state_road', 'state_vehicle', 'state_navigation')}, 'predict')
        img, road, veh, nav = self._states(staged)
        self._check_states(img, road, veh, nav)
        if self._pred_out is None:       # persistent outputs: the captured graph writes to fixed addresses
            self._pred_out = (torch.empty((c.B, 4, c.A), dtype=torch.float32, device=img.device),
                              torch.empty((c.B, 4), dtype=torch.float32, device=img.device),
                              torch.empty((c.B, c.dyn), dtype=torch.float32, device=img.device))
        dist, value, dyn = self._pred_out
        _lib.check(self.lib.cdrl_learner_predict(self.h, _lib.ptr(img), _lib.ptr(road), _lib.ptr(veh), _lib.ptr(nav),
                                                 _lib.ptr(dist), _lib.ptr(value), _lib.ptr(dyn), self._stream()), 'predict')
        return dict(alpha=dist[:, 0], beta=dist[:, 1], mean=dist[:, 2], std=dist[:, 3], value=value[:, :2],
                    speed=value[:, 2], similarity=value[:, 3], dynamics=dyn)

    def metrics(self, which='policy'):
        if which == 'representation':
            m = self.buffer(_lib.BUF_METRICS_R).cpu().numpy()
            return {k: float(m[i]) for i, k in enumerate(REPRESENTATION_METRICS)}
        m = self.buffer(_lib.BUF_METRICS_P if which in ('policy', 'clone', 'demo') else _lib.BUF_METRICS_V).cpu().numpy()
        if which == 'policy':
            keys = ('loss', 'policy_loss', 'entropy', 'speed_loss', 'similarity_loss', 'ratio', 'log_prob')
        elif which == 'clone':      # the policy block as a clone pass leaves it
            keys = CLONE_METRICS
        elif which == 'demo':       # ... as a demonstration pass leaves it
            keys = DEMO_METRICS
        else:
            keys = ('loss', 'value_loss', 'speed_loss', 'similarity_loss')
        return {k: float(m[i]) for i, k in enumerate(keys)}


TRUST_PARAMS = ('target_kl', 'kl_stop_factor', 'kl_coef')      # cdrl_trust_params, in this order
BETA_KL_METRICS = ('kl', 'kl_row_max', 'kl_per_action')        # cdrl_beta_kl's metrics


def beta_kl(lin: torch.Tensor, anchor: torch.Tensor, kl_coef: float = 0.0, grad_scale: float = 1.0, dlin: torch.Tensor = None,
            metrics: torch.Tensor = None):
    """Analytic KL(Beta(anchor) || Beta(policy head on lin)) (cdrl_beta_kl, one launch): lin (B, 2A+2) linear head outputs, anchor
    (B, 2, A) alpha0 / beta0.  kl_coef > 0: dlin (B, 2A+2) += grad_scale * kl_coef * dKL/dlin in place; kl_coef == 0: dlin is not
    touched (and may be None).  -> metrics (3,) device tensor: BETA_KL_METRICS."""
    lib = _lib.load()
    for name, t in (('lin', lin), ('anchor', anchor), ('dlin', dlin)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
            raise ValueError(f'beta_kl: {name} must be a contiguous float32 device tensor, got {tuple(t.shape)} {t.dtype}')
    if lin.dim() != 2 or lin.shape[1] < 4 or lin.shape[1] % 2:
        raise ValueError(f'beta_kl: lin must be (B, 2A+2), got {tuple(lin.shape)}')
    B, A = int(lin.shape[0]), (int(lin.shape[1]) - 2) // 2
    if tuple(anchor.shape) != (B, 2, A):
        raise ValueError(f'beta_kl: anchor must be ({B}, 2, {A}), got {tuple(anchor.shape)}')
    if dlin is not None and tuple(dlin.shape) != tuple(lin.shape):
        raise ValueError(f'beta_kl: dlin must have the shape of lin {tuple(lin.shape)}, got {tuple(dlin.shape)}')
    if dlin is None and kl_coef != 0.0:
        raise ValueError('beta_kl: kl_coef != 0 needs a dlin to add to')
    if metrics is None:
        metrics = torch.empty(3, dtype=torch.float32, device=lin.device)
    _lib.check(lib.cdrl_beta_kl(_lib.ptr(lin), _lib.ptr(anchor), B, A, float(kl_coef), float(grad_scale), _lib.ptr(dlin),
                                _lib.ptr(metrics), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'cdrl_beta_kl')
    return metrics


# slots 0..7 of CDRL_BUF_METRICS_P after a clone pass (cdrl_beta_clone_loss, include/cdrl.h)
CLONE_METRICS = ('loss', 'clone_loss', 'entropy', 'speed_loss', 'similarity_loss', 'weight', 'log_prob', 'mode_error')


# slots 0..10 of CDRL_BUF_METRICS_P after a demonstration pass (cdrl_beta_mixed_policy_loss, include/cdrl.h)
DEMO_METRICS = ('loss', 'policy_loss', 'entropy', 'speed_loss', 'similarity_loss', 'ratio', 'log_prob', 'demo_loss', 'demo_log_prob',
                'demo_mode_error', 'demo_rows')
DEMO_BLOCK_DOUBLES = 5          # cdrl_demo_stats: four double sums and an int64 pass count


def demo_block(device) -> torch.Tensor:
    """A zeroed demonstration block (cdrl_demo_stats) for LearnerEngine.set_demo_block."""
    return torch.zeros(DEMO_BLOCK_DOUBLES, dtype=torch.float64, device=device)


def read_demo_block(block: torch.Tensor) -> dict:
    """ONE device-to-host copy of a demonstration block: the four sums and the pass count."""
    host = block.cpu()
    out = {n: float(host[i]) for i, n in enumerate(('loss_sum', 'log_prob_sum', 'mode_error_sum', 'rows_sum'))}
    out['passes'] = int(host.view(torch.int64)[4])
    return out


def mixed_policy_loss(lin, adv, old_logp, speed, similarity, u, demo_u, demo_w, clip_ratio: float, entropy_coef: float, du_da=None,
                      du_db=None, grad_scale: float = 1.0, block: torch.Tensor = None):
    """cdrl_beta_mixed_policy_loss, one launch: lin (B, 2A+2) -> (dlin (B, 2A+2), metrics (16,), aux (B, 4, A)) device tensors."""
    lib = _lib.load()
    B, A = int(lin.shape[0]), (int(lin.shape[1]) - 2) // 2
    for name, t, shape in (('lin', lin, (B, 2 * A + 2)), ('adv', adv, (B,)), ('old_logp', old_logp, (B, A)), ('speed', speed, (B,)),
                           ('similarity', similarity, (B,)), ('u', u, (B, A)), ('du_da', du_da, (B, A)), ('du_db', du_db, (B, A)),
                           ('demo_u', demo_u, (B, A)), ('demo_w', demo_w, (B,))):
        if t is not None:
            LearnerEngine._chk(t, shape, f'mixed_policy_loss: {name}')
    dlin = torch.empty_like(lin)
    metrics = torch.zeros(16, dtype=torch.float32, device=lin.device)
    aux = torch.empty((B, 4, A), dtype=torch.float32, device=lin.device)
    hp = torch.empty(16, dtype=torch.float32, device=lin.device)
    _lib.check(lib.cdrl_beta_mixed_policy_loss(_lib.ptr(lin), _lib.ptr(adv), _lib.ptr(old_logp), _lib.ptr(speed), _lib.ptr(similarity),
                                               _lib.ptr(u), _lib.ptr(du_da), _lib.ptr(du_db), _lib.ptr(demo_u), _lib.ptr(demo_w),
                                               float(clip_ratio), float(entropy_coef), B, A, float(grad_scale), _lib.ptr(dlin),
                                               _lib.ptr(metrics), _lib.ptr(aux), _lib.ptr(hp), _lib.ptr(block),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'cdrl_beta_mixed_policy_loss')
    return dlin, metrics, aux


# slots 0..5 of CDRL_BUF_METRICS_R after a representation pass (cdrl_ntxent_loss, include/cdrl.h)
REPRESENTATION_METRICS = ('loss', 'accuracy', 'similarity_pos', 'similarity_neg', 'embedding_norm', 'temperature')


def ntxent_loss(z: torch.Tensor, temperature: float, grad_scale: float = 1.0):
    """NT-Xent over pairs of views (cdrl_ntxent_loss): z (B, D) float32 on the device, B = 2N, rows i and i + N the two views of one
    observation.  -> (dz (B, D) = grad_scale * dL/dz, metrics (16,): loss, top-1 accuracy, pair cosine, negatives' cosine, mean
    norm, temperature).  Owns its workspace."""
    lib = _lib.load()
    if z.dim() != 2 or z.dtype != torch.float32 or not z.is_contiguous() or not z.is_cuda:
        raise ValueError(f'ntxent_loss: z must be a contiguous float32 (B, D) device tensor, got {tuple(z.shape)} {z.dtype}')
    B, D = z.shape
    n = int(lib.cdrl_ntxent_workspace_floats(B, D))
    if n < 0:
        raise _lib.CdrlError('cdrl_ntxent_workspace_floats: ' + lib.cdrl_last_error().decode())
    ws = torch.empty(n, dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z)
    metrics = torch.empty(16, dtype=torch.float32, device=z.device)
    _lib.check(lib.cdrl_ntxent_loss(_lib.ptr(z), B, D, float(temperature), float(grad_scale), _lib.ptr(dz), _lib.ptr(metrics),
                                    _lib.ptr(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'cdrl_ntxent_loss')
    return dz, metrics


def gae_returns(rewards: torch.Tensor, values_be: torch.Tensor, gamma: float, lambda_: float, scale: float = 2.0):
    """Device GAE / returns for one env shard (cdrl_gae_returns).  rewards (N+1,), values_be (N+1,2)."""
    lib = _lib.load()
    n = rewards.numel() - 1
    dev = rewards.device
    returns = torch.empty(n, dtype=torch.float32, device=dev)
    returns_be = torch.empty((n, 2), dtype=torch.float32, device=dev)
    adv_raw = torch.empty(n, dtype=torch.float32, device=dev)
    adv = torch.empty(n, dtype=torch.float32, device=dev)
    scratch = torch.empty(2 * (n + 1) + 2, dtype=torch.float64, device=dev)
    _lib.check(lib.cdrl_gae_returns(_lib.ptr(rewards), _lib.ptr(values_be), n, float(gamma), float(lambda_), float(scale),
                                    _lib.ptr(returns), _lib.ptr(returns_be), _lib.ptr(adv_raw), _lib.ptr(adv),
                                    _lib.ptr(scratch), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'gae_returns')
    return returns, returns_be, adv_raw, adv


def gae_returns_segments(rewards: torch.Tensor, values_be: torch.Tensor, lengths, gamma: float, lambda_: float, scale: float = 2.0):
    """Device GAE / returns for S trajectories in ONE launch (cdrl_gae_returns_segments), one workgroup per trajectory.
    `lengths`: host list of the S row counts n_s >= 1 (N = their sum); rewards (N+S,), values_be (N+S, 2): the trajectories one after
    the other, each followed by its own bootstrap entry.  -> packed returns (N,), returns_be (N, 2), adv_raw (N,), adv (N,), every
    trajectory's rows bit-identical to `gae_returns` on that trajectory alone.  One host-to-device copy (the row offsets), no
    device-to-host read."""
    lengths = [int(n) for n in lengths]
    S, n = len(lengths), sum(lengths)
    if S < 1 or min(lengths) < 1:
        raise ValueError(f'gae_returns_segments: every trajectory needs at least one row (lengths {lengths})')
    if n + S != rewards.numel() or 2 * (n + S) != values_be.numel():
        raise ValueError(f'gae_returns_segments: {S} trajectories of {n} rows in all need {n + S} rewards and ({n + S}, 2) values '
                         f'(one bootstrap entry each), got {rewards.numel()} and {tuple(values_be.shape)}')
    lib = _lib.load()
    dev = rewards.device
    offsets = [0] * (S + 1)
    for s, k in enumerate(lengths):
        offsets[s + 1] = offsets[s] + k
    seg_off = torch.tensor(offsets, dtype=torch.int32, device=dev)
    returns = torch.empty(n, dtype=torch.float32, device=dev)
    returns_be = torch.empty((n, 2), dtype=torch.float32, device=dev)
    adv_raw = torch.empty(n, dtype=torch.float32, device=dev)
    adv = torch.empty(n, dtype=torch.float32, device=dev)
    scratch = torch.empty(int(lib.cdrl_gae_segments_scratch_doubles(n, S)), dtype=torch.float64, device=dev)
    _lib.check(lib.cdrl_gae_returns_segments(_lib.ptr(rewards), _lib.ptr(values_be), _lib.ptr(seg_off), S, n, float(gamma),
                                             float(lambda_), float(scale), _lib.ptr(returns), _lib.ptr(returns_be), _lib.ptr(adv_raw),
                                             _lib.ptr(adv), _lib.ptr(scratch), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               'gae_returns_segments')
    return returns, returns_be, adv_raw, adv


VTRACE_CHUNK = 2048     # VTRACE_CH (csrc/cdrl_kernels.h): rows per LDS chunk of cdrl_vtrace_segments' recurrences


def vtrace_segments(rewards: torch.Tensor, values_be: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, actions: torch.Tensor,
                    log_prob_old: torch.Tensor, lengths, gamma: float, lambda_: float, rho_bar: float = 1.0, c_bar: float = 1.0,
                    scale: float = 2.0):
    """V-trace targets for S replayed trajectories in ONE launch (cdrl_vtrace_segments), one workgroup per trajectory.
    `lengths`, rewards (N+S,), values_be (N+S, 2) as `gae_returns_segments` takes them -- values_be from the CURRENT value head --;
    alpha, beta (N, A) of the current policy, actions (N, A) in [0, 1] and log_prob_old (N, A) as stored.  -> packed returns (N,),
    returns_be (N, 2), adv_raw (N,), adv (N,), rho (N,) = the unclipped joint ratio.  One host-to-device copy (the row offsets), no
    device-to-host read."""
    lengths = [int(n) for n in lengths]
    S, n = len(lengths), sum(lengths)
    if S < 1 or min(lengths) < 1:
        raise ValueError(f'vtrace_segments: every trajectory needs at least one row (lengths {lengths})')
    if n + S != rewards.numel() or 2 * (n + S) != values_be.numel():
        raise ValueError(f'vtrace_segments: {S} trajectories of {n} rows in all need {n + S} rewards and ({n + S}, 2) values '
                         f'(one bootstrap entry each), got {rewards.numel()} and {tuple(values_be.shape)}')
    A = int(actions.shape[-1]) if actions.dim() == 2 else 0
    dense = dict(alpha=alpha, beta=beta, actions=actions, log_prob_old=log_prob_old)
    for name, t in dict(dense, rewards=rewards, values_be=values_be).items():
        if t.dtype != torch.float32 or not t.is_contiguous() or (name in dense and tuple(t.shape) != (n, A)):
            raise ValueError(f'vtrace_segments: {name} must be a contiguous float32 tensor'
                             + (f' of shape ({n}, {A})' if name in dense else '') + f', got {tuple(t.shape)} {t.dtype}')
    lib = _lib.load()
    dev = rewards.device
    offsets = [0] * (S + 1)
    for s, k in enumerate(lengths):
        offsets[s + 1] = offsets[s] + k
    seg_off = torch.tensor(offsets, dtype=torch.int32, device=dev)
    returns = torch.empty(n, dtype=torch.float32, device=dev)
    returns_be = torch.empty((n, 2), dtype=torch.float32, device=dev)
    adv_raw = torch.empty(n, dtype=torch.float32, device=dev)
    adv = torch.empty(n, dtype=torch.float32, device=dev)
    rho = torch.empty(n, dtype=torch.float32, device=dev)
    scratch = torch.empty(int(lib.cdrl_vtrace_segments_scratch_doubles(n, S)), dtype=torch.float64, device=dev)
    _lib.check(lib.cdrl_vtrace_segments(_lib.ptr(rewards), _lib.ptr(values_be), _lib.ptr(alpha), _lib.ptr(beta), _lib.ptr(actions),
                                        _lib.ptr(log_prob_old), _lib.ptr(seg_off), S, n, A, float(gamma), float(lambda_), float(rho_bar),
                                        float(c_bar), float(scale), _lib.ptr(returns), _lib.ptr(returns_be), _lib.ptr(adv_raw),
                                        _lib.ptr(adv), _lib.ptr(rho), _lib.ptr(scratch),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'vtrace_segments')
    return returns, returns_be, adv_raw, adv, rho


ACT_SAMPLE, ACT_MODE = 0, 1


def act_stats_width(A: int) -> int:
    """CDRL_ACT_STATS(A) (include/cdrl.h): doubles per row of a cdrl_beta_act stats block."""
    return 3 * int(A) + 2


def beta_act(dist: torch.Tensor, value, mode: int, seed: int = 0, offset: int = 0, active=None, stats=None, action=None, log_prob=None):
    """Evaluation-time action for the rows of a predict block (cdrl_beta_act, one launch).  dist (rows, 4, A): alpha, beta, mean,
    std; value (rows, 4) or None; mode ACT_SAMPLE (the draw of cdrl_beta_sample_logp on (seed, offset), bit for bit) or ACT_MODE
    (the mode of the Beta); active: int32 (rows,) device tensor or None = every row; stats: float64 (rows, 3A + 2) running sums
    that the ACTIVE rows add to, or None.  -> (action, log_prob), (rows, A) each (written into `action` / `log_prob` when given)."""
    lib = _lib.load()
    rows, four, A = dist.shape
    if four != 4 or dist.dtype != torch.float32 or not dist.is_contiguous():
        raise ValueError(f'beta_act: dist must be a contiguous float32 (rows, 4, A) tensor, got {tuple(dist.shape)} {dist.dtype}')
    if value is not None and (tuple(value.shape) != (rows, 4) or value.dtype != torch.float32 or not value.is_contiguous()):
        raise ValueError(f'beta_act: value must be a contiguous float32 ({rows}, 4) tensor')
    if active is not None and (tuple(active.shape) != (rows,) or active.dtype != torch.int32 or not active.is_contiguous()):
        raise ValueError(f'beta_act: active must be a contiguous int32 ({rows},) tensor')
    if stats is not None and (tuple(stats.shape) != (rows, act_stats_width(A)) or stats.dtype != torch.float64
                              or not stats.is_contiguous()):
        raise ValueError(f'beta_act: stats must be a contiguous float64 ({rows}, {act_stats_width(A)}) tensor')
    if action is None:
        action = torch.empty((rows, A), dtype=torch.float32, device=dist.device)
    if log_prob is None:
        log_prob = torch.empty((rows, A), dtype=torch.float32, device=dist.device)
    _lib.check(lib.cdrl_beta_act(_lib.ptr(dist), _lib.ptr(value), rows, A, int(mode), int(seed), int(offset), _lib.ptr(active),
                                 _lib.ptr(action), _lib.ptr(log_prob), _lib.ptr(stats),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'cdrl_beta_act')
    return action, log_prob


# ---------------------------------------------------------------- occlusion saliency (csrc/explain.hip)
def _occ_check(name, t, shape=None, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda \
            or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f'{name} must be a contiguous {str(dtype)[6:]} device tensor' + (f' of shape {tuple(shape)}' if shape else '')
                         + f', got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}'
                         f' {getattr(t, "dtype", "")}')


def occlusion_baseline(image: torch.Tensor, mode: str = 'mean', out: torch.Tensor = None):
    """The neutral stack a cell is replaced by (cdrl_occlusion_baseline, one launch): image (T, H, W, 3) -> baseline of the same
    shape, 'zero' or 'mean' (each frame's channel mean, fixed-order double sums: the same input gives the same bytes)."""
    from .explain import BASELINES
    if mode not in BASELINES:
        raise ValueError(f'occlusion_baseline: mode {mode!r}: one of {BASELINES}')
    _occ_check('occlusion_baseline: image', image)
    if image.dim() != 4 or image.shape[3] != 3:
        raise ValueError(f'occlusion_baseline: image must be (T, H, W, 3), got {tuple(image.shape)}')
    if out is None:
        out = torch.empty_like(image)
    _occ_check('occlusion_baseline: out', out, image.shape)
    T, H, W, _ = image.shape
    _lib.check(_lib.load().cdrl_occlusion_baseline(_lib.ptr(image), _lib.ptr(out), T, H, W, BASELINES.index(mode),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'cdrl_occlusion_baseline')
    return out


def occlusion_rows(image, baseline, road, vehicle, navigation, grid, per_frame: bool, modalities: bool, first: int, out: dict):
    """Rows [first, first + count) of the N occluded variants of one observation (cdrl_occlusion_rows, one launch) into the chunk
    `out`: dict(state_image (count, T, H, W, 3), state_road (count, T, Dr), state_vehicle, state_navigation), what
    LearnerEngine.predict takes.  image, baseline (T, H, W, 3); road / vehicle / navigation (T, D*).  A row index >= N is a copy of
    row 0: every chunk is written in full.  -> out."""
    _occ_check('occlusion_rows: image', image)
    if image.dim() != 4 or image.shape[3] != 3:
        raise ValueError(f'occlusion_rows: image must be (T, H, W, 3), got {tuple(image.shape)}')
    T, H, W, _ = (int(x) for x in image.shape)
    _occ_check('occlusion_rows: baseline', baseline, (T, H, W, 3))
    gh, gw = (int(g) for g in grid)
    if not (1 <= gh <= H and 1 <= gw <= W):
        raise ValueError(f'occlusion_rows: grid ({gh}, {gw}) outside 1..{H} x 1..{W}')
    vectors = dict(road=road, vehicle=vehicle, navigation=navigation)
    for name, t in vectors.items():
        _occ_check(f'occlusion_rows: {name}', t)
        if t.dim() != 2 or t.shape[0] != T:
            raise ValueError(f'occlusion_rows: {name} must be ({T}, D), got {tuple(t.shape)}')
    try:
        chunk = [out['state_image'], out['state_road'], out['state_vehicle'], out['state_navigation']]
    except (KeyError, TypeError):
        raise ValueError('occlusion_rows: out must hold state_image, state_road, state_vehicle and state_navigation') from None
    count = int(chunk[0].shape[0]) if isinstance(chunk[0], torch.Tensor) and chunk[0].dim() == 5 else 0
    if count < 1 or int(first) < 0:
        raise ValueError(f'occlusion_rows: first = {first} and a chunk of {count} rows: need first >= 0 and at least one row')
    _occ_check('occlusion_rows: out state_image', chunk[0], (count, T, H, W, 3))
    for t, (name, v) in zip(chunk[1:], vectors.items()):
        _occ_check(f'occlusion_rows: out state_{name}', t, (count, T, int(v.shape[1])))
    _lib.check(_lib.load().cdrl_occlusion_rows(_lib.ptr(image), _lib.ptr(baseline), _lib.ptr(road), _lib.ptr(vehicle), _lib.ptr(navigation),
                                               T, H, W, int(road.shape[1]), int(vehicle.shape[1]), int(navigation.shape[1]), gh, gw,
                                               int(bool(per_frame)), int(bool(modalities)), int(first), count, *(_lib.ptr(t) for t in chunk),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'cdrl_occlusion_rows')
    return out


def occlusion_scores(alpha: torch.Tensor, beta: torch.Tensor, value: torch.Tensor, out: torch.Tensor = None):
    """Rows 1 .. N-1 against row 0 (cdrl_occlusion_scores, one launch, double arithmetic): alpha, beta (N, A), value (N, 2) as
    (base, exponent) -> float64 (N - 1, 2 + A): KL(Beta(row 0) || Beta(row g)) summed over the actions, the value difference
    base_g * 10^exp_g - base_0 * 10^exp_0, and per action the signed shift of the Beta mean."""
    _occ_check('occlusion_scores: alpha', alpha)
    if alpha.dim() != 2 or alpha.shape[0] < 2 or not 1 <= alpha.shape[1] <= 8:
        raise ValueError(f'occlusion_scores: alpha must be (N >= 2, 1 <= A <= 8), got {tuple(alpha.shape)}')
    N, A = (int(x) for x in alpha.shape)
    _occ_check('occlusion_scores: beta', beta, (N, A))
    _occ_check('occlusion_scores: value', value, (N, 2))
    if out is None:
        out = torch.empty((N - 1, 2 + A), dtype=torch.float64, device=alpha.device)
    _occ_check('occlusion_scores: out', out, (N - 1, 2 + A), torch.float64)
    _lib.check(_lib.load().cdrl_occlusion_scores(_lib.ptr(alpha), _lib.ptr(beta), _lib.ptr(value), N, A, _lib.ptr(out),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'cdrl_occlusion_scores')
    return out


def occlusion_maps(scores: torch.Tensor, frames: int, grid, size, upsample: str = 'nearest', normalize: bool = True):
    """Cell scores -> maps (cdrl_occlusion_maps, one launch): scores float64 (rows >= F*gh*gw, K), of which the first F*gh*gw rows
    are the cells in row order -> float32 (K, F, H, W).  'nearest': a pixel takes the score of its cell (the attribution itself);
    'bilinear': the gh x gw grid resized with the half-pixel rule of the contrastive views (display only).  normalize: each column
    divided by its largest |score| over all its cells; an all-zero column gives zeros."""
    from .explain import UPSAMPLES
    if upsample not in UPSAMPLES:
        raise ValueError(f'occlusion_maps: upsample {upsample!r}: one of {UPSAMPLES}')
    F, (gh, gw), (H, W) = int(frames), (int(g) for g in grid), (int(s) for s in size)
    if F < 1 or not (1 <= gh <= H and 1 <= gw <= W):
        raise ValueError(f'occlusion_maps: {F} frames, grid ({gh}, {gw}) outside 1..{H} x 1..{W}')
    _occ_check('occlusion_maps: scores', scores, None, torch.float64)
    if scores.dim() != 2 or scores.shape[0] < F * gh * gw or not 1 <= scores.shape[1] <= 10:
        raise ValueError(f'occlusion_maps: scores must be (rows >= {F * gh * gw}, 1 <= K <= 10), got {tuple(scores.shape)}')
    K = int(scores.shape[1])
    maps = torch.empty((K, F, H, W), dtype=torch.float32, device=scores.device)
    _lib.check(_lib.load().cdrl_occlusion_maps(_lib.ptr(scores), K, F, gh, gw, H, W, UPSAMPLES.index(upsample), int(bool(normalize)),
                                               _lib.ptr(maps), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               'cdrl_occlusion_maps')
    return maps


# ---------------------------------------------------------------- scoring on held-out rows (csrc/score.hip)
SCORE_BINS = 10
# the score block of cdrl_beta_score (include/cdrl.h, csrc/score_block.h): slot of every head entry, slot of every entry inside an
# action's group, the size of both; all doubles
SCORE_LAYOUT = dict(
    head=dict(rows=0, rows_returns=1, rows_aux=2, nonfinite=3, pit_unconverged=4, value_error=8, value_error2=9, returns=10,
              returns2=11, speed_error2=12, similarity_error2=13),
    head_size=16,
    action=dict(count=0, log_prob=1, mode_error=2, error=3, error2=4, variance=5, entropy=6, cover_50=7, cover_90=8, histogram=9),
    action_size=9 + SCORE_BINS)


def score_block_size(A: int) -> int:
    """CDRL_SCORE_BLOCK(A) (include/cdrl.h): doubles of a score block."""
    return SCORE_LAYOUT['head_size'] + SCORE_LAYOUT['action_size'] * int(A)


def score_block(A: int, device) -> torch.Tensor:
    """A zeroed score block for `A` actions: what beta_score adds to and read_score_block reads."""
    if not 1 <= int(A) <= 8:
        raise ValueError(f'score_block: A = {A} actions outside 1..8')
    return torch.zeros(score_block_size(A), dtype=torch.float64, device=device)


def beta_score(dist: torch.Tensor, value: torch.Tensor, u: torch.Tensor, returns: torch.Tensor = None, speed: torch.Tensor = None,
               similarity: torch.Tensor = None, count: int = None, block: torch.Tensor = None, pit: torch.Tensor = None):
    """The head outputs of one inference chunk against recorded rows (cdrl_beta_score, one launch, double arithmetic): dist
    (rows, 4, A) and value (rows, 4) as LearnerEngine.predict leaves them, u (count, A) expert actions in the unit interval, returns
    (count, 2) as (base, exponent) or None, speed / similarity (count,) -- both or neither.  Only the first `count` <= rows rows are
    scored (default: the rows of u).  block: a score_block(A) the sums are ADDED to (None: a fresh one); pit: float64 (count, A) that
    takes every element's Beta CDF at the expert action, or None.  -> block."""
    _occ_check('beta_score: dist', dist)
    if dist.dim() != 3 or dist.shape[1] != 4 or not 1 <= dist.shape[2] <= 8:
        raise ValueError(f'beta_score: dist must be (rows, 4, 1 <= A <= 8), got {tuple(dist.shape)}')
    rows, A = int(dist.shape[0]), int(dist.shape[2])
    _occ_check('beta_score: value', value, (rows, 4))
    _occ_check('beta_score: u', u)
    count = int(u.shape[0]) if count is None else int(count)
    if not 1 <= count <= rows:
        raise ValueError(f'beta_score: count = {count} outside 1..{rows} (the rows of dist)')
    _occ_check('beta_score: u', u, (count, A))
    if (speed is None) != (similarity is None):
        raise ValueError('beta_score: speed and similarity go together: both or neither')
    for name, t, shape in (('returns', returns, (count, 2)), ('speed', speed, (count,)), ('similarity', similarity, (count,))):
        if t is not None:
            _occ_check(f'beta_score: {name}', t, shape)
    if block is None:
        block = score_block(A, dist.device)
    _occ_check('beta_score: block', block, (score_block_size(A),), torch.float64)
    if pit is not None:
        _occ_check('beta_score: pit', pit, (count, A), torch.float64)
    for name, t in (('value', value), ('u', u), ('returns', returns), ('speed', speed), ('similarity', similarity), ('block', block),
                    ('pit', pit)):
        if t is not None and t.device != dist.device:
            raise ValueError(f'beta_score: {name} is on {t.device}, dist on {dist.device}')
    _lib.check(_lib.load().cdrl_beta_score(_lib.ptr(dist), _lib.ptr(value), _lib.ptr(u), _lib.ptr(returns), _lib.ptr(speed),
                                           _lib.ptr(similarity), rows, count, A, _lib.ptr(block), _lib.ptr(pit),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'cdrl_beta_score')
    return block


def _score_figures(host: np.ndarray, A: int) -> dict:
    """The derived figures of one score block on the host (numpy float64 of score_block_size(A) entries)."""
    head, act = SCORE_LAYOUT['head'], SCORE_LAYOUT['action']
    groups = host[SCORE_LAYOUT['head_size']:].reshape(A, SCORE_LAYOUT['action_size'])
    div = lambda s, n: float(s) / float(n) if n > 0 else float('nan')
    root = lambda s, n: float(np.sqrt(max(float(s), 0.0) / float(n))) if n > 0 else float('nan')
    n = groups[:, act['count']]
    total = float(n.sum())
    out = dict(rows=int(host[head['rows']]), nonfinite=int(host[head['nonfinite']]), pit_unconverged=int(host[head['pit_unconverged']]))
    for name, slot in (('log_prob', 'log_prob'), ('mode_error', 'mode_error'), ('bias', 'error'), ('entropy', 'entropy')):
        out[name] = div(groups[:, act[slot]].sum(), total)
        out[name + '_per_action'] = [div(groups[a, act[slot]], n[a]) for a in range(A)]
    for name, slot in (('rmse', 'error2'), ('predicted_std', 'variance')):
        out[name] = root(groups[:, act[slot]].sum(), total)
        out[name + '_per_action'] = [root(groups[a, act[slot]], n[a]) for a in range(A)]
    hist = groups[:, act['histogram']:act['histogram'] + SCORE_BINS]
    out['pit_histogram'] = np.rint(hist).astype(np.int64)
    with_pit = hist.sum(axis=1)                 # elements whose PIT was formed
    out['coverage_50'] = [div(groups[a, act['cover_50']], with_pit[a]) for a in range(A)]
    out['coverage_90'] = [div(groups[a, act['cover_90']], with_pit[a]) for a in range(A)]
    nr, na = host[head['rows_returns']], host[head['rows_aux']]
    out.update(value_bias=None, value_rmse=None, explained_variance=None, speed_rmse=None, similarity_rmse=None)
    if nr > 0:
        e, e2, r, r2 = (float(host[head[k]]) for k in ('value_error', 'value_error2', 'returns', 'returns2'))
        var_e, var_r = e2 / nr - (e / nr) ** 2, r2 / nr - (r / nr) ** 2
        out.update(value_bias=e / nr, value_rmse=root(e2, nr), explained_variance=1.0 - var_e / var_r if var_r > 0.0 else float('nan'))
    if na > 0:
        out.update(speed_rmse=root(host[head['speed_error2']], na), similarity_rmse=root(host[head['similarity_error2']], na))
    out['block'] = host.copy()
    return out


def read_score_block(block: torch.Tensor, A: int) -> dict:
    """ONE device-to-host copy of a score block (or of a (K, size) stack of blocks -> a list of K dicts) and the figures derived
    from it on the host: rows; log_prob, mode_error, bias, rmse, predicted_std (the root of the mean predicted variance) and
    entropy, each as the mean over all scored elements and `_per_action`; pit_histogram (A, SCORE_BINS) ints; coverage_50 /
    coverage_90 per action (the share of PIT values inside the central 50 % / 90 %; 0.5 / 0.9 for a calibrated policy);
    value_bias, value_rmse, explained_variance (None without returns); speed_rmse, similarity_rmse (None without auxiliary
    targets); nonfinite, pit_unconverged; block, the sums themselves (numpy float64, SCORE_LAYOUT).  A mean over nothing is NaN."""
    A = int(A)
    if block.dtype != torch.float64 or block.dim() not in (1, 2) or block.shape[-1] != score_block_size(A):
        raise ValueError(f'read_score_block: a float64 block of {score_block_size(A)} entries for A = {A}, got {tuple(block.shape)} '
                         f'{block.dtype}')
    host = block.cpu().numpy()
    return _score_figures(host, A) if host.ndim == 1 else [_score_figures(h, A) for h in host]

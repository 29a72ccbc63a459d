"""CARLANetwork on top of the native learner engine.

Keeps the reference's surface (core/networks.py): module-level `dynamics_layers`, `control_branch`,
`PolicyNetwork`, and `CARLANetwork` with predict / predict_last_value / dynamics_predict(_train) /
update_old_policy / save_weights / load_weights / reset / summary, while the four Keras models
(dynamics, policy, old_policy, value) live in flat device arenas owned by a LearnerEngine.
"""
import os
from typing import Dict

import numpy as np
import torch

from .. import _lib
from ..engine import LearnerEngine, beta_act, ACT_SAMPLE, ACT_MODE, occlusion_rows, occlusion_scores, occlusion_maps, \
    beta_score, score_block
from ..explain import occlusion_row_count, occlusion_frames
from ..init import init_engine_parameters
from ..rl.networks import Network
from ..rl import utils
from . import architectures as nn


def relu6(x):
    return torch.clamp(x, 0.0, 6.0)


def dynamics_layers(inputs: dict, time_horizon: int, **kwargs) -> dict:
    """Shared-network description: ShuffleNet-v2 tower + road / vehicle / navigation feature nets, one
    GRU per modality, concat -> BatchNorm -> Dense(units).  inputs: {name: per-slice shape}."""
    rnn = kwargs.get('rnn')
    if rnn is None:
        raise ValueError("dynamics_layers needs rnn=dict(image=, road=, vehicle=, navigation=)")
    small = {rnn['road'], rnn['vehicle'], rnn['navigation']}
    if len(small) != 1:
        raise NotImplementedError('road / vehicle / navigation GRUs must share one width')
    feats = {k: nn.feature_net(inputs[f'state_{k}'], time_horizon, **kwargs.get(k, {})) for k in ('road', 'vehicle', 'navigation')}
    if len({f['units'] for f in feats.values()}) != 1:
        raise NotImplementedError('feature nets must share one width')
    return dict(kind='dynamics', time_horizon=time_horizon,
                image=nn.shufflenet_v2(inputs['state_image'], time_horizon, **kwargs.get('shufflenet', {})),
                features=feats, rnn=dict(rnn), units=int(kwargs.get('dynamics', {}).get('units', 32)))


def control_branch(inputs: dict, units: int, num_layers: int, activation=utils.swish6) -> dict:
    """[BatchNorm -> Dense(units, swish6)] x num_layers on the dynamics output."""
    if num_layers != 2 or getattr(activation, '__name__', activation) != 'swish6':
        raise NotImplementedError('control branches are built as 2 x [BN -> Dense(units, swish6)] (reference default)')
    return dict(kind='control_branch', units=int(units))


class PolicyNetwork:
    """Policy head description: control branch + Beta(alpha, beta) + auxiliary speed / similarity."""

    def __init__(self, agent, inputs: dict = None, name='PolicyNetwork', **kwargs):
        self.agent = agent
        self.name = name
        self.spec = dict(branch=control_branch(inputs or {}, **kwargs), num_actions=agent.num_actions)


class CARLANetwork(Network):
    def __init__(self, agent, control_policy: dict, control_value: dict, dynamics: dict, update_dynamics=True, compute='f32'):
        """compute: 'f32' (the reference's arithmetic) or 'bf16' -- bf16 MFMA operands in the tower's 1x1 convolutions
        (include/cdrl.h CDRL_COMPUTE_BF16_OPERANDS, BASELINE.json configs[2]; see DESIGN.md section 7 for what it costs numerically).
        update_dynamics=False: frozen trunk -- the learner engines train the policy / value heads only (cdrl_config.freeze_trunk);
        CARLAgent passes its own update_dynamics.  (The reference's keyword defaults to False but is never read there; here it
        drives the engine, so the default is the agent's.)
        The agent's optimizer name and polyak coefficient (PPOAgent(optimizer=..., polyak=...)) configure every engine built here
        (cdrl_config.optimizer / polyak), and so do its clip_mode and skip_nonfinite (PPOAgent(clip_mode=..., skip_nonfinite=...):
        the gradient gate, cdrl_config.clip_mode / skip_nonfinite).  When the agent logs (log_mode is not None) the learner engines keep a train-stats ring
        of `agent.train_stats_rows` rows (cdrl_config.train_stats): `train_stats()` fetches one update()'s diagnostics."""
        super().__init__(agent)
        env = agent.env
        T = env.time_horizon
        spec = agent.state_spec
        for key in ('state_image', 'state_road', 'state_vehicle', 'state_navigation'):
            if key not in spec:
                raise ValueError(f'observation space lacks {key[6:]!r}')
        self.dynamics_spec = dynamics_layers({k: spec[k] for k in spec}, time_horizon=T, **dynamics)
        control_value = dict(control_value)
        self.exp_scale = float(control_value.pop('exponent_scale', 6.0))
        if control_value.pop('components', 1) != 1:
            raise NotImplementedError('value head with components != 1')
        p_branch = control_branch({}, **control_policy)
        v_branch = control_branch({}, **control_value)
        if p_branch['units'] != v_branch['units']:
            raise NotImplementedError('policy and value control branches must share one width')
        img = self.dynamics_spec['image']
        self.cfg = dict(T=T, H=img['image'][0], W=img['image'][1], road=spec['state_road'][0],
                        vehicle=spec['state_vehicle'][0], navigation=spec['state_navigation'][0], A=agent.num_actions,
                        stem=img['stem'], stage_c=img['stage_c'], stage_n=img['stage_n'], last=img['last'],
                        feat=self.dynamics_spec['features']['road']['units'], rnn_image=self.dynamics_spec['rnn']['image'],
                        rnn_small=self.dynamics_spec['rnn']['road'], dyn=self.dynamics_spec['units'],
                        head=p_branch['units'], exp_scale=self.exp_scale, compute=compute, freeze_trunk=not update_dynamics,
                        optimizer=getattr(agent, 'optimizer_name', 'adam'), polyak=float(getattr(agent, 'polyak_coeff', 1.0)),
                        clip_mode=getattr(agent, 'clip_mode', 'tensor'), skip_nonfinite=bool(getattr(agent, 'skip_nonfinite', False)))
        if getattr(agent, 'trust', False):      # PPOAgent(target_kl=... / kl_penalty=...): the trust-region guard (cdrl_config.trust)
            self.cfg['trust'] = True
        self.device = agent.device
        # update diagnostics: the learner engines only (main + ragged share one ring); off when the agent does not log
        self.train_stats_rows = int(getattr(agent, 'train_stats_rows', 0)) if agent.statistics.mode is not None else 0
        self.engine = LearnerEngine(agent.batch_size, device=self.device, train_stats=self.train_stats_rows, **self.cfg)   # learner minibatches
        self._rollouts = {}                # number of environments E -> inference engine over the same arenas
        self.rollout = self.rollout_for(1)                                                       # B = 1 inference
        self._explain_chunks = {}          # chunk rows -> the input buffers explain_rows fills (built on first use, kept)
        self._ragged = {}                  # minibatch rows -> engine for a ragged last minibatch (shares arenas + optimizer)
        init_engine_parameters(self.engine, seed=agent.seed if agent.seed is not None else 0)
        self.last_value = torch.zeros((1, 2), dtype=torch.float32, device=self.device)   # (base, exp) at terminal states
        self.action_index = 0              # Philox offset of the rollout sampler: one stream per predict() call
        self.sample_seed = (agent.seed if agent.seed is not None else 0) + 0x5eed
        self.sample_rank, self.sample_stride = 0, 1      # data-parallel agents: rank-disjoint Philox offsets (CARLAgent._init_data_parallel)
        self.update_dynamics = update_dynamics

    def rollout_for(self, envs: int) -> LearnerEngine:
        """Inference engine for `envs` environments stepped together (one batched forward + one sampling launch per step)."""
        if envs not in self._rollouts:
            self._rollouts[envs] = LearnerEngine(envs, device=self.device, share_with=self.engine, **self.cfg)
        return self._rollouts[envs]

    def engine_for(self, rows: int) -> LearnerEngine:
        """The learner engine for a minibatch of `rows` samples: the main engine, or -- for the ragged last minibatch the
        reference's `batch(drop_remainder=False)` pipeline yields (rl/utils.py:388) -- an engine planned for that size over the
        SAME parameter / gradient / Adam arenas and optimizer counters (built on first use, kept)."""
        if rows == self.engine.cfg.B:
            return self.engine
        if rows not in self._ragged:
            self._ragged[rows] = LearnerEngine(rows, device=self.device, share_with=self.engine, train_stats=self.train_stats_rows,
                                               **self.cfg)
        return self._ragged[rows]

    def train_stats(self, fetch=True):
        """The learner engines' update diagnostics since the last call (LearnerEngine.train_stats), or None when the ring is off.
        fetch=False empties the ring without the device-to-host copy (data-parallel ranks that do not write summaries)."""
        if self.train_stats_rows <= 0:
            return None
        if not fetch:
            self.engine.train_stats_reset()
            return None
        return self.engine.train_stats()

    # -- hyper-parameters -----------------------------------------------------------------------
    def set_hparams(self, **kw):
        self.engine.set_hparams(**kw)

    # -- inference (rollout) ------------------------------------------------------------------------
    def _pick(self, inputs: dict) -> Dict[str, torch.Tensor]:
        return {k: inputs[k].to(self.device, torch.float32).contiguous()
                for k in ('state_image', 'state_road', 'state_vehicle', 'state_navigation')}

    def predict(self, inputs: dict, deterministic=False):
        """-> (action sample, mean, std, log_prob of the clipped sample, value (base, exp)); uses old_policy and BatchNorm
        moving statistics, like the reference's rollout forward (core/networks.py:181-193).  The leading axis of the inputs
        is the number of environments E stepped together (1 in the reference's loop); the Beta sample and its log-density
        come from one cdrl_beta_sample_logp launch on the (alpha, beta) the forward left on the device -- no host round trip.
        Returned tensors are fresh (not views of the engine's persistent output buffers).
        deterministic=True: the action is the mode of the Beta, (alpha - 1) / (alpha + beta - 2), and log_prob its log-density
        (cdrl_beta_act, mode 1); nothing is drawn, so `action_index` does not advance and the sampler's stream is untouched."""
        st = self._pick(inputs)
        E = st['state_image'].shape[0]
        eng = self.rollout_for(E)
        out = eng.predict(st)
        A = out['alpha'].shape[1]
        action = torch.empty((E, A), dtype=torch.float32, device=self.device)
        log_prob = torch.empty((E, A), dtype=torch.float32, device=self.device)
        if deterministic:
            beta_act(eng._pred_out[0], None, ACT_MODE, action=action, log_prob=log_prob)
            return action, out['mean'].clone(), out['std'].clone(), log_prob, out['value'].clone()
        self.action_index += 1
        alpha, beta = out['alpha'], out['beta']              # views of the persistent (E, 4, A) block: row stride 4A
        _lib.check(self.engine.lib.cdrl_beta_sample_logp(_lib.ptr(alpha), _lib.ptr(beta), E, A, 4 * A, int(self.sample_seed),
                                                         int(self.action_index * self.sample_stride + self.sample_rank), _lib.ptr(action), _lib.ptr(log_prob),
                                                         self.engine._stream()), 'cdrl_beta_sample_logp')
        return action, out['mean'].clone(), out['std'].clone(), log_prob, out['value'].clone()

    def _row_chunks(self, st: dict, chunk: int):
        """The N rows of picked inputs, `chunk` at a time -> (start, rows that count, chunk of inputs): a full chunk is a view, the
        last one is filled up by repeating the last row instead of planning an engine for its size."""
        n = st['state_image'].shape[0]
        for start in range(0, n, chunk):
            m = min(chunk, n - start)
            if m == chunk:
                yield start, m, {k: v[start:start + chunk] for k, v in st.items()}
            else:
                index = torch.arange(start, start + chunk, device=self.device).clamp_(max=n - 1)
                yield start, m, {k: v.index_select(0, index) for k, v in st.items()}

    def distribution_and_value(self, inputs: dict, chunk: int):
        """The acting network on N stored rows -> (alpha (N, A), beta (N, A), value (N, 2)), fresh tensors: inference forwards as
        predict() runs them (old_policy, moving statistics) through ONE engine, rollout_for(chunk), `chunk` rows at a time; the last
        chunk is filled up by repeating the last row instead of planning an engine for its size.  Nothing is sampled: `action_index`
        stays where it is.  What update() refreshes kept rollouts with (PPOAgent.refresh_replay)."""
        st = self._pick(inputs)
        n = st['state_image'].shape[0]
        eng = self.rollout_for(chunk)
        A = self.cfg['A']
        alpha = torch.empty((n, A), dtype=torch.float32, device=self.device)
        beta = torch.empty((n, A), dtype=torch.float32, device=self.device)
        value = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        for start, m, rows in self._row_chunks(st, chunk):
            out = eng.predict(rows)
            alpha[start:start + m].copy_(out['alpha'][:m])
            beta[start:start + m].copy_(out['beta'][:m])
            value[start:start + m].copy_(out['value'][:m])
        return alpha, beta, value

    def score_rows(self, inputs: dict, u, returns=None, speed=None, similarity=None, chunk: int = 32, block=None):
        """The acting network scored on N recorded rows: inference forwards exactly as distribution_and_value runs
        them (rollout_for(chunk), old_policy, moving statistics, the last chunk filled up by repeating the last row), and per chunk
        ONE cdrl_beta_score launch that reads the engine's persistent predict outputs where they lie and adds the chunk's sums to
        `block` (engine.score_block; None: a fresh one) -- no per-chunk copy of an output, no host read.  u (N, A) expert actions in
        the unit interval, returns (N, 2) as (base, exponent) or None, speed / similarity (N,) or None: contiguous float32 device
        tensors, of which every chunk is a view.  Nothing is sampled: `action_index`, the memory and the logs stay as they are.
        -> block."""
        st = self._pick(inputs)
        chunk = int(chunk)
        eng = self.rollout_for(chunk)
        if block is None:
            block = score_block(self.cfg['A'], self.device)
        part = lambda t, start, m: None if t is None else t[start:start + m]
        for start, m, rows in self._row_chunks(st, chunk):
            eng.predict(rows)
            beta_score(eng._pred_out[0], eng._pred_out[1], u[start:start + m], part(returns, start, m), part(speed, start, m),
                       part(similarity, start, m), count=m, block=block)
        return block

    def explain_rows(self, inputs: dict, grid, baseline, per_frame=False, modalities=True, upsample='nearest', normalize=True, chunk=32):
        """Occlusion saliency of ONE observation: inputs (T, ...) per key, baseline (T, H, W, 3) on the device.  The
        N = occlusion_row_count(...) variants -- the observation, one row per cell with the cell taken from the baseline, and with
        `modalities` the whole image / road / vehicle / navigation occluded -- go through rollout_for(chunk) as predict() runs it
        (old_policy, moving statistics), `chunk` rows at a time: per chunk ONE cdrl_occlusion_rows launch into buffers the engine
        reads directly, one inference forward, three small copies; then one cdrl_occlusion_scores and one cdrl_occlusion_maps
        launch.  ceil(N / chunk) forwards, no host read.  Nothing is sampled, logged or stored; `action_index` stays where it is.
        Kept between calls: the chunk buffers (chunk rows of inputs) and the engine for `chunk` rows.
        -> dict(alpha (N, A), beta (N, A), value (N, 2), scores float64 (N - 1, 2 + A), maps float32 (2 + A, F, H, W))."""
        st = self._pick(inputs)
        image = st['state_image']
        T, H, W = (int(x) for x in image.shape[:3])
        gh, gw = (int(g) for g in grid)
        chunk = int(chunk)
        N = occlusion_row_count(T, gh, gw, per_frame, modalities)
        eng = self.rollout_for(chunk)
        rows = self._explain_chunks.get(chunk)
        if rows is None:
            rows = self._explain_chunks[chunk] = {k: torch.empty((chunk,) + tuple(v.shape), dtype=torch.float32, device=self.device)
                                                  for k, v in st.items()}
        A = self.cfg['A']
        alpha = torch.empty((N, A), dtype=torch.float32, device=self.device)
        beta = torch.empty((N, A), dtype=torch.float32, device=self.device)
        value = torch.empty((N, 2), dtype=torch.float32, device=self.device)
        for first in range(0, N, chunk):
            occlusion_rows(image, baseline, st['state_road'], st['state_vehicle'], st['state_navigation'], (gh, gw), per_frame,
                           modalities, first, rows)
            out = eng.predict(rows)
            m = min(chunk, N - first)
            alpha[first:first + m].copy_(out['alpha'][:m])
            beta[first:first + m].copy_(out['beta'][:m])
            value[first:first + m].copy_(out['value'][:m])
        scores = occlusion_scores(alpha, beta, value)
        maps = occlusion_maps(scores, occlusion_frames(T, per_frame), (gh, gw), (H, W), upsample, normalize)
        return dict(alpha=alpha, beta=beta, value=value, scores=scores, maps=maps)

    def evaluate_step(self, inputs: dict, deterministic, active=None, stats=None):
        """One evaluation step for E environments -> (action, log_prob): one inference forward plus ONE cdrl_beta_act launch that
        also adds the step's action / mean / std / value to the device block `stats` (float64 (E, 3A + 2), engine.beta_act) for
        the rows whose `active` entry (int32 (E,), None = all) is set -- mean, std and value are never copied.  In sample mode
        the draw is the one predict() would make: `action_index` advances and selects the Philox offset in the same way."""
        st = self._pick(inputs)
        E = st['state_image'].shape[0]
        eng = self.rollout_for(E)
        eng.predict(st)
        dist, value = eng._pred_out[0], eng._pred_out[1]
        if deterministic:
            return beta_act(dist, value, ACT_MODE, active=active, stats=stats)
        self.action_index += 1
        return beta_act(dist, value, ACT_SAMPLE, seed=int(self.sample_seed),
                        offset=int(self.action_index * self.sample_stride + self.sample_rank), active=active, stats=stats)

    def dynamics_predict(self, inputs: dict):
        st = self._pick(inputs)
        return self.rollout_for(st['state_image'].shape[0]).predict(st)['dynamics'].clone()

    def dynamics_predict_train(self, inputs: dict):
        return self.engine.trunk_forward_train(self._pick(inputs))

    def data_for_dynamics(self, inputs):
        return inputs        # the 'action' input is a pass-through that no layer consumes

    def predict_last_value(self, state, is_terminal: bool, **kwargs):
        if is_terminal:
            return self.last_value
        st = self._pick(state)
        return self.rollout_for(st['state_image'].shape[0]).predict(st)['value'].clone()

    def value_predict(self, inputs):
        st = self._pick(inputs)
        return self.rollout_for(st['state_image'].shape[0]).predict(st)['value'].clone()

    # -- weights ----------------------------------------------------------------------------------
    def reset(self):
        super().reset()

    def update_old_policy(self, weights=None):
        if weights:
            self.engine.load_params('old_policy', weights)
        else:
            self.engine.update_old_policy()

    def get_weights(self) -> dict:
        return {m: self.engine.export_params(m) for m in ('policy', 'value', 'trunk')}

    def set_weights(self, weights: dict):
        for m, w in weights.items():
            self.engine.load_params(m, w)

    def trainable_variables(self):
        """Trainable tensors per model; the trunk's only when it is updated (frozen: the heads alone)."""
        models = ('policy', 'value', 'trunk') if self.update_dynamics else ('policy', 'value')
        return {m: {k: v for k, v in self.engine.param_views(m).items() if self.engine.tables[m].by_name[k]['trainable']}
                for m in models}

    def _paths(self):
        return dict(policy=self.agent.weights_path['policy'] + '.npz', value=self.agent.weights_path['value'] + '.npz',
                    trunk=self.agent.dynamics_path + '.npz')

    def save_weights(self):
        """policy_net / value_net / dynamics_model as TensorFlow checkpoint-V2 files (`<name>.index` + two data shards), the
        layout Keras' `save_weights` leaves in the reference (core/networks.py:297-300), keyed `layer_with_weights-N/<var>` in
        Keras' layer order; optimizer state is not saved, as in the reference."""
        from .. import tf_checkpoint
        for model, path in self._paths().items():
            tf_checkpoint.save_from_engine(self.engine, model, path[:-4])

    def load_weights(self, full=True):
        """Loads TensorFlow checkpoint-V2 files (`<name>.index`: this package's own or the reference's shipped ones), or the
        `.npz` containers earlier versions of this package wrote (tf_checkpoint.py; tensors whose data shard is absent are skipped
        with a warning, e.g. the trunk shards the reference repository does not ship)."""
        from .. import tf_checkpoint
        paths = self._paths()
        for model in (('policy', 'value', 'trunk') if full else ('trunk',)):
            prefix = paths[model][:-4]
            if os.path.exists(prefix + '.index'):
                loaded = tf_checkpoint.load_into_engine(self.engine, model, prefix, strict=False)
                n = len(self.engine.tables[model].entries)
                if len(loaded) < n:
                    print(f'[load_weights] {prefix}: {len(loaded)}/{n} tensors present in the TF checkpoint')
                continue
            with np.load(paths[model]) as f:
                self.engine.load_params(model, {k: f[k] for k in f.files})
        if full:
            self.engine.update_old_policy()

    def save_state(self, prefix: str, extra: dict = None):
        """The full learner state under the directory `prefix` (learner_state.py: `learner_state.index` + data shards, then
        `learner_state.json`): the engine's export_state() -- whole parameter arena with old_policy and the moving statistics, both
        slot arenas, the six optimizer scalars, manifest -- plus the rollout sampler's Philox seed and offset (`sample_seed`,
        `action_index`).  `extra`: JSON-able entries of the caller's that travel in the same JSON file (the agent's counters and
        generators).  One host read of the device scalars and three arena copies; nothing on the step path changes."""
        from .. import learner_state
        state = self.engine.export_state()
        opt = state['optimizer']
        arrays = dict(params=state['params'], adam_m=state['adam_m'], adam_v=state['adam_v'],
                      m_cache=np.asarray([opt['m_cache_policy'], opt['m_cache_value'], opt['m_cache_dynamics']], dtype=np.float32))
        meta = dict(extra or {})
        meta.update(manifest=state['manifest'], optimizer_steps=[opt['t_policy'], opt['t_value'], opt['t_dynamics']],
                    action_index=int(self.action_index), sample_seed=int(self.sample_seed))
        learner_state.save(prefix, arrays, meta)

    def load_state(self, prefix: str) -> dict:
        """Inverse of save_state; returns the JSON file's entries (the caller's `extra` among them).  Everything is read and
        validated before anything is written (LearnerEngine.import_state).  old_policy comes back as it was saved -- after an
        update() it is the policy BEFORE the last minibatch step, which is what the rollouts sample from -- so, unlike
        load_weights, this does not end in update_old_policy()."""
        from .. import learner_state
        arrays, meta = learner_state.load(prefix)
        for name in ('params', 'adam_m', 'adam_v', 'm_cache'):
            if name not in arrays:
                raise learner_state.LearnerStateError(f'{prefix}: array {name!r} is missing from the learner state')
        t, mc = meta['optimizer_steps'], arrays['m_cache'].reshape(-1)
        if len(t) != 3 or mc.shape[0] != 3:
            raise learner_state.LearnerStateError(f'{prefix}: three step counters and three m_caches expected')
        self.engine.import_state(dict(params=arrays['params'], adam_m=arrays['adam_m'], adam_v=arrays['adam_v'],
                                      manifest=meta['manifest'],
                                      optimizer=dict(t_policy=int(t[0]), t_value=int(t[1]), t_dynamics=int(t[2]),
                                                     m_cache_policy=float(mc[0]), m_cache_value=float(mc[1]),
                                                     m_cache_dynamics=float(mc[2]))))
        self.action_index = int(meta['action_index'])
        self.sample_seed = int(meta['sample_seed'])
        return meta

    def summary(self):
        for model, title in (('policy', 'Policy Network'), ('value', 'Value Network'), ('trunk', 'Dynamics Model')):
            table = self.engine.tables[model]
            total = sum(e['numel'] for e in table.entries)
            train = sum(e['numel'] for e in table.entries if e['trainable'])
            print(f'==== {title} ====')
            for e in table.entries:
                print(f"  {e['name']:<34} {str(e['shape']):<20} {e['numel']:>9}{'' if e['trainable'] else '  (non-trainable)'}")
            print(f'  Total params: {total:,}  trainable: {train:,}  non-trainable: {total - train:,}\n')

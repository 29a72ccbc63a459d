"""PPOAgent / PPOMemory: host-side control flow of the learner (what to run, in which order);
all arithmetic runs in libcdrl_hip.so through the network's LearnerEngine.

Surface and step order follow the reference rl/agents/ppo.py: constructor keywords (:26-32),
update() = all policy minibatches then all value minibatches (:190-226), learn() rollout loop
(:464-568), end_episode (:574-585), PPOMemory (:629-733)."""
import os
import time
from typing import Optional, Sequence, Union

import numpy as np
import torch

from .. import utils
from ..parameters import DynamicParameter
from ..replay import ReplayPeriod, RolloutReplay, TrajectoryTable
from ..demonstrations import DemonstrationStore, demo_split, draw_rows
from .agents import Agent
from ..._lib import CLIP_MODES, OPTIMIZERS
from ... import traces, train_stats


def demo_weight_checked(weight):
    """demo_weight as given: a number must be finite and not negative (a schedule is taken as it is)."""
    if isinstance(weight, (int, float)) and not isinstance(weight, bool) and not (np.isfinite(weight) and weight >= 0.0):
        raise ValueError(f'demo_weight={weight!r} must be a finite number >= 0, or a DynamicParameter / schedule')
    return weight


class PPOAgent(Agent):
    replay, _replay_active = None, ()       # class-level defaults: an agent that never ran __init__ reuses nothing
    trust, _trust_anchor, _trust_stats = False, None, None      # ... and has no trust-region guard
    demo_traces, _demo_active = None, False                     # ... and no demonstrations

    def __init__(self, *args, policy_lr=1e-3, gamma=0.99, lambda_=0.95, value_lr=3e-4, load=False,
                 optimization_steps=(1, 1), name='ppo-agent', optimizer='adam', clip_norm=(1.0, 1.0), clip_ratio=0.2,
                 seed_regularization=False, entropy_regularization=0.0, network: dict = None, update_frequency=1,
                 polyak=1.0, repeat_action=1, advantage_scale=2.0, train_stats_rows=256, clip_mode='tensor', skip_nonfinite=False,
                 joint_update=False, replay_rollouts=0, replay_rho_clip=1.0, replay_c_clip=1.0, target_kl=None, kl_penalty=0.0,
                 kl_stop_factor=1.5, demo_traces=None, demo_fraction=0.25, demo_weight=0.1, demo_rows=4096, demo_seed=None, **kwargs):
        """clip_mode: 'tensor' (default; utils.clip_gradients of the reference: tf.clip_by_norm per tensor of each head) or 'global'
        (tf.clip_by_global_norm of each optimizer's gradient list, the max_grad_norm of other PPO implementations; thresholds are
        those of clip_norm).  skip_nonfinite=True: a minibatch step whose gradients hold a NaN or an Inf leaves parameters and
        optimizer state untouched; update() logs how many were skipped (skipped_steps_policy / _value) and says so in one line.
        With either option update() reads the gate statistics once, after the minibatch loops (one small copy); in global mode it
        also logs the last gradients_global_norm_{policy,value,dynamics}.
        train_stats_rows: capacity, in minibatch steps, of the device ring the learner engines append their per-step diagnostics
        to when the agent logs (log_mode is not None); update() reads it once.  An update() with more policy + value steps than
        that keeps the newest rows and reports how many it lost.
        joint_update=True: update() runs ONE minibatch loop whose steps take the policy and the value loss together (agents that
        implement get_joint_gradients / apply_joint_gradients: CARLAgent); needs optimization_steps[0] == optimization_steps[1].
        replay_rollouts=K > 0 (not in the reference, not written to config.json): update() keeps the K most recent
        update-periods on the device (rl/replay.py) instead of discarding their rows, and trains on them again behind the fresh rows.
        Before the minibatches are formed the kept rows are re-evaluated with the acting network (inference forwards in chunks of
        batch_size) and their targets corrected for the policy lag by V-trace in ONE launch (utils.vtrace_segments) with the
        importance ratio clipped at replay_rho_clip (TD weight) and replay_c_clip (trace cut); fresh rows keep their GAE targets bit
        for bit.  Needs the stored-action policy loss (an agent with a re-sampled loss refuses) and one GPU.  The store is not saved
        by save_state(); clear_replay() empties it.  Nobody has measured what reuse does to driving quality.
        target_kl / kl_penalty / kl_stop_factor (not in the reference's constructor, not written to config.json): a
        trust-region guard of the policy steps, on when target_kl is given or kl_penalty > 0.  update() then evaluates the acting
        network once on all policy rows (the anchor), every policy minibatch pass measures the analytic Beta KL between the anchor
        and its policy on the device, and -- with target_kl -- once a pass finds it above kl_stop_factor * target_kl (1.5: Spinning
        Up's convention, not a measurement) the device leaves out every remaining policy apply of the update() and the remaining
        policy epochs are not run (one small read per epoch); the value loop runs as before.  kl_penalty = c > 0 adds c * KL to the
        policy objective.  Logged per update(): kl_divergence, kl_divergence_max, kl_stopped_steps, kl_stop_pass.  Needs the separate
        policy / value loops (joint_update=True: ValueError) and one process (an initialised process group: ValueError -- the ranks
        would decide differently); imitate() with a value weight runs joint passes, which such an agent's engines refuse.  Nobody has
        measured what the guard does to learning or driving quality.
        demo_traces / demo_fraction / demo_weight / demo_rows / demo_seed (not in the reference, not written to config.json;
        DESIGN.md 6.16): expert demonstrations inside the PPO update, on when demo_traces is a directory of trace files.  At the
        first update() the traces are loaded once, in sorted file order, into a device store of at most demo_rows rows (what does
        not fit is counted in one printed line).  Every policy minibatch then holds batch_size - D fresh rows followed by
        D = round(demo_fraction * batch_size) demonstration rows, drawn without replacement from the store by a generator of its
        own (demo_seed) at every minibatch step; one trunk pass trains the fresh rows by the PPO surrogate and the demonstration
        rows by the Beta log-likelihood of the expert's action with weight demo_weight -- a float or any DynamicParameter, read
        once per update() and ticked per episode; at 0 the update() runs without demonstrations.  The value loop sees fresh rows
        only.  Logged per update(): loss_demo, demo_log_prob, demo_mode_error, demo_rows_per_batch, demo_weight.  Refused with
        ValueError: joint_update=True (no joint form of the mixed pass), replay_rollouts > 0 (kept rows and demonstration rows
        would compete for the rows behind the fresh ones), target_kl / kl_penalty (the anchor sweep has no demonstration rows), an
        initialised process group (the ranks would draw different rows for one collective step), a demo_fraction with D outside
        1 .. batch_size - 1.  save_state() holds the generator and the schedule; the store is reloaded from the directory.  Nobody
        has measured what demonstrations do to learning or driving quality."""
        assert 0.0 < polyak <= 1.0
        self.joint_update = bool(joint_update)
        if self.joint_update and optimization_steps[0] != optimization_steps[1]:
            raise ValueError(f'joint_update=True runs one minibatch loop for both losses: optimization_steps must be equal, got '
                             f'{tuple(optimization_steps)}')
        assert repeat_action >= 1
        self.target_kl = None if target_kl is None else float(target_kl)
        self.kl_penalty, self.kl_stop_factor = float(kl_penalty), float(kl_stop_factor)
        if (self.target_kl is not None and not self.target_kl >= 0.0) or not self.kl_penalty >= 0.0 or not self.kl_stop_factor > 0.0:
            raise ValueError(f'target_kl={target_kl!r} and kl_penalty={kl_penalty!r} must not be negative and '
                             f'kl_stop_factor={kl_stop_factor!r} must be positive')
        self.trust = self.target_kl is not None or self.kl_penalty > 0.0        # reaches the learner engines through the network
        if self.trust and self.joint_update:
            raise ValueError('target_kl / kl_penalty need the separate policy and value loops: the trust-region latch gates the policy '
                             'apply only, and half of a joint apply has no gated form; create the agent with joint_update=False')
        if self.trust and torch.distributed.is_available() and torch.distributed.is_initialized():
            raise ValueError('target_kl / kl_penalty run in one process: every rank would measure the KL of its own shard and decide '
                             'on its own whether a collective step is taken; create the data-parallel agents without them')
        self._trust_anchor = None                   # (N, 2, A) alpha0 / beta0 of the policy rows of the running update()
        self.demo_traces = demo_traces
        if int(replay_rollouts) != replay_rollouts or replay_rollouts < 0:
            raise ValueError(f'replay_rollouts={replay_rollouts!r}: the number of finished update-periods to keep, an integer >= 0 '
                             f'(0 = no reuse)')
        if not float(replay_rho_clip) >= 0.0 or not float(replay_c_clip) >= 0.0:
            raise ValueError(f'replay_rho_clip={replay_rho_clip!r}, replay_c_clip={replay_c_clip!r}: V-trace clips the importance '
                             f'ratio from above at these values, so they must be >= 0 (1.0 is the usual choice)')
        self.replay_rollouts = int(replay_rollouts)
        self.replay_rho_clip, self.replay_c_clip = float(replay_rho_clip), float(replay_c_clip)
        self.replay = RolloutReplay(self.replay_rollouts) if self.replay_rollouts > 0 else None
        self._replay_table = TrajectoryTable()      # trajectories stored since the last update()
        self._replay_active = []                    # the kept periods whose rows ride along in the running update()
        # utils.get_optimizer_by_name (reference rl/utils.py:29-46): one Keras optimizer class, by name, for the policy and value
        # optimizers (and CARLAgent's dynamics optimizer); it and polyak reach the learner engines through the network
        if str(optimizer).lower() not in OPTIMIZERS:
            raise ValueError(f'Cannot find optimizer {optimizer}. Select one of {OPTIMIZERS}.')
        self.optimizer_name = str(optimizer).lower()
        if str(clip_mode).lower() not in CLIP_MODES:
            raise ValueError(f'Unknown clip_mode {clip_mode}. Select one of {CLIP_MODES}.')
        self.clip_mode = str(clip_mode).lower()
        self.skip_nonfinite = bool(skip_nonfinite)
        self._gate_seen = dict(policy=0, value=0)      # skip counts already reported by an earlier update()
        self.train_stats_rows = int(train_stats_rows)
        super().__init__(*args, name=name, **kwargs)
        if demo_traces is not None:         # (behind the base class: the split needs batch_size; in front of the network: a refusal allocates nothing)
            self._init_demonstrations(demo_fraction, demo_weight, demo_rows, demo_seed, replay_rollouts)
        self.memory: PPOMemory = None
        self.gamma = gamma
        self.lambda_ = lambda_
        self.repeat_action = repeat_action
        self.adv_scale = DynamicParameter.create(value=advantage_scale)
        if seed_regularization:
            def _seed_regularization():
                self.set_random_seed(int(np.random.randint(0, 2 ** 31 - 1)))
            self.seed_regularization = _seed_regularization
            self.seed_regularization()
        else:
            self.seed_regularization = lambda: None
        self.entropy_strength = DynamicParameter.create(value=entropy_regularization)
        self.clip_ratio = DynamicParameter.create(value=clip_ratio)
        self._init_action_space()
        self._init_gradient_clipping(clip_norm)
        self.update_frequency = update_frequency
        self.policy_lr = DynamicParameter.create(value=policy_lr)
        self.value_lr = DynamicParameter.create(value=value_lr)
        self.optimization_steps = dict(policy=optimization_steps[0], value=optimization_steps[1])
        self.should_polyak_average = polyak < 1.0
        self.polyak_coeff = polyak
        if not isinstance(network, dict) or 'network' not in network:
            raise ValueError("PPOAgent needs network=dict(network=<Network class>, ...)")
        network = dict(network)
        network_class = network.pop('network')
        self.network = network_class(agent=self, **network)
        if load:
            self.load()

    # -- setup ------------------------------------------------------------------------------------
    def _init_gradient_clipping(self, clip_norm):
        def one(c):
            return (False, None) if c is None else (True, float(c))
        if clip_norm is None:
            clip_norm = (None, None)
        elif isinstance(clip_norm, float):
            assert clip_norm > 0.0
            clip_norm = (clip_norm, clip_norm)
        self.should_clip_policy_grads, self.grad_norm_policy = one(clip_norm[0])
        self.should_clip_value_grads, self.grad_norm_value = one(clip_norm[1])

    def _init_action_space(self):
        space = self.env.action_space
        if not (isinstance(space, utils.spaces.Box) and space.is_bounded()):
            raise NotImplementedError('only bounded Box action spaces (Beta policy) are on the native path')
        self.num_actions = space.shape[0]
        self.distribution_type = 'beta'
        self.action_low = np.asarray(space.low, dtype=np.float32)
        self.action_high = np.asarray(space.high, dtype=np.float32)
        self.action_range = self.action_high - self.action_low
        # (E, A) device sample in [0, 1] -> environment actions; one row (the reference's single environment) comes back as (A,)
        self.convert_action = lambda a: np.squeeze(a.detach().cpu().numpy() * self.action_range + self.action_low, axis=0) \
            if a.shape[0] == 1 else a.detach().cpu().numpy() * self.action_range + self.action_low

    # -- acting -----------------------------------------------------------------------------------
    def predict(self, state, *args, deterministic=False, **kwargs):
        """deterministic=True: the mode of the policy instead of a sample (no sampler offset is consumed); the keyword reaches
        the network only then, so a network without it keeps serving the sampled path."""
        if deterministic:
            return self.network.predict(inputs=state, deterministic=True)
        return self.network.predict(inputs=state)

    def act(self, state, *args, deterministic=False, **kwargs):
        if deterministic:
            return self.convert_action(self.network.predict(inputs=state, deterministic=True)[0])
        return self.convert_action(self.network.predict(inputs=state)[0])

    # -- update -----------------------------------------------------------------------------------
    def hyper_parameters(self) -> dict:
        hp = dict(policy_lr=self.policy_lr(), value_lr=self.value_lr(), clip_ratio=self.clip_ratio(),
                  entropy_coef=self.entropy_strength(),
                  clip_norm_policy=self.grad_norm_policy if self.should_clip_policy_grads else 0.0,
                  clip_norm_value=self.grad_norm_value if self.should_clip_value_grads else 0.0)
        if self.trust:       # (only engines built with trust=True take them)
            hp.update(target_kl=self.target_kl or 0.0, kl_stop_factor=self.kl_stop_factor, kl_coef=self.kl_penalty)
        return hp

    def update(self):
        t0 = time.time()
        self.seed_regularization()
        self.network.set_hparams(**self.hyper_parameters())
        if self.replay is not None:
            self.refresh_replay()
        if self.joint_update:
            return self._update_joint(t0)
        if self.trust:
            self.begin_trust_region()
        if self.demo_traces is not None:
            self.begin_demonstrations()
        value_batches = list(self.get_value_batches())
        policy_batches = list(self.get_policy_batches())
        policy_batches, value_batches = self.agree_on_batches(policy_batches, value_batches)
        for _ in range(self.optimization_steps['policy']):
            for batch in policy_batches:
                self.seed_regularization()
                if self._demo_active:
                    batch = self.with_demonstrations(batch)
                total_loss, grads = self.get_policy_gradients(batch)
                self.update_policy(grads)
                self.log(loss_total=total_loss, lr_policy=self.policy_lr.value)
            if self.trust and self.trust_region_left():
                break
        for _ in range(self.optimization_steps['value']):
            for batch in value_batches:
                self.seed_regularization()
                value_loss, grads = self.get_value_gradients(batch)
                self.update_value(grads)
                self.log(loss_value=value_loss, lr_value=self.value_lr.value)
        self.after_update()
        self.log_train_stats()
        self.log_gate_stats()
        if self.trust:
            self.end_trust_region()
        if self.demo_traces is not None:
            self.end_demonstrations()
        if self.replay is not None:
            self.keep_period()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        print(f'Update took {round(time.time() - t0, 3)}s')

    # -- expert demonstrations inside the update (demo_traces; rl/demonstrations.py) ---------------------------------
    def _init_demonstrations(self, fraction, weight, rows, seed, replay_rollouts):
        """Constructor half: every refusal, the split, the schedule and the generator.  Nothing touches the device."""
        if not isinstance(self.demo_traces, (str, os.PathLike)) or not os.path.isdir(self.demo_traces):
            raise ValueError(f'demo_traces={self.demo_traces!r} is not a directory of trace files (None turns demonstrations off)')
        if self.joint_update:
            raise ValueError('demo_traces needs the separate policy and value loops: the mixed policy pass has no joint form; create '
                             'the agent with joint_update=False')
        if replay_rollouts:
            raise ValueError('demo_traces and replay_rollouts > 0 exclude each other: kept rollout rows and demonstration rows would '
                             'both ride behind the fresh rows of a policy minibatch; create the agent with replay_rollouts=0')
        if self.trust:
            raise ValueError('demo_traces and target_kl / kl_penalty exclude each other: the anchor sweep of the trust-region guard '
                             'covers the rollout rows and has no demonstration rows')
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            raise ValueError('demo_traces runs in one process: every rank would draw demonstration rows of its own for a collective '
                             'step; create the data-parallel agents without it')
        self.demo_rows_per_batch, self.demo_fresh_rows = demo_split(self.batch_size, fraction)
        if int(rows) != rows or rows < self.demo_rows_per_batch:
            raise ValueError(f'demo_rows={rows!r}: the cap of the demonstration store, an integer of at least the '
                             f'{self.demo_rows_per_batch} rows a policy minibatch takes')
        self.demo_fraction, self.demo_store_cap = float(fraction), int(rows)
        self.demo_weight = DynamicParameter.create(value=demo_weight_checked(weight))
        self.demo_rng = np.random.default_rng(seed)
        self.demo_store, self._demo_block, self._demo_w = None, None, 0.0

    def load_demonstrations(self) -> DemonstrationStore:
        """The store, built at the first call: the traces of demo_traces in sorted file order through the checks and the windowing
        of imitate() (need_info: the auxiliary heads train on every row), until demo_rows rows are on the device."""
        if self.demo_store is None:
            def tensors():
                rows = 0
                for trace in traces.load_traces(self.demo_traces):
                    if rows >= self.demo_store_cap:      # counted, not uploaded
                        yield dict(u=torch.empty((self._check_trace(trace, True, 0.0), 0)))
                        continue
                    t = self._trace_tensors(trace, None, True, 0.0)
                    rows += int(t['u'].shape[0])
                    yield t
            self.demo_store = DemonstrationStore(tensors(), self.demo_store_cap, self.demo_rows_per_batch)
            print(f'[demonstrations] {self.demo_store.rows} rows of {self.demo_store.traces} traces on the device'
                  + (f'; {self.demo_store.left_out} rows left out (demo_rows={self.demo_store_cap})' if self.demo_store.left_out else ''))
        return self.demo_store

    def begin_demonstrations(self):
        """In front of the batch pipelines: the store (first call), this update()'s weight, the zeroed statistics block."""
        self._demo_w = float(self.demo_weight())
        self._demo_active = bool(np.float32(self._demo_w) > 0.0)       # (as the device will see it: demo_w > 0 makes the row a demonstration row)
        if not self._demo_active:
            return
        self.load_demonstrations()
        if self._demo_block is None:
            from ...engine import demo_block
            self._demo_block = demo_block(self.device)
        self._demo_block.zero_()

    def draw_demonstrations(self) -> dict:
        """D rows of the store for one minibatch step: one draw of the demonstration generator, one device gather per tensor."""
        return self.demo_store.gather(draw_rows(self.demo_rng, self.demo_store.rows, self.demo_rows_per_batch))

    def with_demonstrations(self, batch):
        """Hook: a policy minibatch of fresh rows -> what get_policy_gradients takes for the mixed pass (CARLAgent)."""
        raise NotImplementedError(f'{type(self).__name__} has no mixed policy pass: demo_traces is implemented by CARLAgent')

    def end_demonstrations(self):
        """Behind the minibatch loops: ONE small copy of the statistics block, logged as per-pass means."""
        if not self._demo_active:
            self.log(demo_weight=self._demo_w, demo_rows_per_batch=0)
            return
        self._demo_active = False
        from ...engine import read_demo_block
        st = read_demo_block(self._demo_block)
        n = max(1, st['passes'])
        self.log(loss_demo=st['loss_sum'] / n, demo_log_prob=st['log_prob_sum'] / n, demo_mode_error=st['mode_error_sum'] / n,
                 demo_rows_per_batch=st['rows_sum'] / n, demo_weight=self._demo_w)

    # -- trust-region guard (target_kl / kl_penalty) -----------------------------------------------------------------
    def begin_trust_region(self):
        """Behind refresh_replay(), in front of the batch pipelines: the anchor of this update() -- (alpha0, beta0) of the acting
        network on every policy row, fresh and kept, from ONE sweep of inference forwards in chunks of batch_size -- packed as
        (N, 2, A), which travels through the batch pipeline as one more component of the policy batch; and the trust block's reset.
        Nothing is sampled: the rollout sampler's offset and every generator stay where they were."""
        states = self.with_replay(self.memory.states, 'states')
        alpha, beta, _ = self.network.distribution_and_value(states, chunk=self.batch_size)
        self._trust_anchor = torch.stack([alpha, beta], dim=1).contiguous()
        self._trust_stats = None
        self.network.engine.trust_reset()

    def trust_region_left(self) -> bool:
        """After a policy epoch: ONE small copy of the trust block (the only host read the guard adds).  True when the latch is
        set: inside the epoch the device already left out every apply behind the pass that set it."""
        self._trust_stats = self.network.engine.trust_stats()
        return bool(self._trust_stats['stop'])

    def end_trust_region(self):
        st, self._trust_anchor = self._trust_stats, None
        if st is None or not st['passes']:
            return
        self.log(kl_divergence=st['kl_sum'] / st['passes'], kl_divergence_max=st['kl_max'], kl_stopped_steps=st['skipped'],
                 kl_stop_pass=st['stop_pass'])
        if st['stop']:
            print(f"[update] policy steps stopped early: KL {st['kl_max']:.3g} above {self.kl_stop_factor} * target_kl "
                  f"{self.target_kl:.3g} at policy pass {st['stop_pass']}; {st['skipped']} minibatch steps left out")

    def _update_joint(self, t0):
        """update() with joint_update=True: one loop of optimization_steps['policy'] passes over the policy batch pipeline (the
        policy's shuffle settings, one generator draw), every minibatch carrying the returns as well; each step is one joint pass
        (one trunk forward and backward for both losses) and one joint apply (one trunk optimizer step)."""
        batches, _ = self.agree_on_batches(list(self.get_joint_batches()), [])
        for _ in range(self.optimization_steps['policy']):
            for batch in batches:
                self.seed_regularization()
                (total_loss, value_loss), grads = self.get_joint_gradients(batch)
                self.apply_joint_gradients(grads)
                self.log(loss_total=total_loss, loss_value=value_loss, lr_policy=self.policy_lr.value, lr_value=self.value_lr.value)
        self.after_update()
        self.log_train_stats()
        self.log_gate_stats()
        if self.replay is not None:
            self.keep_period()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        print(f'Update took {round(time.time() - t0, 3)}s')

    def agree_on_batches(self, policy_batches, value_batches):
        """Hook for data-parallel agents: every rank must run the same number of minibatch steps (each one is a collective)."""
        return policy_batches, value_batches

    def after_update(self):
        """Hook for data-parallel agents (BatchNorm moving statistics are averaged once per update())."""

    def log_train_stats(self):
        """The reference's per-minibatch scalars of update() (ratio, entropy, loss terms, head means, gradients_norm_*; reference
        rl/agents/ppo.py:209-225 and the objectives of the agent), read from the engines' train-stats ring in ONE copy after the
        minibatch loops and logged under the reference's keys.  loss_total / loss_value / lr_* are logged by the loops above.
        Only the rank that writes summaries fetches; the others empty their ring."""
        fetch = getattr(self.network, 'train_stats', None)
        if fetch is None:
            return
        stats = fetch(fetch=self.is_writer())
        if stats is None:
            return
        if stats['dropped']:
            print(f"[train stats] ring of {self.train_stats_rows} rows was full: {stats['dropped']} oldest minibatch steps not logged "
                  f'(raise train_stats_rows)')
        for kw in train_stats.log_entries(stats['rows'], skip=train_stats.LOGGED_BY_UPDATE):
            self.log(**kw)

    def log_gate_stats(self):
        """Gradient-gate statistics of this update() (clip_mode='global' and / or skip_nonfinite): ONE copy after the minibatch
        loops, by the rank that writes summaries only (every rank decides alike: the counters agree)."""
        eng = getattr(self.network, 'engine', None)
        if eng is None or not getattr(eng, 'gated', False) or not self.is_writer():
            return
        stats = eng.gate_stats()
        new = {h: stats[h]['skipped'] - self._gate_seen[h] for h in ('policy', 'value')}
        self._gate_seen = {h: stats[h]['skipped'] for h in ('policy', 'value')}
        self.log(skipped_steps_policy=new['policy'], skipped_steps_value=new['value'])
        if self.clip_mode == 'global':
            self.log(gradients_global_norm_policy=stats['policy']['norm'], gradients_global_norm_value=stats['value']['norm'],
                     gradients_global_norm_dynamics=stats['value']['norm_dynamics'])
        if new['policy'] or new['value']:
            print(f"[update] non-finite gradients: skipped {new['policy']} policy and {new['value']} value minibatch steps")

    def update_policy(self, gradients):
        return self.apply_policy_gradients(gradients), True

    def update_value(self, gradients):
        return self.apply_value_gradients(gradients), True

    def get_policy_gradients(self, batch):
        raise NotImplementedError

    def get_value_gradients(self, batch):
        raise NotImplementedError

    def apply_policy_gradients(self, gradients):
        raise NotImplementedError

    def apply_value_gradients(self, gradients):
        raise NotImplementedError

    def get_joint_gradients(self, batch):
        raise NotImplementedError

    def apply_joint_gradients(self, gradients):
        raise NotImplementedError

    def value_batch_tensors(self):
        return self.with_replay(self.memory.states, 'states'), self.with_replay(self.memory.returns, 'returns_be')

    def policy_batch_tensors(self):
        return (self.with_replay(self.memory.states, 'states'), self.with_replay(self.memory.advantages, 'advantages'),
                self.with_replay(self.memory.actions, 'actions'), self.with_replay(self.memory.log_probabilities, 'log_probs'))

    # -- reuse of recent rollouts (replay_rollouts > 0; rl/replay.py) ----------------------------------------------
    def with_replay(self, fresh, name: str):
        """`fresh` (the memory's tensor, or dict of tensors, of one batch component) followed by the same component of every kept
        period that the running update() refreshed; `fresh` itself -- the same object -- when there is none.  name: 'states',
        'actions', 'log_probs' (the stored behaviour log-probabilities), 'advantages' / 'returns_be' (the V-trace targets), or a key
        of the periods' info targets."""
        if not self._replay_active:
            return fresh

        def part(p):
            if name in ('states', 'actions', 'log_probs'):
                return getattr(p, name)
            return p.targets[name] if name in p.targets else p.info[name]

        parts = [part(p) for p in self._replay_active]
        if isinstance(fresh, dict):
            return {k: torch.cat([fresh[k]] + [q[k] for q in parts], dim=0) for k in fresh}
        return torch.cat([fresh] + parts, dim=0)

    def replay_info(self, rows: int):
        """Hook: per-row auxiliary targets of the `rows` memory rows that a kept period must carry, as a dict of (rows,) device
        tensors, or None (this class has none)."""
        return None

    def refresh_replay(self):
        """First step of update() with a non-empty store: re-evaluates the acting network on every kept period's rows (inference
        forwards in chunks of batch_size, the last chunk padded with repeated rows; one more forward for the observations behind the
        truncated trajectories), then ONE V-trace launch over all kept trajectories gives the rows' advantages and value targets
        under the current policy.  The periods ride along in this update()'s batches (with_replay).  No per-trajectory host read;
        with logging on, one small copy (three scalars)."""
        self._replay_active = []
        periods = list(self.replay.periods)
        if not periods:
            return
        dev = self.device
        r_parts, v_parts, dense, lengths = [], [], dict(alpha=[], beta=[], actions=[], log_probs=[]), []
        for p in periods:
            alpha, beta, value = self.network.distribution_and_value(p.states, chunk=self.batch_size)
            S = len(p.trajectories)
            boot = torch.zeros((S, 2), dtype=torch.float32, device=dev)            # zero behind a terminal step
            if p.finals is not None:
                _, _, final_value = self.network.distribution_and_value(p.finals, chunk=self.batch_size)
                boot[torch.as_tensor(p.truncated, dtype=torch.int64, device=dev)] = final_value
            row_index, boot_index = (torch.as_tensor(i, device=dev) for i in p.padded_index())
            values_be = torch.empty((p.rows + S, 2), dtype=torch.float32, device=dev)
            values_be[row_index], values_be[boot_index] = value, boot
            rewards = torch.empty(p.rows + S, dtype=torch.float32, device=dev)
            rewards[row_index] = p.rewards
            rewards[boot_index] = boot[:, 0] * torch.pow(torch.tensor(10.0, device=dev), boot[:, 1])      # as end_trajectory
            r_parts.append(rewards)
            v_parts.append(values_be)
            for k, t in (('alpha', alpha), ('beta', beta), ('actions', p.actions), ('log_probs', p.log_probs)):
                dense[k].append(t)
            lengths += p.lengths
        cat = lambda parts: parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
        inputs = dict(rewards=cat(r_parts), values_be=cat(v_parts), alpha=cat(dense['alpha']), beta=cat(dense['beta']),
                      actions=cat(dense['actions']), log_prob_old=cat(dense['log_probs']))
        scale = float(self.adv_scale.value)
        out = utils.vtrace_segments(lengths=lengths, gamma=self.gamma, lambda_=self.lambda_, rho_bar=self.replay_rho_clip,
                                    c_bar=self.replay_c_clip, scale=scale, device=dev, **inputs)
        row = 0
        for p in periods:
            p.targets = dict(advantages=out['advantages'][row:row + p.rows], returns_be=out['returns_be'][row:row + p.rows])
            row += p.rows
        self.replay.last_refresh = dict(inputs, lengths=lengths, scale=scale, **out)
        self._replay_active = periods
        if self.statistics.mode is not None:
            rho = out['rho'].double()
            m = torch.stack([rho.mean(), (rho > self.replay_rho_clip).double().mean()]).cpu().numpy()       # the update()'s one copy
            self.log(replay_rows=row, replay_rho_mean=float(m[0]), replay_rho_clipped=float(m[1]))

    def keep_period(self):
        """Last step of update(): the fresh period -- the memory's rows with the trajectory table trajectory_stored() collected --
        moves into the store (the oldest kept period leaves when it is full); the periods that rode along drop their targets."""
        for p in self._replay_active:
            p.targets = None
        self._replay_active = []
        table, self._replay_table = self._replay_table, TrajectoryTable()
        m = self.memory
        n = len(m)
        if n == 0 or sum(rows for rows, _ in table.entries) != n:
            print(f'[replay] the trajectory table counts {sum(rows for rows, _ in table.entries)} rows, the memory holds {n}: period '
                  f'not kept (rows must reach the memory through store())')
            return
        self.replay.add(ReplayPeriod(states=m.states, actions=m.actions, log_probs=m.log_probabilities, rewards=m.rewards[:n],
                                     trajectories=table.entries, finals=table.stacked_finals(), info=self.replay_info(n)))

    def discard_period(self):
        """For an update() that returns without training (CARLAgent: memory too small): the rows are dropped, so is their table."""
        self._replay_table = TrajectoryTable()

    def clear_replay(self):
        """Empties the store of kept periods (replay_rollouts > 0); the next update() trains on fresh rows only."""
        if self.replay is not None:
            self.replay.clear()
        self._replay_active = []

    def _batches(self, tensors, shuffle, shuffle_batches, batch_size=None):
        return utils.data_to_batches(tensors=tensors, batch_size=batch_size or self.batch_size, drop_remainder=self.drop_batch_remainder,
                                     skip=self.skip_count, num_shards=self.obs_skipping, shuffle=shuffle,
                                     shuffle_batches=shuffle_batches, seed=int(self.rng.integers(2 ** 31)))

    def get_value_batches(self):
        return self._batches(self.value_batch_tensors(), True, False)

    def get_policy_batches(self):
        # (demonstrations: minibatches of the fresh rows alone; with_demonstrations puts D rows behind each)
        return self._batches(self.policy_batch_tensors(), self.shuffle, self.shuffle_batches,
                             self.demo_fresh_rows if self._demo_active else None)

    def joint_batch_tensors(self):
        return tuple(self.policy_batch_tensors()) + (self.with_replay(self.memory.returns, 'returns_be'),)

    def get_joint_batches(self):
        return self._batches(self.joint_batch_tensors(), self.shuffle, self.shuffle_batches)

    # -- learning loop ------------------------------------------------------------------------------
    @staticmethod
    def _period(every, episodes: int, end_keyword=False) -> int:
        """`save_every` / `render_every` of the reference's learn() as a period in episodes: False / None -> never,
        True -> every episode, 'end' (saving only) -> the last episode, an int -> that period (must divide `episodes`)."""
        if every is False or every is None:
            return episodes + 1
        if every is True:
            return 1
        if end_keyword and every == 'end':
            return episodes
        assert not isinstance(every, str) and episodes % every == 0
        return int(every)

    def learn(self, episodes: int, timesteps: int, save_every: Union[bool, str, int] = False,
              render_every: Union[bool, str, int] = False, close=True, envs: Optional[Sequence] = None, auto_reset=False):
        """The reference's training loop (rl/agents/ppo.py:464-568: roll out up to `timesteps` steps per episode, close the
        trajectory with the bootstrap value, update() every `update_frequency` episodes, then the host side effects) built around
        an ENVIRONMENT SHARD: `envs` (default `[self.env]`, the reference's case) are stepped in lockstep, one batched
        `predict` per step for all of them, their rows stay on the device, and at the end of the episode every environment's
        trajectory is appended to the memory with its own bootstrap value and its own returns / GAE(lambda).  With one environment
        the sequence of environment, sampler and memory operations is the reference's.
        `auto_reset=True` (opt-in): an environment that reports `done` before `timesteps` is reset on the spot
        and starts a new trajectory, so every environment records every step, and all trajectories of the rollout are closed by
        ONE segmented returns / GAE launch (PPOMemory.extend_trajectories) instead of one end_episode each."""
        assert episodes % self.update_frequency == 0
        mode = dict(auto_reset=True) if auto_reset else {}      # (not passed on otherwise: collect / store overrides keep their signature)
        save_period = self._period(save_every, episodes, end_keyword=True)
        render_period = self._period(render_every, episodes)
        shard = list(envs) if envs is not None else [self.env]
        try:
            self.memory = self.get_memory()
            for episode in range(1, episodes + 1):
                self.seed_regularization()
                self.on_episode_start()
                self.reset()
                rollout = self.collect(shard, timesteps, render=episode % render_period == 0, episode=episode, **mode)
                updating = episode % self.update_frequency == 0
                self.store(rollout, timesteps, keep_open=not updating, **mode)
                if updating:
                    self.update()
                    self.memory.delete()
                    self.memory = self.get_memory()
                self.log(episode_rewards=rollout.episode_reward if len(shard) > 1 else rollout.episode_reward[0])
                # host side effects: ONE writer under data parallelism (N ranks writing the same checkpoint / summary files
                # concurrently leave torn files), everyone waits for it
                if self.is_writer():
                    self.write_summaries()
                    if self.should_record:
                        self.record(episode)
                else:
                    self.statistics.stats = {}
                self.on_episode_end()
                if episode % save_period == 0:
                    # the writer's failure (disk full, permissions) must not leave the other ranks waiting in a bare barrier until the
                    # process-group timeout: the meeting point carries a status flag and every rank raises
                    failure = None
                    try:
                        if self.is_writer():
                            self.save()
                        elif self.full_state:
                            self.save_state()          # (a rank that is not the writer: its own counters and generators only)
                    except Exception as exc:           # noqa: BLE001 -- re-raised below, on every rank
                        failure = exc
                    self.rank_barrier(failed=failure is not None)
                    if failure is not None:
                        raise failure
        finally:
            if close:
                for env in shard:
                    env.close()

    # -- imitation: behaviour cloning on expert traces ------------------------------------------------
    def _traces_dir(self, traces_dir):
        path = traces_dir if traces_dir is not None else getattr(self, 'traces_dir', None)
        if path is None:
            raise ValueError('no traces directory: pass traces_dir=..., or create the agent with traces_dir=...')
        return path

    # -- device-resident trace sets --------------------------------------------------------------------
    def load_trace_set(self, traces_dir=None, **options):
        """The traces of a directory read once and kept on the device in their most compact lossless code (rl/trace_set.py):
        TraceSet.from_dir(self, traces_dir, **options) -- max_traces, storage, weights.  Wherever a call takes `traces_dir`
        (imitate, learn_representation, score_traces) the set may be passed in its place.  Nothing of the agent changes."""
        from ..trace_set import TraceSet
        return TraceSet.from_dir(self, self._traces_dir(traces_dir), **options)

    def _trace_source(self, traces_dir, shuffle_data=False, what='imitate'):
        """What a `traces_dir` argument names: -> (directory, None, False), or for a TraceSet (None, the checked set, whether
        shuffle_data='set' asks for minibatches mixed over the whole set)."""
        from ..trace_set import TraceSet
        mix = isinstance(shuffle_data, str)
        if mix and shuffle_data != 'set':
            raise ValueError(f"{what}(shuffle_data={shuffle_data!r}): True, False or 'set'")
        if not isinstance(traces_dir, TraceSet):
            if mix:
                raise ValueError(f"{what}(shuffle_data='set') draws minibatches across traces: it needs a trace set "
                                 f'(load_trace_set) in place of the directory')
            return self._traces_dir(traces_dir), None, False
        traces_dir.check_fits(self)
        if mix and (self.skip_count > 0 or self.obs_skipping > 1):
            raise ValueError(f"{what}(shuffle_data='set'): skip_data = {self.skip_count} and consider_obs_every = {self.obs_skipping} "
                             f'are per-trajectory notions; a mixed minibatch has no trajectory')
        return None, traces_dir, mix

    def _set_columns(self, trace_set, need_info: bool, value_weight: float) -> tuple:
        """The columns of a trace set that _trace_tensors would upload for these options; refuses what the set lacks in
        _check_trace's words."""
        if need_info and not trace_set.has_info:
            raise ValueError('trace has no info_speed / info_similarity: the auxiliary and value losses need them -- set '
                             'value_weight=0 and aux_weight=0 to clone the actions alone')
        if value_weight > 0.0 and not trace_set.has_value:
            raise ValueError('the trace set has no returns: a trace in it lacks a reward of one entry per step and the trailing one')
        return ('u',) + (('weight',) if trace_set.has_weight else ()) + (('speed', 'similarity') if need_info else ()) + \
            (('returns',) if value_weight > 0.0 else ())

    def _imitation_traces(self, path, trace_set, max_traces, weights, need_info: bool, value_weight: float):
        """One epoch's traces in an order drawn from self.rng: per trace a callable -> its tensors on the device (from its file, or
        from the trace set by one launch)."""
        if trace_set is None:
            for trace in traces.load_traces(path, max_amount=max_traces, shuffle=True, rng=self.rng):
                yield lambda trace=trace: self._trace_tensors(trace, weights, need_info, value_weight)
            return
        columns = self._set_columns(trace_set, need_info, value_weight)
        for i in trace_set.epoch_order(self.rng, max_traces):
            yield lambda i=i: trace_set.trace_tensors(i, columns, self.gamma)

    def _log_imitation(self, kept: list, with_returns: bool):
        """The metric rows the minibatches of imitate() left on the device: ONE device-to-host copy, one log entry per minibatch."""
        names = ('total', 'clone', 'entropy', 'speed', 'similarity')
        for m in torch.stack(kept).cpu().numpy():
            entry = {f'imitation_loss_{k}': float(m[j]) for j, k in enumerate(names)}
            entry['imitation_entropy'] = entry.pop('imitation_loss_entropy')
            entry['imitation_mode_error'] = float(m[7])
            if with_returns:
                entry['imitation_loss_value'] = float(m[8])
            self.log(**entry)

    def _clone_and_keep(self, batch: dict, weights3: tuple, kept: list):
        eng = self.clone_minibatch(batch, *weights3)
        row = [eng.buffer(2)[:8].clone()]       # CDRL_BUF_METRICS_P as the clone loss left it; copies stay on the device
        if 'returns' in batch:
            row.append(eng.buffer(3)[:1].clone())
        kept.append(torch.cat(row))

    def clone_minibatch(self, batch: dict, policy_weight: float, value_weight: float, aux_weight: float):
        """Hook: one behaviour-cloning minibatch step (pass + apply) on `batch` -- dict(states, u, and optionally weight, speed,
        similarity, returns) of device tensors.  -> the learner engine that ran it (imitate reads its metric buffers)."""
        raise NotImplementedError

    def _check_trace(self, trace: dict, need_info: bool, value_weight: float) -> int:
        """Refuses a trace that does not fit the agent or the options, before anything is uploaded.  -> its number of rows."""
        keys = self.imitation_state_keys()
        missing = [k for k in keys if k not in trace]
        if missing or 'action' not in trace:
            raise ValueError(f"trace lacks {missing or ['action']}: it was recorded from another observation space; the agent needs "
                             f'{list(keys)} and action (traces.write_trace layout)')
        actions = np.asarray(trace['action'])
        n = actions.shape[0]
        if actions.reshape(n, -1).shape[1] != self.num_actions:
            raise ValueError(f'trace actions have width {actions.reshape(n, -1).shape[1]}, the agent has {self.num_actions} actions: '
                             f'collect the traces with the same action space')
        self._check_trace_states(trace, n)
        if need_info and ('info_speed' not in trace or 'info_similarity' not in trace):
            raise ValueError('trace has no info_speed / info_similarity: the auxiliary and value losses need them -- set '
                             'value_weight=0 and aux_weight=0 to clone the actions alone')
        if value_weight > 0.0 and np.size(trace.get('reward', ())) != n + 1:
            raise ValueError(f"trace reward has {np.size(trace.get('reward', ()))} entries; {n} steps need {n + 1} (the trailing one "
                             f'included)')
        return n

    def _check_trace_states(self, trace: dict, n=None) -> int:
        """The state entries of a trace against the agent's state_spec.  n: the row count they must have (None: that of the first
        state entry; a trace without actions).  -> the row count."""
        keys = self.imitation_state_keys()
        missing = [k for k in keys if k not in trace]
        if missing:
            raise ValueError(f'trace lacks {missing}: it was recorded from another observation space; the agent needs {list(keys)} '
                             f'(traces.write_trace layout)')
        if n is None:
            n = int(np.shape(trace[keys[0]])[0])
        T = int(getattr(self.env, 'time_horizon', 1))
        for k in keys:
            shape, want = tuple(np.shape(trace[k])), tuple(self.state_spec[k])
            if shape[:1] != (n,) or shape[1:] not in (want, (T,) + want):
                raise ValueError(f'trace {k} has shape {shape}; the agent needs ({n},) + {want} per step, or ({n}, {T}) + {want} '
                                 f'with the time_horizon axis')
        return n

    def _trace_states(self, trace: dict, n: int) -> dict:
        """The state entries of a checked trace on the device, uploaded once: stacked over time_horizon when the rows come without
        that axis (one windowing gather per key)."""
        T = int(getattr(self.env, 'time_horizon', 1))
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        index, states = None, {}
        for k in self.imitation_state_keys():
            want = tuple(self.state_spec[k])
            dev = up(trace[k])
            if tuple(dev.shape[1:]) == want and self.stacks_time():
                if index is None:
                    index = torch.as_tensor(traces.window_index(n, T)).to(self.device)
                dev = utils.gather_rows(dev, index).view((n, T) + want)
            states[k] = dev
        return states

    def _trace_tensors(self, trace: dict, weights, need_info: bool, value_weight: float) -> dict:
        """One trace on the device, uploaded once: states (stacked over time_horizon when the rows come without that axis, one
        windowing gather per key), unit actions, and what the options ask for (weight, speed / similarity, returns)."""
        n = self._check_trace(trace, need_info, value_weight)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        out = dict(states=self._trace_states(trace, n), u=up(traces.unit_actions(np.asarray(trace['action']).reshape(n, -1), self.action_low, self.action_high)))
        if weights is not None:
            w = np.asarray(weights(trace), dtype=np.float32).reshape(-1)
            if w.shape[0] != n:
                raise ValueError(f'weights(trace) returned {w.shape[0]} values for a trace of {n} rows')
            out['weight'] = up(w)
        if need_info:
            out['speed'] = up(np.reshape(trace['info_speed'], -1)) / 100.0
            out['similarity'] = up(np.reshape(trace['info_similarity'], -1))
        if value_weight > 0.0:
            # returns of the whole trace in one launch: zero values, the trace's own trailing reward as the bootstrap entry
            zeros = torch.zeros((n + 1, 2), dtype=torch.float32, device=self.device)
            out['returns'] = utils.returns_and_advantages(np.reshape(trace['reward'], -1), zeros, self.gamma, 0.0, 1.0,
                                                          self.device)['returns_be']
        return out

    def imitation_state_keys(self) -> list:
        """The state entries a trace must carry (those the network reads)."""
        return list(self.state_spec)

    def stacks_time(self) -> bool:
        """Whether the learner's state rows carry a time_horizon axis in front of the per-step shape (CARLAgent: yes)."""
        return False

    def imitate(self, epochs=1, batch_size: Union[None, int] = None, shuffle_batches=False, shuffle_data=False, close=True, seed=None,
                *, traces_dir=None, policy_weight=1.0, value_weight=0.0, aux_weight=1.0, lr=None, clip_norm=None, weights=None,
                max_traces=None):
        """Supervised pre-training on `trace-*.npz` files (traces.py): maximum likelihood of the recorded action under the policy's
        Beta (behaviour cloning), plus -- value_weight > 0 -- the value loss on the traces' discounted returns, one minibatch step
        per batch through the clone pass (one trunk forward and backward).  The first six parameters are the reference's
        PPOAgent.imitate (rl/agents/ppo.py:415-462); its body is PPO on self-collected traces, which has no meaning for traces of
        another expert, so the objective is this project's own.
        Per epoch the files are read in an order drawn from `self.rng`; each trace is uploaded once and cut into minibatches by the
        update()'s pipeline (skip_data, consider_obs_every, drop_batch_remainder; shuffle_data / shuffle_batches as given).
        policy_weight / value_weight scale the two losses' gradients, aux_weight the speed / similarity terms of the clone loss.
        lr / clip_norm: one learning rate / clip threshold for all optimizers during the run (the agent's own come back afterwards,
        also after an error).  weights: callable(trace dict) -> (N,) per-row weights.  max_traces: read at most that many files.
        No augmentation; the rollout sampler and the re-sampling offsets are not touched.  Ends with update_old_policy().
        traces_dir may be a TraceSet (load_trace_set) in place of the directory: the same loop with every trace's tensors made from the
        device-resident set by one launch instead of read from its file -- the same order, the same draws, the same bits; its
        weights are those it was loaded with.  With a set, shuffle_data='set' mixes the traces: per epoch ONE true permutation of
        all rows of the set (plan_epoch, from a generator seeded by one self.rng draw) uploaded once, every minibatch drawn across
        the traces by one launch, one device-to-host copy per epoch; skip_data, consider_obs_every and max_traces are
        per-trajectory notions and refused."""
        if getattr(self, 'data_parallel', False):
            raise RuntimeError('imitate() runs on one GPU: pre-train in a single process, save(), and load the weights in the '
                               'data-parallel run')
        path, trace_set, mix_traces = self._trace_source(traces_dir, shuffle_data, 'imitate')
        if trace_set is not None and weights is not None:
            raise ValueError('imitate(weights=...) with a trace set: the set evaluates the weights when it is loaded '
                             '(load_trace_set(weights=...))')
        if mix_traces and max_traces is not None:
            raise ValueError(f"imitate(shuffle_data='set', max_traces={max_traces}): max_traces is a per-trajectory notion; a mixed "
                             f'minibatch has no trajectory (load the set with max_traces instead)')
        batch_size = self.batch_size if batch_size is None else int(batch_size)
        if seed is not None:
            self.set_random_seed(seed)
        policy_weight, value_weight, aux_weight = float(policy_weight), float(value_weight), float(aux_weight)
        need_info = value_weight > 0.0 or aux_weight > 0.0
        base = self.hyper_parameters()
        run = dict(base)
        if lr is not None:
            run.update({k: float(lr) for k in base if k.endswith('_lr')})
        if clip_norm is not None:
            run.update({k: float(clip_norm) for k in base if k.startswith('clip_norm_')})
        weights3 = (policy_weight, value_weight, aux_weight)
        try:
            self.network.set_hparams(**run)
            for epoch in range(1, epochs + 1):
                if mix_traces:
                    t0 = time.time()
                    columns = self._set_columns(trace_set, need_info, value_weight)
                    order, cuts = trace_set.plan_epoch(np.random.default_rng(int(self.rng.integers(2 ** 31))), batch_size,
                                                       self.drop_batch_remainder)
                    index = trace_set.upload_index(order)       # the epoch's whole row order, uploaded once
                    kept = []
                    for offset, rows in cuts:
                        self._clone_and_keep(trace_set.batch(index, offset, rows, columns, self.gamma), weights3, kept)
                    if kept:        # ONE device-to-host copy per epoch
                        self._log_imitation(kept, 'returns' in columns)
                    self.write_summaries()
                    print(f'[{epoch}] {len(cuts)} mixed minibatches took {round(time.time() - t0, 3)}s.')
                for i, load in enumerate(() if mix_traces else self._imitation_traces(path, trace_set, max_traces, weights, need_info,
                                                                                     value_weight)):
                    t0 = time.time()
                    data = load()
                    order = [k for k in ('u', 'weight', 'speed', 'similarity', 'returns') if k in data]
                    batches = utils.data_to_batches((data['states'],) + tuple(data[k] for k in order), batch_size=batch_size,
                                                    shuffle_batches=shuffle_batches, shuffle=shuffle_data,
                                                    seed=int(self.rng.integers(2 ** 31)), skip=self.skip_count,
                                                    num_shards=self.obs_skipping, drop_remainder=self.drop_batch_remainder)
                    kept = []
                    for states, *rest in batches:
                        self._clone_and_keep(dict(zip(order, rest), states=states), weights3, kept)
                    if kept:        # ONE device-to-host copy per trace
                        self._log_imitation(kept, 'returns' in data)
                    self.write_summaries()
                    print(f'[{epoch}] Trace-{i} took {round(time.time() - t0, 3)}s.')
                if self.imitation_epoch_end(epoch):
                    break
            self.network.update_old_policy()
        finally:
            self.network.set_hparams(**base)
            fetch = getattr(self.network, 'train_stats', None)
            if fetch is not None:
                fetch(fetch=False)          # the imitation steps' rows never reach the next update()'s log
            if close:
                self.env.close()

    def imitation_epoch_end(self, epoch: int) -> bool:
        """Hook: called by imitate() behind every epoch; True ends the run early (the final update_old_policy() still runs).  An agent
        that validates on held-out traces does it here (CARLAgent.imitate(validation_dir=...))."""
        return False

    def score_traces(self, traces_dir=None, *, max_traces=None, chunk=None, value=True, aux=True, per_trace=False) -> dict:
        """Hook: how well the acting policy fits expert traces it is NOT trained on -- log-likelihood, mode error, bias, RMSE,
        calibration of the Beta's spread, and the value head against the traces' returns.  Needs a device scoring pass over the
        acting network's outputs; implemented by CARLAgent."""
        raise NotImplementedError(f'{type(self).__name__} has no scoring pass: score_traces is implemented by CARLAgent')

    def learn_representation(self, epochs=1, batch_size: Union[None, int] = None, *, traces_dir=None, temperature=0.1, intensity=1.0,
                             vector_inputs='zero', lr=None, shuffle_data=True, max_traces=None, seed=None, close=False):
        """Hook: the representation stage of the reference's curriculum (Stage.representation_learning, core/learning.py, calls
        agent.learn_representation(**repr_args); the reference defines it on no agent).  An agent with a shared trunk implements it
        (CARLAgent: contrastive pre-training of the trunk on trace files); this class has no trunk of its own."""
        raise NotImplementedError(f'{type(self).__name__} has no shared trunk to pre-train: learn_representation is implemented by '
                                  f'CARLAgent')

    def collect_traces(self, episodes: int, timesteps: int, envs: Optional[Sequence] = None, record_threshold=0.0, seeds=None,
                       deterministic=False, traces_dir=None, close=False) -> list:
        """The reference's PPOAgent.collect (rl/agents/ppo.py:360-413) on an environment shard: `episodes` rollouts of up to
        `timesteps` steps with the CURRENT policy (deterministic=True: its mode), every environment's episode whose reward reaches
        `record_threshold` written as one trace (traces.write_trace: states as observed, actions in environment units, the info
        buffer's speed / similarity).  Nothing is appended to self.memory.  seeds: an int seeds the agent once, a list draws one
        seed per episode.  -> the paths written.  A trained agent's traces are what another agent -- another compute mode, another
        head size -- is distilled from with imitate()."""
        path = self._traces_dir(traces_dir)
        shard = list(envs) if envs is not None else [self.env]
        if isinstance(seeds, int):
            self.set_random_seed(seeds)
        written = []
        sampled = self.predict
        try:
            if deterministic:
                self.predict = lambda state, *a, **kw: sampled(state, deterministic=True)
            for episode in range(1, episodes + 1):
                if isinstance(seeds, (list, tuple)):
                    self.set_random_seed(int(seeds[int(self.rng.integers(len(seeds)))]))
                self.reset()
                before = [len(env.info_buffer['speed']) if hasattr(env, 'info_buffer') else 0 for env in shard]
                rollout = self.collect(shard, timesteps, episode=episode)
                for e, env in enumerate(shard):
                    self.log(evaluation_reward=rollout.episode_reward[e])
                    if rollout.episode_reward[e] < record_threshold:
                        print(f'Trace-{episode} [env {e}] discarded: reward {round(rollout.episode_reward[e], 2)} below the threshold')
                        continue
                    states, actions, rewards, _, _ = rollout.trajectory(e)
                    n = rollout.length[e]
                    info = None
                    if hasattr(env, 'info_buffer'):     # one entry per environment step: the last of each repeated action
                        info = {}
                        for k in ('speed', 'similarity'):
                            piece = np.asarray(env.info_buffer[k][before[e]:], dtype=np.float32)[self.repeat_action - 1::self.repeat_action][:n]
                            info[k] = np.pad(piece, (0, n - piece.shape[0]))
                    done = np.zeros(n, np.float32)
                    done[-1] = float(rollout.terminal[e])
                    written.append(traces.write_trace(path, episode, {k: v.cpu().numpy() for k, v in states.items()},
                                                      np.atleast_2d(self.convert_action(actions)), rewards, done, info))
                self.write_summaries()
            if self.memory is None or len(self.memory) == 0:     # the info buffers hold these rollouts' entries, not an update()'s
                for env in shard:
                    if hasattr(env, 'reset_info'):
                        env.reset_info()
        finally:
            if deterministic:
                del self.predict
            if close:
                for env in shard:
                    env.close()
        return written

    def is_writer(self) -> bool:
        """Hook for data-parallel agents: the rank that writes checkpoints, summaries and traces."""
        return True

    def rank_barrier(self, failed: bool = False):
        """Hook for data-parallel agents: all ranks meet here after the writer has written; `failed` = this rank's write raised --
        the hook must make EVERY rank raise then."""

    def observe(self, observations: list, preprocess_fn) -> dict:
        """Per-environment observations -> one dict of (E, ...) device tensors: keys get the reference's `state_` prefix, the
        agent's preprocess function runs per environment (it may return device tensors: the augmentation kernels), host arrays
        cross PCIe as ONE copy per key.  A preprocess function that carries a `shard` attribute (a callable: list of observations ->
        dict of (E, ...) device tensors) is called ONCE for several observations instead of once per environment."""
        shard = getattr(preprocess_fn, 'shard', None)
        if shard is not None and len(observations) > 1:
            return shard([{f'state_{k}': v for k, v in obs.items()} if isinstance(obs, dict) else obs for obs in observations])
        prepared = []
        for obs in observations:
            if isinstance(obs, dict):
                obs = {f'state_{k}': v for k, v in obs.items()}
            prepared.append(preprocess_fn(obs))
        if not isinstance(prepared[0], dict):
            prepared = [dict(state=p) for p in prepared]
        out = {}
        for key in prepared[0]:
            vals = [p[key] for p in prepared]
            if any(isinstance(v, torch.Tensor) for v in vals):
                vals = [v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float32)) for v in vals]
                out[key] = torch.stack([v.to(device=self.device, dtype=torch.float32) for v in vals], dim=0)
            else:
                out[key] = torch.as_tensor(np.stack([np.asarray(v, dtype=np.float32) for v in vals], axis=0)).to(self.device)
        return out

    def collect(self, shard: list, timesteps: int, render=False, episode=0, auto_reset=False) -> 'Rollout':
        """One episode of every environment of the shard, in lockstep.  An environment that terminates early keeps its last
        observation in the batch (its rows are not recorded any more), so the inference engine sees one shape throughout.
        `auto_reset`: it is reset instead and goes on recording (collect_auto_reset)."""
        if auto_reset:
            return self.collect_auto_reset(shard, timesteps, render=render, episode=episode)
        E = len(shard)
        preprocess_fn = self.preprocess()
        observations = [env.reset() for env in shard]
        rollout = Rollout(E, timesteps, self.device)
        running = list(range(E))
        t0 = time.time()
        batch = self.observe(observations, preprocess_fn)
        for t in range(1, timesteps + 1):
            if render:
                for e in running:
                    shard[e].render()
            action, mean, std, log_prob, value = self.predict(batch)
            rollout.record(batch, action, log_prob, value, running)
            env_actions = np.atleast_2d(self.convert_action(action))
            rewards = []
            for e in list(running):
                reward, done = 0.0, False
                for _ in range(self.repeat_action):
                    observations[e], reward, done, _ = shard[e].step(env_actions[e])
                    rollout.episode_reward[e] += reward
                    rollout.env_steps[e] += 1
                    if done:
                        break
                rollout.rewards[e].append(float(reward))
                rewards.append(reward)
                if done or t == timesteps:
                    rollout.terminal[e] = done
                    running.remove(e)
                    print(f'Episode {episode}{f" [env {e}]" if E > 1 else ""} terminated after {t} timesteps in '
                          f'{round(time.time() - t0, 3)}s with reward {round(rollout.episode_reward[e], 3)}.')
                    self.log(timestep=t)
            self.log(actions=action, rewards=rewards if E > 1 else rewards[0], distribution_mean=mean, distribution_std=std)
            batch = self.observe(observations, preprocess_fn)
            if not running:
                break
        rollout.final = batch               # the observation behind every environment's last recorded step
        return rollout

    def collect_auto_reset(self, shard: list, timesteps: int, render=False, episode=0) -> 'Rollout':
        """`timesteps` steps of every environment of the shard, in lockstep, one batched `predict` per step.  An environment that
        reports `done` at step t < timesteps has its trajectory closed as terminal, is reset, and starts a new trajectory with the
        next step; at t == timesteps the open trajectory is closed as terminal (`done`, no reset) or as truncated.  Every
        environment records every step; `rollout.segments[e]` lists its trajectories."""
        E = len(shard)
        preprocess_fn = self.preprocess()
        observations = [env.reset() for env in shard]
        rollout = Rollout(E, timesteps, self.device)
        everyone = list(range(E))
        trajectory_reward = [0.0] * E
        t0 = time.time()
        batch = self.observe(observations, preprocess_fn)
        for t in range(1, timesteps + 1):
            if render:
                for env in shard:
                    env.render()
            action, mean, std, log_prob, value = self.predict(batch)
            rollout.record(batch, action, log_prob, value, everyone)
            env_actions = np.atleast_2d(self.convert_action(action))
            rewards = []
            for e in everyone:
                reward, done = 0.0, False
                for _ in range(self.repeat_action):
                    observations[e], reward, done, _ = shard[e].step(env_actions[e])
                    rollout.episode_reward[e] += reward
                    trajectory_reward[e] += reward
                    rollout.env_steps[e] += 1
                    if done:
                        break
                rollout.rewards[e].append(float(reward))
                rewards.append(reward)
                if done or t == timesteps:
                    start, stop = rollout.close_segment(e, terminal=done)[:2]
                    print(f'Episode {episode}{f" [env {e}]" if E > 1 else ""} terminated after {stop - start} timesteps '
                          f'(step {t} of the rollout) in {round(time.time() - t0, 3)}s with reward {round(trajectory_reward[e], 3)}.')
                    self.log(timestep=stop - start)
                    trajectory_reward[e] = 0.0
                    if t < timesteps:
                        observations[e] = shard[e].reset()
            self.log(actions=action, rewards=rewards if E > 1 else rewards[0], distribution_mean=mean, distribution_std=std)
            batch = self.observe(observations, preprocess_fn)
        rollout.final = batch               # the observation behind every environment's last recorded step
        return rollout

    def store(self, rollout: 'Rollout', timesteps: int, keep_open: bool, auto_reset=False):
        """Appends every environment's trajectory to the memory: rows, bootstrap value (zero at a terminal state, the value
        head's estimate of the final observation otherwise), returns and GAE(lambda) of THAT trajectory (end_episode).
        `keep_open`: more rows follow before the next update() (update_frequency > 1) -- the bootstrap entry is removed again.
        `auto_reset`: the rollout holds several trajectories per environment; they are closed together (store_segments)."""
        if auto_reset:
            return self.store_segments(rollout, timesteps, keep_open)
        E = rollout.envs
        estimate = None
        if not all(rollout.terminal):
            t_last = max(rollout.length)
            estimate = self.network.predict_last_value(rollout.final, timestep=(t_last + 1) / timesteps, is_terminal=False)
        # `append` (reference: update_frequency > 1) = the memory's row index advances PAST rows only, because the bootstrap entry of
        # this trajectory is removed again before the next one arrives -- also the case between the trajectories of a shard
        append = self.update_frequency > 1 or E > 1
        for e in range(E):
            self.memory.extend(*rollout.trajectory(e))
            last_value = (self.network.predict_last_value(None, is_terminal=True) if rollout.terminal[e] else estimate[e:e + 1])
            self.end_episode(last_value, append=append)
            self.trajectory_stored(e, rollout)
            if keep_open or e < E - 1:
                self.memory.drop_bootstrap()
        rollout.blocks = None               # the trajectories were copied into the memory: release the timesteps-long staging blocks

    def store_segments(self, rollout: 'Rollout', timesteps: int, keep_open: bool):
        """Appends every trajectory of an auto-reset rollout to the memory, in memory order (Rollout.trajectories): one batched
        value estimate for the truncated ones, zero bootstrap for the terminal ones, then ONE segmented returns / GAE(lambda) launch
        for all of them (PPOMemory.extend_trajectories) and the logging of end_episode once per trajectory, in that order."""
        estimate = None
        if not all(rollout.terminal):
            t_last = max(rollout.length)
            estimate = self.network.predict_last_value(rollout.final, timestep=(t_last + 1) / timesteps, is_terminal=False)
        pieces, rows, last_values = [], [], []
        for e, segment, trajectory in rollout.trajectories():
            pieces.append((e, segment))
            rows.append(trajectory)
            last_values.append(self.network.predict_last_value(None, is_terminal=True) if segment[2] else estimate[e:e + 1])
        last_values = torch.cat([v.to(device=self.device, dtype=torch.float32).reshape(1, 2) for v in last_values], dim=0)
        scale = self.adv_scale()
        closed = self.memory.extend_trajectories(rows, last_values, self.gamma, self.lambda_, scale,
                                                 append=self.update_frequency > 1 or len(rows) > 1)
        for (e, segment), returns, values, advantages in zip(pieces, *closed):
            self.log(returns=returns, advantages=advantages, values=values, advantage_scale=self.adv_scale.value)
            self.trajectory_stored(e, rollout, segment)
        if keep_open:
            self.memory.drop_bootstrap()
        rollout.blocks = None

    def trajectory_stored(self, env_index: int, rollout: 'Rollout', segment=None):
        """Hook: environment `env_index`'s trajectory of this rollout now sits at the end of the memory.  `segment`: which one of the
        environment's trajectories (an entry of `rollout.segments[env_index]`) when the rollout was collected with auto-reset.
        With replay_rollouts > 0 this class records the trajectory table here (overrides call super()): rows, terminal flag and, for
        a truncated trajectory, the environment's row of `rollout.final`."""
        if self.replay is None:
            return
        if segment is not None:
            rows, terminal = segment[1] - segment[0], bool(segment[2])
        else:
            rows, terminal = rollout.length[env_index], bool(rollout.terminal[env_index])
        final = None
        if not terminal:
            final = {k: v[env_index:env_index + 1].clone() for k, v in rollout.final.items()}
        self._replay_table.record(rows, terminal, final)

    def get_memory(self):
        return PPOMemory(state_spec=self.state_spec, num_actions=self.num_actions, device=self.device)

    def end_episode(self, last_value, append=False):
        self.memory.end_trajectory(last_value)
        returns = self.memory.compute_returns(discount=self.gamma, append=append)
        values, advantages = self.memory.compute_advantages(self.gamma, self.lambda_, scale=self.adv_scale(), append=append)
        self.memory.update_index(append=append)
        self.log(returns=returns, advantages=advantages, values=values, advantage_scale=self.adv_scale.value)

    def summary(self):
        self.network.summary()

    def save_weights(self):
        self.network.save_weights()

    def load_weights(self):
        self.network.load_weights()

    # -- full state: bit-exact resume (learner_state.py) ----------------------------------
    def state_rank(self) -> Optional[int]:
        """Hook for data-parallel agents: this rank's number when every rank keeps host state of its own, else None."""
        return None

    def save_state(self):
        """Writes the full learner state under `base_path` (save() does with full_state=True): the network's device state
        (CARLANetwork.save_state: parameter arena with old_policy and the moving statistics, optimizer slots, step counters, Nadam
        m_caches, rollout sampler offset) and this agent's host_state().  A later load_state() continues the run as if it had not
        stopped: bit for bit, given an environment that is deterministic per episode or restores itself.
        Not saved: the environment (the user's object), and rows pending in the rollout memory -- exact resume holds when the save
        falls behind an update(), i.e. update_frequency=1 or save_every a multiple of update_frequency; otherwise the number of
        rows left out is printed.  The DynamicParameter steps travel in config.json (save_config).
        Data parallelism: the device state is identical on all ranks and written by the writer rank; every rank writes its own
        `learner_state.rank<r>.json` (its counters and generators differ: rank-offset seeds, early episode ends)."""
        from ... import learner_state
        pending = len(self.memory) if self.memory is not None else 0
        if pending:
            print(f'[save_state] {pending} rollout rows pending in the memory are not saved: a run resumed from this state starts '
                  f'the update period over')
        kept = self.replay.rows if getattr(self, 'replay', None) is not None else 0
        if kept:
            print(f'[save_state] {kept} kept rollout rows of the replay store ({len(self.replay)} periods) are not saved: a run '
                  f'resumed from this state refills the store from its first updates')
        host = self.host_state()
        rank = self.state_rank()
        if self.is_writer():
            self.network.save_state(self.base_path, extra=dict(agent=host))
        if rank is not None:
            opt = self.network.engine.get_optimizer_state()
            learner_state.save_rank(self.base_path, rank, dict(agent=host, optimizer_steps=[opt['t_policy'], opt['t_value'],
                                                                                            opt['t_dynamics']]))

    def load_state(self, missing_ok=False) -> bool:
        """Restores what save_state wrote (load() does, after the weights, with full_state=True).  Without a state under
        `base_path`: LearnerStateError, or with missing_ok one printed line and False -- the first stage of a curriculum loads
        weights only.  Data parallelism: every rank reads the device state and its own rank file; a rank without one (the world size
        changed) keeps its seed-derived counters and generators and says so."""
        from ... import learner_state
        if missing_ok and not learner_state.exists(self.base_path):
            print(f'[load_state] no learner state under {self.base_path}: weights only, fresh optimizer')
            return False
        meta = self.network.load_state(self.base_path)
        self.restore_host_state(meta)
        return True

    def restore_host_state(self, meta: dict):
        """Second half of load_state: `meta` is the state's JSON file."""
        from ... import learner_state
        rank = self.state_rank()
        if rank is None:
            self.set_host_state(meta['agent'])
            return
        own = learner_state.load_rank(self.base_path, rank)
        if own is None or own.get('optimizer_steps') != meta.get('optimizer_steps'):
            print(f'[load_state] rank {rank}: no {os.path.basename(learner_state.rank_json_path(self.base_path, rank))} that belongs '
                  f'to this state: keeping the seed-derived counters and generators')
            return
        self.set_host_state(own['agent'])

    def save_config(self):
        self.update_config(policy_lr=self.policy_lr.serialize(), value_lr=self.value_lr.serialize(),
                           adv_scale=self.adv_scale.serialize(), entropy_strength=self.entropy_strength.serialize(),
                           clip_ratio=self.clip_ratio.serialize())
        super().save_config()

    def load_config(self):
        super().load_config()
        for key, p in (('policy_lr', self.policy_lr), ('value_lr', self.value_lr), ('adv_scale', self.adv_scale),
                       ('entropy_strength', self.entropy_strength), ('clip_ratio', self.clip_ratio)):
            p.load(config=self.config.get(key, {}))

    def reset(self):
        super().reset()
        self.network.reset()

    def on_episode_end(self):
        super().on_episode_end()
        self.policy_lr.on_episode()
        self.value_lr.on_episode()
        self.adv_scale.on_episode()
        if self.demo_traces is not None:
            self.demo_weight.on_episode()

    def host_state(self) -> dict:
        """Agent.host_state; with demonstrations on also their generator and the weight's schedule step."""
        state = super().host_state()
        if self.demo_traces is not None:
            state['demo'] = dict(rng=self.demo_rng.bit_generator.state, weight=self.demo_weight.serialize())
        return state

    def set_host_state(self, state: dict):
        super().set_host_state(state)
        if self.demo_traces is not None:
            if 'demo' not in state:
                print('[load_state] the state was saved without demonstrations: their generator and schedule start over')
                return
            self.demo_rng.bit_generator.state = state['demo']['rng']
            self.demo_weight.load(config=state['demo']['weight'])


class Rollout:
    """What an environment shard stepped in lockstep leaves behind: (steps, E, ...) device blocks written in place, one per
    state component / action / log-probability / value, plus the host-side bookkeeping per environment (rewards, number of
    recorded steps, terminal flag).  `trajectory(e)` hands environment e's rows to the memory as contiguous blocks.
    With auto-reset an environment leaves several trajectories: `segments[e]` = [(start_step, stop_step, terminal,
    env_steps_at_start), ...] in time order, `trajectories()` hands them out in MEMORY ORDER -- environment 0's in time order, then
    environment 1's, and so on; `length[e]` / `terminal[e]` describe the environment's steps as a whole / its last trajectory."""

    def __init__(self, envs: int, timesteps: int, device):
        self.envs, self.timesteps, self.device = envs, timesteps, device
        self.blocks = None                                  # name -> (timesteps, E, ...) tensor, allocated by the first record()
        self.rewards = [[] for _ in range(envs)]
        self.length = [0] * envs
        self.env_steps = [0] * envs                         # environment steps incl. repeated actions (info-buffer entries)
        self.terminal = [False] * envs
        self.episode_reward = [0.0] * envs
        self.final = None
        self.step = 0
        self.segments = [[] for _ in range(envs)]
        self._open = [(0, 0)] * envs                        # (first step, environment steps taken before it) of the open trajectory

    def record(self, states: dict, action, log_prob, value, running):
        rows = dict(states)
        rows.update({'/action': action, '/log_prob': log_prob, '/value': value})
        if self.blocks is None:
            self.blocks = {k: torch.empty((self.timesteps,) + tuple(v.shape), dtype=torch.float32, device=self.device)
                           for k, v in rows.items()}
        for k, v in rows.items():
            self.blocks[k][self.step].copy_(v)
        self.step += 1
        for e in running:
            self.length[e] += 1

    def close_segment(self, e: int, terminal: bool):
        """Environment e's open trajectory ends with the step just recorded; the next recorded step starts a new one."""
        start, env_steps = self._open[e]
        segment = (start, self.length[e], bool(terminal), env_steps)
        assert segment[1] > start, 'a trajectory holds at least one step'
        self.segments[e].append(segment)
        self._open[e] = (self.length[e], self.env_steps[e])
        self.terminal[e] = bool(terminal)
        return segment

    def trajectories(self):
        """-> (e, segment, (states, actions, rewards, values, log_probs)) per trajectory, in memory order."""
        for e in range(self.envs):
            for segment in self.segments[e]:
                start, stop = segment[:2]
                take = lambda k: self.blocks[k][start:stop, e].clone(memory_format=torch.contiguous_format)
                states = {k: take(k) for k in self.blocks if not k.startswith('/')}
                yield e, segment, (states, take('/action'), self.rewards[e][start:stop], take('/value'), take('/log_prob'))

    def trajectory(self, e: int):
        """-> (states, actions, rewards, values, log_probs) of environment e: its first `length[e]` steps."""
        n = self.length[e]
        # a COPY of the environment's rows: for one environment `[:n, 0].contiguous()` would be a view that keeps the whole
        # timesteps-long block alive inside the memory after an early episode end
        take = lambda k: self.blocks[k][:n, e].clone(memory_format=torch.contiguous_format)
        states = {k: take(k) for k in self.blocks if not k.startswith('/')}
        return states, take('/action'), self.rewards[e][:n], take('/value'), take('/log_prob')


class PPOMemory:
    """Rollout buffer resident in HBM.  Rows arrive one at a time (`append`, (1, ...) device tensors) or as whole
    trajectories (`extend`, (n, ...) blocks) and are concatenated on demand; returns / advantages come from the
    cdrl_gae_returns kernel."""

    def __init__(self, state_spec: dict, num_actions: int, device='cuda:0'):
        self.device = device
        self.index = 0
        self.simple_state = list(state_spec.keys()) == ['state']
        self.state_spec = state_spec
        self.num_actions = num_actions
        self._states = [] if self.simple_state else {name: [] for name in state_spec}
        self._rewards, self._values, self._actions, self._log_probs = [], [], [], []
        self.returns = None
        self.advantages = None
        self._cache = {}
        self._n = 0

    def __len__(self):
        return self._n

    def delete(self):
        self._states = None
        self._rewards = self._values = self._actions = self._log_probs = None
        self.returns = self.advantages = None
        self._cache = {}
        self._n = 0

    @staticmethod
    def _row(x, device, width=None):
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
        t = t.to(device=device, dtype=torch.float32)
        return t.reshape(1, -1) if width else t

    def append(self, state, action, reward, value, log_prob):
        self._cache = {}
        if self.simple_state:
            self._states.append(self._row(state, self.device))
        else:
            assert isinstance(state, dict)
            for k, v in state.items():
                if k in self._states:
                    self._states[k].append(self._row(v, self.device))
        self._actions.append(self._row(action, self.device, True))
        self._rewards.append(float(reward))
        self._values.append(self._row(value, self.device, True))
        self._log_probs.append(self._row(log_prob, self.device, True))
        self._n += 1

    def extend(self, states, actions, rewards, values, log_probs):
        """A whole trajectory of n rows: (n, ...) device blocks (state dict or tensor, actions (n, A), values (n, 2),
        log-probabilities (n, A)) and n host rewards."""
        n = int(actions.shape[0])
        if n == 0:
            return
        self._cache = {}
        if self.simple_state:
            self._states.append(states['state'] if isinstance(states, dict) else states)
        else:
            for k, v in states.items():
                if k in self._states:
                    self._states[k].append(v)
        self._actions.append(actions.reshape(n, -1))
        self._rewards.extend(float(r) for r in rewards)
        self._values.append(values.reshape(n, -1))
        self._log_probs.append(log_probs.reshape(n, -1))
        self._n += n

    def _cat(self, key, rows):
        if key not in self._cache:
            self._cache[key] = torch.cat(rows, dim=0).contiguous()
        return self._cache[key]

    @property
    def states(self):
        if self.simple_state:
            return self._cat('states', self._states)
        return {k: self._cat(f'states/{k}', v) for k, v in self._states.items()}

    @property
    def actions(self):
        return self._cat('actions', self._actions) if self._actions else torch.zeros((0, self.num_actions), device=self.device)

    @property
    def log_probabilities(self):
        return self._cat('log_probs', self._log_probs)

    @property
    def values(self):
        return self._cat('values', self._values)

    @property
    def rewards(self):
        if 'rewards' not in self._cache:
            self._cache['rewards'] = torch.as_tensor(np.asarray(self._rewards, dtype=np.float32), device=self.device)
        return self._cache['rewards']

    def end_trajectory(self, last_value):
        """bootstrap: reward <- base * 10^exp of the last value, value <- last_value."""
        lv = self._row(last_value, self.device, True)
        self._cache = {}
        self._rewards.append(float((lv[0, 0] * torch.pow(torch.tensor(10.0, device=lv.device), lv[0, 1])).item()))
        self._values.append(lv)

    def extend_trajectories(self, trajectories, last_values, gamma: float, lambda_: float, scale=2.0, append=False):
        """Appends S whole trajectories -- `trajectories`: [(states, actions, rewards, values, log_probs), ...] as `extend` takes them,
        `last_values`: (S, 2) device tensor of their bootstrap values (zeros behind a terminal step) -- and closes ALL of them with one
        segmented returns / GAE launch.  The memory ends up exactly as `extend` + end_trajectory + compute_returns +
        compute_advantages + update_index(append=True) + drop_bootstrap per trajectory (all but the last drop) would leave it:
        `_rewards` / `_values` keep the last trajectory's bootstrap entry only, `index` = number of rows.  The returns scan does not
        depend on lambda, so `returns_be` of the (gamma, lambda_, scale) launch is what compute_returns' (gamma, 0, 1) launch gives.
        One device-to-host read (the bootstrap reward `_rewards` keeps as a float).  No bootstrap entry may be open on entry.
        -> (returns, values, raw advantages): three tuples of per-trajectory views, what end_episode logs."""
        trajectories = list(trajectories)
        S = len(trajectories)
        lengths = [int(t[1].shape[0]) for t in trajectories]
        if S < 1 or min(lengths) < 1:
            raise ValueError(f'extend_trajectories: every trajectory needs at least one row (lengths {lengths})')
        lv = last_values.to(device=self.device, dtype=torch.float32).reshape(-1, 2)
        if lv.shape[0] != S:
            raise ValueError(f'extend_trajectories: {S} trajectories, {lv.shape[0]} last values')
        first = len(self._rewards)
        for t in trajectories:
            self.extend(*t)
        # padded sequences: every trajectory followed by its bootstrap entry (the elementwise ops of end_trajectory, for all S at once)
        boot = lv[:, 0] * torch.pow(torch.tensor(10.0, device=lv.device), lv[:, 1])
        rows = torch.as_tensor(np.asarray(self._rewards[first:], dtype=np.float32), device=self.device)
        r_parts, v_parts, off = [], [], 0
        for s, n in enumerate(lengths):
            r_parts += [rows[off:off + n], boot[s:s + 1]]
            v_parts += [self._values[len(self._values) - S + s], lv[s:s + 1]]
            off += n
        rewards, values_be = torch.cat(r_parts), torch.cat(v_parts, dim=0)
        out = utils.returns_and_advantages_segments(rewards, values_be, lengths, gamma, lambda_, scale, device=self.device)
        keep = append and self.returns is not None
        self.returns = torch.cat([self.returns, out['returns_be']], dim=0) if keep else out['returns_be']
        self.advantages = torch.cat([self.advantages, out['advantages']], dim=0) if keep else out['advantages']
        self._cache = {}
        self._rewards.append(float(boot[S - 1].item()))
        self._values.append(lv[S - 1:S])
        self.index = len(self._rewards) - 1
        values = values_be[:, 0] * torch.pow(torch.tensor(10.0, device=values_be.device), values_be[:, 1])
        return (torch.split(out['returns'], lengths), torch.split(values, [n + 1 for n in lengths]),
                torch.split(out['advantages_raw'], lengths))

    def drop_bootstrap(self):
        self._cache = {}
        self._rewards = self._rewards[:-1]
        self._values = self._values[:-1]

    def _kernel(self, gamma, lambda_, scale):
        return utils.returns_and_advantages(self.rewards[self.index:], self.values[self.index:], gamma, lambda_, scale,
                                            device=self.device)

    def compute_returns(self, discount: float, append=False):
        out = self._kernel(discount, 0.0, 1.0)
        new = out['returns_be']
        self.returns = new if (self.returns is None or not append) else torch.cat([self.returns, new], dim=0)
        return out['returns']

    def compute_advantages(self, gamma: float, lambda_: float, scale=2.0, append=False):
        out = self._kernel(gamma, lambda_, scale)
        new = out['advantages']
        self.advantages = new if (self.advantages is None or not append) else torch.cat([self.advantages, new], dim=0)
        v = self.values[self.index:]
        return v[:, 0] * torch.pow(torch.tensor(10.0, device=v.device), v[:, 1]), out['advantages_raw']

    def update_index(self, append=False):
        self.index = len(self._rewards) - 1 if append else len(self._rewards)

    def serialize(self, episode: int, save_path: str):
        path = os.path.join(save_path, f'trace-{episode}-{time.strftime("%Y%m%d-%H%M%S")}.npz')
        buf = dict(reward=self.rewards.cpu().numpy(), action=self.actions.cpu().numpy(), value=self.values.cpu().numpy(),
                   log_prob=self.log_probabilities.cpu().numpy())
        st = self.states
        if self.simple_state:
            buf['state'] = st.cpu().numpy()
        else:
            buf.update({k: v.cpu().numpy() for k, v in st.items()})
        np.savez_compressed(file=path, **buf)

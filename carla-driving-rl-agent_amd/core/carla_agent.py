"""CARLAgent / CARLAMemory / FakeCARLAEnvironment on the native learner.

Surface follows the reference core/carla_agent.py: constructor keywords (:70-72), class-level
DEFAULT_* architectures (:61-68), update() guard (:129-145), policy / value batch tensors
(:323-349), get_*_gradients / apply_*_gradients (:351-388, :430-463), CARLAMemory (:586-596) and
the FakeCARLAEnvironment entry point (:26-52), evaluate() (:205-321, here over an environment shard).  record() needs the
simulator's frame recorder and is outside what this package implements: it raises instead of pretending.
"""
import json
import os
import time
import warnings

import numpy as np
import torch
import torch.distributed as dist

from .. import _lib, traces, train_stats
from ..engine import act_stats_width, occlusion_baseline, read_score_block, score_block
from ..explain import BASELINES, MODALITIES, check_arguments, occlusion_frames, score_names
from ..evaluation import RESULT_KEYS, evaluation_info, summarize, trial_seed
from ..parallel import DataParallelLearner
from ..rl import utils, spaces
from ..rl.agents.ppo import PPOAgent, PPOMemory
from ..rl.parameters import DynamicParameter
from .networks import CARLANetwork, relu6


class FakeCARLAEnvironment(spaces.Env):
    """Environment with the state / action spaces of a CARLA environment and no simulator.

    Defaults reproduce the reference's class (three-camera image (90, 360, 3) in [-1, 1], road 9,
    vehicle 5, past_control 4, command 6, navigation 10, action Box(-1, 1, (3,)), time_horizon 1).
    Superset for running the learner without CARLA: every size is overridable, step() / reset()
    return seeded synthetic observations stacked over `time_horizon`, and `info_buffer` /
    `reset_info()` exist as CARLAgent.update() expects from the real CARLAEnv."""

    def __init__(self, image_shape=(90, 360, 3), time_horizon=1, num_waypoints=10, vehicle_features=5, road_features=9,
                 num_actions=3, image_range=(-1.0, 1.0), episode_length=None, seed=0):
        super().__init__()
        self.num_waypoints = num_waypoints
        self.NAVIGATION_FEATURES = dict(space=spaces.Box(low=0.0, high=25.0, shape=(num_waypoints,)),
                                        default=np.zeros(shape=num_waypoints, dtype=np.float32))
        self.time_horizon = time_horizon
        self.action_space = spaces.Box(low=-1.0, high=1.0, shape=(num_actions,))
        self.observation_space = spaces.Dict(
            road=spaces.Box(low=0.0, high=15.0, shape=(road_features,)),
            vehicle=spaces.Box(low=-np.inf, high=np.inf, shape=(vehicle_features,)),
            past_control=spaces.Box(low=-1.0, high=1.0, shape=(4,)), command=spaces.Box(low=0.0, high=1.0, shape=(6,)),
            image=spaces.Box(low=image_range[0], high=image_range[1], shape=tuple(image_shape)),
            navigation=self.NAVIGATION_FEATURES['space'])
        self.image_range = image_range
        self.episode_length = episode_length
        self.info_buffer = dict(speed=[], similarity=[])
        self._rng = np.random.default_rng(seed)
        self._t = 0
        self._speed, self._similarity = 0.0, 0.0        # what step() last drew (evaluation_info)
        self.current_town = None

    def set_town(self, town):
        self.current_town = town

    def evaluation_info(self):
        """-> (similarity, speed, waypoint_distance, collided) after a step, for CARLAgent.evaluate: the similarity and speed
        step() last drew, a waypoint distance derived from them (5 * (1 - |similarity|)), and `collided` exactly when
        `episode_length` is reached.  Draws nothing from the generator: a seeded observation sequence is the same with and
        without these calls."""
        collided = self.episode_length is not None and self._t >= self.episode_length
        return self._similarity, self._speed, 5.0 * (1.0 - abs(self._similarity)), collided

    def seed(self, seed=None):
        self._rng = np.random.default_rng(seed)

    def reset_info(self):
        self.info_buffer = dict(speed=[], similarity=[])

    def _observation(self):
        T, sp = self.time_horizon, self.observation_space.spaces
        lo, hi = self.image_range
        obs = dict(image=self._rng.uniform(lo, hi, size=(T,) + sp['image'].shape).astype(np.float32),
                   road=self._rng.integers(0, 2, size=(T,) + sp['road'].shape).astype(np.float32),
                   vehicle=self._rng.uniform(0.0, 1.0, size=(T,) + sp['vehicle'].shape).astype(np.float32),
                   navigation=np.sort(self._rng.uniform(0.0, 25.0, size=(T,) + sp['navigation'].shape), axis=-1).astype(np.float32),
                   past_control=np.zeros((T, 4), np.float32), command=np.zeros((T, 6), np.float32))
        return obs

    def reset(self):
        self._t = 0
        return self._observation()

    def step(self, action):
        self._t += 1
        speed = float(self._rng.uniform(0.0, 30.0))
        similarity = float(self._rng.uniform(-1.0, 1.0))
        self.info_buffer['speed'].append(speed)
        self.info_buffer['similarity'].append(similarity)
        self._speed, self._similarity = speed, similarity
        done = self.episode_length is not None and self._t >= self.episode_length
        return self._observation(), speed / 3.0 * abs(similarity), done, {}

    def render(self, mode='human'):
        pass


class CARLAgent(PPOAgent):
    _constructed = False        # load=True runs inside PPOAgent.__init__, before this class's counters and generators exist
    _pending_state_meta = None
    DEFAULT_CONTROL = dict(units=320, num_layers=2, activation=utils.swish6)
    DEFAULT_CONTROL_VALUE = dict(units=320, num_layers=2, activation=utils.swish6)
    DEFAULT_DYNAMICS = dict(road=dict(units=16, num_layers=2, activation=relu6),
                            vehicle=dict(units=16, num_layers=2, activation=relu6),
                            navigation=dict(units=16, num_layers=2, activation=relu6),
                            shufflenet=dict(g=1.0, last_channels=768),
                            rnn=dict(image=256, road=32, vehicle=32, navigation=32),
                            dynamics=dict(units=512))

    def __init__(self, *args, aug_intensity=1.0, clip_norm=(1.0, 1.0, 1.0), name='carla', load_full=True, eta=0.0,
                 dynamics_lr=1e-3, update_dynamics=True, delta=0.0, aux=1.0, resample_actions=True, compute='f32', batch_augment=False,
                 view_pipeline='agent', **kwargs):
        """`resample_actions=True` (default, the reference's behaviour): the policy loss is evaluated on a fresh Beta sample of
        the NEW policy with pathwise gradients, as PolicyNetwork.call does (reference core/networks.py:96-110);
        the sample is drawn on the device.  `False` is the textbook-PPO variant on the stored rollout actions
        (rl/agents/ppo.py:322-325 semantics; deterministic, same cost).
        `compute='bf16'`: the engine's bf16-operand mode (not in the reference; CARLANetwork docstring).
        `update_dynamics=False`: frozen trunk -- every minibatch step runs the trunk forward in training mode (its BatchNorm moving
        statistics update) and trains the policy / value heads only; `dynamics_lr` is then accepted and unused, as in the
        reference (core/carla_agent.py:351-373,430-463).  Typical use: load a trained trunk with `load_full=False`, fine-tune the heads.
        `optimizer=name` (PPOAgent): one Keras optimizer class for the policy, value AND dynamics optimizers, as the reference builds
        all three from the one name (core/carla_agent.py:123-124); `polyak < 1` averages the policy / value heads, not the trunk.
        `clip_norm=(policy, value, dynamics)`: with `clip_mode='tensor'` (PPOAgent; the default) the first two are the per-tensor
        tf.clip_by_norm thresholds of the heads and the third is parsed and unused -- the reference's trunk is never clipped (F9).
        With `clip_mode='global'` each optimizer's gradient list is clipped by its global norm: the heads with the first two, the
        trunk with the third (`clip_norm_dynamics` of hyper_parameters(): clip_norm[2] when it is a float, clip_norm itself when a
        single float, else 0 = unclipped).  `skip_nonfinite=True` (PPOAgent) works in both modes.
        `batch_augment=True` (with `aug_intensity > 0` and an environment shard): the image stacks of all E environments are
        augmented by ONE batched call per step (Augmenter.batch) instead of one call per environment; plans, Philox offsets and
        the augmented images are those of the per-environment loop, bit for bit.
        `full_state=True` (Agent): save() also writes the full learner state and load() restores it when it is there, so that an
        interrupted run continues bit for bit (save_state / load_state; without the keyword both behave as in the reference:
        weights and config.json, fresh optimizers).
        `joint_update=True` (PPOAgent; not in the reference): every minibatch step takes the policy loss and the value loss on ONE
        train-mode trunk forward and back-propagates their sum once (engine.joint_forward_backward / joint_apply) instead of running
        the trunk twice.  `dynamics_lr` then acts ONCE per minibatch -- the trunk's optimizer takes one step on the summed gradient
        where the default takes two -- and the trunk's moving statistics update once.  update() runs one minibatch loop of
        optimization_steps[0] passes over the policy batch pipeline (optimization_steps must be equal, else ValueError).
        `view_pipeline` (not in config.json): how learn_representation() makes its two views of a row.  'agent' (default): the
        rollout augmentation (draw_plans -> Augmenter.batch), pixel-aligned views.  'simclr': the SimCLR view pipeline -- random
        crop resized back, flip, colour jitter, colour drop, Gaussian blur (draw_view_plans -> Augmenter.views).
        A dict of draw_view_plans options (crop_scale, flip_prob, jitter_prob, drop_prob, blur_prob, blur_sigma) implies 'simclr'.
        An unknown name or option: ValueError.
        `demo_traces=dir` (PPOAgent; not in the reference): every policy minibatch keeps
        D = round(demo_fraction * batch_size) rows of the expert traces in `dir` behind its batch_size - D fresh rows, trained on the
        same trunk pass by `demo_weight` times the Beta log-likelihood of the expert's action (with_demonstrations, the engines'
        demo_forward_backward(_resample)); works with both policy losses; the value loop is unchanged."""
        assert aug_intensity >= 0.0
        if kwargs.get('replay_rollouts', 0) and resample_actions:
            raise ValueError('replay_rollouts > 0 needs the stored-action policy loss: the re-sampled loss (resample_actions=True, the '
                             'default) evaluates a fresh sample of the new policy and has no importance ratio against the policy '
                             'that collected a kept row; create the agent with resample_actions=False')
        if kwargs.get('replay_rollouts', 0) and self._process_group()[3]:
            raise RuntimeError('replay_rollouts > 0 runs on one GPU: the kept periods differ per rank in size, and every minibatch step '
                               'is a collective; create the data-parallel agents with replay_rollouts=0')
        self.view_pipeline, self.view_options = self.parse_view_pipeline(view_pipeline)
        network_spec = dict(kwargs.pop('network', {}))
        network_spec.setdefault('network', CARLANetwork)
        network_spec.setdefault('control_policy', self.DEFAULT_CONTROL)
        network_spec.setdefault('control_value', self.DEFAULT_CONTROL_VALUE)
        network_spec.setdefault('dynamics', self.DEFAULT_DYNAMICS)
        network_spec.setdefault('compute', compute)
        network_spec.setdefault('update_dynamics', update_dynamics)
        self.should_update_dynamics = update_dynamics
        self.dynamics_path = os.path.join(kwargs.get('weights_dir', 'weights'), name, 'dynamics_model')
        self.load_full = load_full
        head_clip = clip_norm if isinstance(clip_norm, float) or clip_norm is None else tuple(clip_norm[:2])
        super().__init__(*args, name=name, network=network_spec, clip_norm=head_clip, **kwargs)
        self.network: CARLANetwork = self.network
        self.aug_intensity = aug_intensity
        self.batch_augment = bool(batch_augment)
        self.delta, self.eta, self.aux = delta, eta, aux                  # stored, unused (as in the reference)
        self.resample_actions = resample_actions
        self._sample_offset = 0
        # the reference computes should_clip_dynamics_grads but never reads it: trunk grads are unclipped (F9)
        self.should_clip_dynamics_grads = isinstance(clip_norm, float) or (clip_norm is not None and len(clip_norm) > 2
                                                                          and isinstance(clip_norm[2], float))
        self.grad_norm_dynamics = float(clip_norm) if isinstance(clip_norm, float) else \
            (float(clip_norm[2]) if self.should_clip_dynamics_grads else 0.0)
        self.dynamics_lr = DynamicParameter.create(value=dynamics_lr)
        self.dynamics_lr.load(config=self.config.get('dynamics_lr', {}))
        self._augmenter = None
        self._aug_rng = np.random.default_rng(self.seed)
        self._aug_calls = 0
        self._shard, self._info_segments = [self.env], []
        self._init_data_parallel()
        self._constructed = True
        if self._pending_state_meta is not None:        # load=True with a full state: the host half waits for the fields above
            meta, self._pending_state_meta = self._pending_state_meta, None
            self.restore_host_state(meta)

    # -- data parallelism (reference loop rl/agents/ppo.py:190-226 inside :464-548) ------------------------------
    @staticmethod
    def _process_group() -> tuple:
        """-> (world size, rank, collectives forced at world size 1, data parallel) of the initialised process group, if any."""
        on = dist.is_available() and dist.is_initialized()
        world = dist.get_world_size() if on else 1
        force = on and os.environ.get('CDRL_FORCE_COLLECTIVES') == '1'
        return world, (dist.get_rank() if on else 0), force, world > 1 or force

    def _init_data_parallel(self):
        """One CARLAgent per GPU under torch.distributed: every rank rolls out ITS OWN environment shard (environment and
        rollout-sampler seeds offset by the rank), computes returns / GAE locally (per-episode quantities), runs the same
        number of minibatch steps on its shard with gradients pre-scaled by 1 / world, and the gradient arenas are SUM-
        all-reduced before the identical clip + Adam update (DataParallelLearner).  Parameters are broadcast from rank 0 here
        and after load(); BatchNorm moving statistics are averaged once per update().  Without an initialised process group
        (or at world size 1) nothing changes; CDRL_FORCE_COLLECTIVES=1 runs the collectives at world size 1 as well."""
        self.world, self.rank, force, self.data_parallel = self._process_group()
        self._dp = {}
        self._dp_force = force
        if not self.data_parallel:
            return
        self._dp_for(self.network.engine).broadcast_parameters()
        if self.rank:
            # rank-disjoint environment shard and action-sampling stream; weights stay identical (same init seed + broadcast)
            if self.seed is not None:
                self.env.seed(self.seed + self.rank)
            self._aug_rng = np.random.default_rng((self.seed or 0) + 7919 * self.rank)
        self.network.sample_rank, self.network.sample_stride = self.rank, self.world

    def _dp_for(self, eng) -> DataParallelLearner:
        """The DataParallelLearner of an engine (the main one, or a ragged-minibatch engine over the same arenas)."""
        dp = self._dp.get(id(eng))
        if dp is None:
            dp = self._dp[id(eng)] = DataParallelLearner(eng, force_collectives=self._dp_force)
        return dp

    def _all_reduce_ints(self, values, op):
        dev = self.device if dist.get_backend() == 'nccl' else 'cpu'
        t = torch.tensor(list(values), dtype=torch.int64, device=dev)
        dist.all_reduce(t, op=op)
        return [int(x) for x in t.tolist()]

    def agree_on_batches(self, policy_batches, value_batches):
        """Every minibatch step is a collective (the gradient all-reduce), so the NUMBER of steps is decided collectively and
        never from a rank's own list: all ranks run the minimum count of FULL minibatches (episodes that ended early on one rank
        drop the surplus minibatches of the others for this update), followed by ONE ragged step only if every rank holds exactly
        one ragged minibatch with the same row count.  The ragged minibatch is found by its row count, not by its position
        (with shuffle_batches it is not the last one), and is moved to the end of the list."""
        if not self.data_parallel:
            return policy_batches, value_batches

        def split(batches):
            full = [b for b in batches if int(b[1].shape[0]) == self.batch_size]
            ragged = [b for b in batches if int(b[1].shape[0]) != self.batch_size]
            # rows of THE ragged minibatch; 0 = none (or several: a pipeline this agent does not produce, never agreed on)
            return full, ragged, (int(ragged[0][1].shape[0]) if len(ragged) == 1 else 0)

        pf, pr, prow = split(policy_batches)
        vf, vr, vrow = split(value_batches)
        sig = [len(pf), len(vf), prow, vrow]
        lo = self._all_reduce_ints(sig, dist.ReduceOp.MIN)
        hi = self._all_reduce_ints(sig, dist.ReduceOp.MAX)
        policy_batches = pf[:lo[0]] + (pr if lo[2] > 0 and lo[2] == hi[2] else [])
        value_batches = vf[:lo[1]] + (vr if lo[3] > 0 and lo[3] == hi[3] else [])
        return policy_batches, value_batches

    def after_update(self):
        if self.data_parallel:
            self._dp_for(self.network.engine).sync_moving_statistics()

    def is_writer(self) -> bool:
        # every rank runs learn() to its end: checkpoints, summaries and traces are written by rank 0 alone
        return not self.data_parallel or self.rank == 0

    def rank_barrier(self, failed: bool = False):
        if not self.data_parallel:
            return
        # the meeting point doubles as a status exchange: MAX over the ranks' failure flags, so that a writer whose save() raised
        # takes every rank down with an error instead of leaving them in a barrier until the process-group timeout
        flag = torch.tensor([1.0 if failed else 0.0], device=self.device if dist.get_backend() == 'nccl' else 'cpu')
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if float(flag.item()) > 0.0 and not failed:
            raise RuntimeError('data-parallel learn(): the writer rank failed to save the checkpoint (see its traceback)')

    def load(self):
        super().load()
        if getattr(self, 'data_parallel', False):       # (load=True in the constructor runs before _init_data_parallel, which broadcasts itself)
            self._dp_for(self.network.engine).broadcast_parameters()

    # -- full state ----------------------------------------------------------------------------------------------------
    def state_rank(self):
        return self.rank if self.data_parallel else None

    def host_state(self) -> dict:
        """Agent.host_state plus this class's: the re-sampling Philox offset `_sample_offset`, the augmentation plan counter
        `_aug_calls` and generator `_aug_rng`, and the rollout sampler's `action_index` / `sample_seed` (they live in the network
        and differ per rank under data parallelism).  Generators saved in all: `rng`, `_aug_rng`, global `numpy.random`, global
        `random`; the device samplers are counter-based (seed + offset) and have no other state."""
        state = super().host_state()
        state.update(sample_offset=int(self._sample_offset), aug_calls=int(self._aug_calls), aug_rng=self._aug_rng.bit_generator.state,
                     action_index=int(self.network.action_index), sample_seed=int(self.network.sample_seed))
        return state

    def set_host_state(self, state: dict):
        super().set_host_state(state)
        self._sample_offset = int(state['sample_offset'])
        self._aug_calls = int(state['aug_calls'])
        self._aug_rng.bit_generator.state = state['aug_rng']
        self.network.action_index = int(state['action_index'])
        self.network.sample_seed = int(state['sample_seed'])

    def restore_host_state(self, meta: dict):
        if not self._constructed:
            self._pending_state_meta = meta
            return
        super().restore_host_state(meta)

    def hyper_parameters(self) -> dict:
        hp = super().hyper_parameters()
        hp['dynamics_lr'] = self.dynamics_lr()
        hp['clip_norm_dynamics'] = self.grad_norm_dynamics       # read by the engines in clip_mode='global' only
        return hp

    # -- update -----------------------------------------------------------------------------------
    def update(self):
        small = len(self.memory) < self.batch_size
        if self.data_parallel:      # a collective decision: one rank skipping alone would leave the others in an all-reduce
            small = bool(self._all_reduce_ints([int(small)], dist.ReduceOp.MAX)[0])
        if small:
            print('[Not updated] memory too small!')
            self._reset_info()
            self.discard_period()
            return
        super().update()
        if self.statistics.mode is not None:        # (reference core/carla_agent.py:137-140)
            kw = train_stats.action_entries(self.memory.actions)
            if kw is None:
                print('[update] unable to print actions')
            else:
                self.log(**kw)
        self._reset_info()

    def _reset_info(self):
        for env in self._shard:
            env.reset_info()
        self._info_segments = []

    def collect(self, shard, *args, **kwargs):
        self._shard = shard
        return super().collect(shard, *args, **kwargs)

    def trajectory_stored(self, env_index, rollout, segment=None):
        super().trajectory_stored(env_index, rollout, segment)
        # several environments: remember which slice of WHICH environment's info buffer belongs to the rows just appended
        if len(self._shard) > 1:
            have = len(self._shard[env_index].info_buffer['speed'])
            if segment is not None:
                # auto-reset: one of several trajectories of the environment -- it starts `env_steps_at_start` entries (environment
                # steps, repeated actions included) behind what the buffer held before this rollout
                start, stop, _, env_steps_at_start = segment
                self._info_segments.append((env_index, have - rollout.env_steps[env_index] + env_steps_at_start, stop - start))
                return
            self._info_segments.append((env_index, have - rollout.env_steps[env_index], rollout.length[env_index]))

    def _info(self, n):
        """speed / similarity targets of the auxiliary heads, one per memory row, from the environments' info buffers
        (reference core/carla_agent.py:328-329,341-347: padded / truncated to the number of rows).  With an environment shard
        the buffers are cut per trajectory, in the order the trajectories were appended."""
        if self._info_segments:
            sp, si = [], []
            for e, start, rows in self._info_segments:
                buf = self._shard[e].info_buffer
                for dst, key in ((sp, 'speed'), (si, 'similarity')):
                    piece = np.asarray(buf[key][start:start + rows], dtype=np.float32)
                    dst.append(np.pad(piece, (0, rows - piece.shape[0])))
            speed_h, sim_h = np.concatenate(sp), np.concatenate(si)
        else:
            speed_h = np.asarray(self.env.info_buffer['speed'], dtype=np.float32)
            sim_h = np.asarray(self.env.info_buffer['similarity'], dtype=np.float32)
        speed = torch.as_tensor(speed_h, device=self.device) / 100.0
        sim = torch.as_tensor(sim_h, device=self.device)
        if speed.shape[0] >= n:
            return speed[:n].contiguous(), sim[:n].contiguous()
        pad = torch.zeros(n - speed.shape[0], device=self.device)
        return torch.cat([speed, pad]), torch.cat([sim, pad])

    def _info_with_replay(self, n):
        """`_info` for the fresh rows among the `n` rows of a batch component, followed by the kept periods' own targets (the rows
        behind the fresh ones when the running update() reuses kept periods; PPOAgent.with_replay)."""
        speed, similarity = self._info(n - sum(p.rows for p in self._replay_active))
        return self.with_replay(speed, 'speed'), self.with_replay(similarity, 'similarity')

    def replay_info(self, rows):
        speed, similarity = self._info(rows)
        return dict(speed=speed, similarity=similarity)

    def policy_batch_tensors(self):
        states, advantages, actions, log_probabilities = super().policy_batch_tensors()
        speed, similarity = self._info_with_replay(advantages.shape[0])
        if self._trust_anchor is not None:      # target_kl / kl_penalty: the anchor rides along as a seventh component
            return states, advantages, actions, log_probabilities, speed, similarity, self._trust_anchor
        return states, advantages, actions, log_probabilities, speed, similarity

    def value_batch_tensors(self):
        states, returns = super().value_batch_tensors()
        speed, similarity = self._info_with_replay(returns.shape[0])
        return states, returns, speed, similarity

    def _policy_pass(self, kind, batch, **extra):
        """The `kind` ('policy' / 'joint') pass on a policy batch (+ extra tensors), staged under that name; returns the engine."""
        states, advantages, actions, log_probabilities, speed, similarity, *anchor = batch
        if anchor:
            extra = dict(extra, anchor=anchor[0])
        eng = self._step_engine = self.network.engine_for(advantages.shape[0])
        b = dict(states={k: states[k] for k in ('state_image', 'state_road', 'state_vehicle', 'state_navigation')},
                 advantages=advantages, old_log_prob=log_probabilities, speed=speed, similarity=similarity, u=actions, **extra)
        b = eng.stage(b, kind)               # fixed addresses -> the captured hipGraph of the step is replayed
        b.update(du_da=None, du_db=None)
        if kind == 'demo' and getattr(eng, '_demo_block', None) is not self._demo_block:
            eng.set_demo_block(self._demo_block)        # (engines of every minibatch size add to the update()'s one block)
        scale = 1.0 / self.world
        if self.resample_actions:
            # Beta(alpha, beta) of the NEW policy is sampled on the device with pathwise Jacobians (rank-disjoint Philox offsets)
            self._sample_offset += 1
            getattr(eng, f'{kind}_forward_backward_resample')(b, seed=self.seed if self.seed is not None else 0,
                                                              offset=self._sample_offset * self.world + self.rank, grad_scale=scale)
        else:
            getattr(eng, f'{kind}_forward_backward')(b, grad_scale=scale)
        return eng

    def with_demonstrations(self, batch):
        """A policy minibatch of n fresh rows -> (the six components with D demonstration rows behind the fresh ones, dict(demo_u,
        demo_w)) for the mixed pass.  Fresh rows carry demo_w = 0; demonstration rows carry this update()'s weight, their trace's
        speed / similarity targets, and zeros where the mixed loss reads nothing (advantages, stored log-probabilities)."""
        states, advantages, actions, log_probabilities, speed, similarity = batch
        d = self.draw_demonstrations()
        n, D = int(advantages.shape[0]), self.demo_rows_per_batch
        zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=advantages.device)
        cat = lambda a, b: torch.cat([a, b], dim=0)
        mixed = ({k: cat(states[k], d['states'][k]) for k in self.STATE_KEYS}, cat(advantages, zeros(D)), cat(actions, d['u']),
                 cat(log_probabilities, zeros(D, self.num_actions)), cat(speed, d['speed']), cat(similarity, d['similarity']))
        weight = torch.full((D,), self._demo_w, dtype=torch.float32, device=advantages.device)
        return mixed, dict(demo_u=cat(zeros(n, self.num_actions), d['u']), demo_w=cat(zeros(n), weight))

    def get_policy_gradients(self, batch):
        if self._demo_active:       # (batch, extras) of with_demonstrations
            eng = self._policy_pass('demo', batch[0], **batch[1])
            return eng.buffer(2)[0].clone(), 'policy'
        eng = self._policy_pass('policy', batch)
        if self.data_parallel:
            self._dp_for(eng).reduce_policy_gradients()
        return eng.buffer(2)[0].clone(), 'policy'  # device scalar (copy of CDRL_BUF_METRICS_P[0]); gradients stay in the arena

    def apply_policy_gradients(self, gradients):
        self._step_engine.policy_apply()          # trunk Adam (not when frozen) -> clip -> old_policy <- policy -> policy Adam
        return gradients

    def get_value_gradients(self, batch):
        states, returns, speed, similarity = batch
        eng = self._step_engine = self.network.engine_for(returns.shape[0])
        b = dict(states={k: states[k] for k in ('state_image', 'state_road', 'state_vehicle', 'state_navigation')},
                 returns=returns, speed=speed, similarity=similarity)
        eng.value_forward_backward(eng.stage(b, 'value'), grad_scale=1.0 / self.world)
        if self.data_parallel:
            self._dp_for(eng).reduce_value_gradients()
        return eng.buffer(3)[0].clone(), 'value'

    def apply_value_gradients(self, gradients):
        self._step_engine.value_apply()
        return gradients

    def get_joint_gradients(self, batch):
        *policy_batch, returns = batch
        eng = self._policy_pass('joint', policy_batch, returns=returns)
        if self.data_parallel:
            self._dp_for(eng).reduce_joint_gradients()
        return (eng.buffer(2)[0].clone(), eng.buffer(3)[0].clone()), 'joint'

    def apply_joint_gradients(self, gradients):
        self._step_engine.joint_apply()     # trunk step ONCE (not when frozen) -> old_policy <- policy -> policy head -> value head
        return gradients

    # -- imitation (PPOAgent.imitate) ----------------------------------------------------
    STATE_KEYS = ('state_image', 'state_road', 'state_vehicle', 'state_navigation')

    def imitation_state_keys(self) -> list:
        return list(self.STATE_KEYS)

    def stacks_time(self) -> bool:
        return True

    def clone_minibatch(self, batch, policy_weight, value_weight, aux_weight):
        eng = self.network.engine_for(batch['u'].shape[0])          # (a ragged last minibatch: its own engine, as in update())
        b = dict(batch, states={k: batch['states'][k] for k in self.STATE_KEYS})
        eng.clone_step(eng.stage(b, 'clone'), policy_weight, value_weight, aux_weight)
        return eng

    # -- held-out traces: scoring and validation -------------------------------------------------------
    def score_traces(self, traces_dir=None, *, max_traces=None, chunk=None, value=True, aux=True, per_trace=False) -> dict:
        """How well the ACTING network (old_policy, moving statistics: what predict() runs) fits expert traces, e.g. ones it was not
        trained on.  The files are read in sorted order (no generator draw), each is checked and uploaded once like imitate() does
        (returns with the agent's gamma), and goes through inference forwards of `chunk` rows (default batch_size) with one
        cdrl_beta_score launch per chunk; ONE block and one host read for the whole call (per_trace: one block per trace, read
        together at the end and returned under 'traces', the totals being their sums).
        -> engine.read_score_block's dict: rows, log_prob, mode_error, bias, rmse, predicted_std, entropy (each also `_per_action`),
        pit_histogram, coverage_50 / coverage_90 per action, value_bias / value_rmse / explained_variance, speed_rmse /
        similarity_rmse, nonfinite, pit_unconverged, block.  value / aux: score the value head against the returns / the auxiliary
        heads against info_speed (km/h, / 100 as in training) and info_similarity; switched off with one printed line for traces
        that lack `reward` / `info_*` (the figures are then None).
        Not touched: parameters, moving statistics, optimizer state, memories, the sampler's stream; nothing is logged.
        traces_dir may be a TraceSet (load_trace_set) in place of the directory: the same sweep over the set's traces in their sorted
        order, every trace's tensors made by one launch instead of read from its file; the same blocks, bit for bit.
        RuntimeError under data parallelism; ValueError: no traces directory, no trace file in it, chunk outside 1..65535, a trace
        that does not fit the agent (_check_trace), a trace set that does not."""
        if getattr(self, 'data_parallel', False):
            raise RuntimeError('score_traces() runs on one GPU: score in a single process (save(), and load the weights there), not '
                               'in the data-parallel run')
        path, trace_set, _ = self._trace_source(traces_dir, False, 'score_traces')
        chunk = self.batch_size if chunk is None else chunk
        if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or not 1 <= chunk <= 65535:
            raise ValueError(f'score_traces: chunk = {chunk}: 1 to 65535 rows per forward')
        if trace_set is None and not traces.trace_files(path):
            raise ValueError(f'score_traces: no trace-*.npz file in {path}')
        A, chunk = self.num_actions, int(chunk)
        total = None if per_trace else score_block(A, self.device)
        blocks, told = [], set()
        if trace_set is None:
            source = traces.load_traces(path, max_amount=max_traces, shuffle=False)
        else:
            path = trace_set.dir
            source = range(trace_set.traces if max_traces is None else min(trace_set.traces, int(max_traces)))
        for trace in source:
            if trace_set is None:
                with_value = bool(value) and 'reward' in trace
                with_aux = bool(aux) and 'info_speed' in trace and 'info_similarity' in trace
            else:
                with_value, with_aux = bool(value) and trace_set.has_value, bool(aux) and trace_set.has_info
            for asked, given, lacks, what in ((value, with_value, 'reward', 'the value head'),
                                              (aux, with_aux, 'info_speed / info_similarity', 'the auxiliary heads')):
                if asked and not given and what not in told:
                    told.add(what)
                    print(f'score_traces: a trace in {path} has no {lacks}: {what} are not scored on it')
            if trace_set is None:
                data = self._trace_tensors(trace, None, with_aux, 1.0 if with_value else 0.0)
            else:
                data = trace_set.trace_tensors(trace, ('u',) + (('speed', 'similarity') if with_aux else ()) +
                                               (('returns',) if with_value else ()), self.gamma)
            block = score_block(A, self.device) if per_trace else total
            self.network.score_rows(data['states'], data['u'], data.get('returns'), data.get('speed'), data.get('similarity'),
                                    chunk=chunk, block=block)
            blocks.append(block)
        if not per_trace:
            return read_score_block(total, A)
        each = read_score_block(torch.stack(blocks), A)
        out = read_score_block(torch.as_tensor(np.sum([t['block'] for t in each], axis=0)), A)
        out['traces'] = each
        return out

    def imitate(self, *args, validation_dir=None, validation_every=1, patience=None, validation_set=None, trace_set=None,
                mix_traces=False, **kw):
        """PPOAgent.imitate (same arguments) with validation on held-out traces: with `validation_dir`, behind every
        `validation_every`-th epoch the acting network is brought up to date (update_old_policy()) and scored on that directory
        (score_traces); logged: validation_log_prob, validation_mode_error, validation_rmse, validation_coverage_90 (the mean over
        the actions) and, with returns, validation_value_rmse.  patience=k ends the run after k validations in a row without a new
        best validation_log_prob (one printed line); the weights stay those of the last epoch.  The defaults are imitate() as it
        was: no launch more.  With polyak == 1 the validations do not change what imitate() leaves: the clone pass never reads
        the old policy and the final update_old_policy() overwrites it.  With polyak < 1 every update_old_policy() averages, so
        validating would change the result: ValueError.  ValueError also for patience without validation_dir.
        Device-resident trace sets (load_trace_set): trace_set= names the set to learn from instead of traces_dir,
        mix_traces=True asks for minibatches mixed over the whole set (PPOAgent.imitate's traces_dir=set and shuffle_data='set'),
        validation_set= the held-out set instead of validation_dir -- no file is read during the run.  ValueError when a set and
        its directory are both given, or mix_traces without trace_set."""
        if trace_set is not None:
            if kw.get('traces_dir') is not None:
                raise ValueError('imitate(): pass traces_dir or trace_set, not both')
            kw['traces_dir'] = trace_set
        if mix_traces:
            if trace_set is None:
                raise ValueError('imitate(mix_traces=True) draws minibatches across traces: it needs trace_set=')
            kw['shuffle_data'] = 'set'
        if validation_dir is not None and validation_set is not None:
            raise ValueError('imitate(): pass validation_dir or validation_set, not both')
        validation_dir = validation_set if validation_set is not None else validation_dir
        if validation_dir is None:
            if patience is not None:
                raise ValueError(f'imitate(patience={patience}) without validation_dir: early stopping needs held-out traces to score')
            return super().imitate(*args, **kw)
        if float(self.polyak_coeff) < 1.0:
            raise ValueError(f'imitate(validation_dir=...): the agent was created with polyak={self.polyak_coeff}; every validation '
                             f'calls update_old_policy(), which with polyak < 1 averages the old policy once more and so changes '
                             f'what imitate() leaves; validate with score_traces() after the run instead')
        if isinstance(validation_every, bool) or not isinstance(validation_every, (int, np.integer)) or validation_every < 1:
            raise ValueError(f'imitate(validation_every={validation_every}): a number of epochs, at least 1')
        if patience is not None and (isinstance(patience, bool) or not isinstance(patience, (int, np.integer)) or patience < 1):
            raise ValueError(f'imitate(patience={patience}): a number of validations, at least 1 (or None)')
        self._validation = dict(dir=validation_dir, every=int(validation_every), patience=patience, best=-np.inf, stale=0)
        try:
            return super().imitate(*args, **kw)
        finally:
            self._validation = None

    _validation = None          # the run in flight of imitate(validation_dir=...)

    def imitation_epoch_end(self, epoch: int) -> bool:
        v = self._validation
        if v is None or epoch % v['every']:
            return False
        self.network.update_old_policy()
        s = self.score_traces(v['dir'])
        entry = dict(validation_log_prob=s['log_prob'], validation_mode_error=s['mode_error'], validation_rmse=s['rmse'],
                     validation_coverage_90=float(np.mean(s['coverage_90'])))
        if s['value_rmse'] is not None:
            entry['validation_value_rmse'] = s['value_rmse']
        self.log(**entry)
        self.write_summaries()
        if v['patience'] is None:
            return False
        if s['log_prob'] > v['best']:
            v['best'], v['stale'] = s['log_prob'], 0
            return False
        v['stale'] += 1
        if v['stale'] < v['patience']:
            return False
        print(f"[{epoch}] imitate: no new best validation_log_prob ({v['best']:.6g}) in {v['stale']} validation(s): stopping")
        return True

    def imitation_learning(self, alpha=0.5, beta=0.5, clip_grad=1.0, lr=1e-3, polyak=None, epochs=1, shuffle_data=True,
                           traces_dir=None, **kw):
        """The supervised stage of the reference's curriculum (Stage.imitation_learning, core/learning.py:180-181, calls this name
        with these keywords; the reference never defines it): imitate() with alpha as the policy weight, beta as the value weight,
        clip_grad as every optimizer's clip threshold and lr as every optimizer's learning rate; every other keyword of imitate()
        (validation_dir, validation_every, patience among them) goes through.  polyak: fixed when the learner
        engines are created (CARLAgent(polyak=...)), so any other value is refused."""
        if polyak is not None and float(polyak) != float(self.polyak_coeff):
            raise ValueError(f'imitation_learning(polyak={polyak}): the agent was created with polyak={self.polyak_coeff}, which its '
                             f'learner engines are built with; create the agent with CARLAgent(polyak={polyak}) instead')
        return self.imitate(epochs=epochs, shuffle_data=shuffle_data, traces_dir=traces_dir, policy_weight=alpha, value_weight=beta,
                            clip_norm=clip_grad, lr=lr, **kw)

    # -- contrastive pre-training of the trunk ----------------------------------------------------------
    VECTOR_KEYS = ('state_road', 'state_vehicle', 'state_navigation')
    REPRESENTATION_LOG = ('representation_loss', 'representation_accuracy', 'representation_similarity_pos',
                          'representation_similarity_neg', 'representation_embedding_norm')

    view_pipeline, view_options = 'agent', {}       # class-level defaults: an agent that never ran __init__ has the old views

    @staticmethod
    def parse_view_pipeline(value) -> tuple:
        """CARLAgent(view_pipeline=...) -> (name, options of draw_view_plans)."""
        from ..rl.augmentations import check_view_options
        if isinstance(value, dict):
            check_view_options(**value)
            return 'simclr', dict(value)
        if value in ('agent', 'simclr'):
            return value, {}
        raise ValueError(f"view_pipeline must be 'agent', 'simclr' or a dict of draw_view_plans options, got {value!r}")

    def representation_views(self, rows: dict, plans, vector_inputs='zero') -> dict:
        """The two views of N observation rows as one batch of 2N, the vector inputs zeroed ('zero') or passed through ('keep').
        plans, a list (view_pipeline 'agent'): the rows stacked twice, all 2N image stacks augmented by ONE Augmenter.batch call with
        `plans` (2N of them; empty = no augmentation, as preprocess() at intensity 0).  plans, a record array of view plans
        ('simclr'): ONE Augmenter.views call makes the 2N image stacks from the N rows, which are not stacked twice."""
        if vector_inputs not in ('zero', 'keep'):
            raise ValueError(f"vector_inputs must be 'zero' or 'keep', got {vector_inputs!r}")
        if (isinstance(plans, np.ndarray) or plans) and self._augmenter is None:
            from ..rl.augmentations import Augmenter
            self._augmenter = Augmenter(self.device)
        twice = lambda k: torch.cat([rows[k], rows[k]], dim=0)
        if isinstance(plans, np.ndarray):
            views = {k: self._augmenter.views(rows[k], plans) if k == 'state_image' else twice(k) for k in self.STATE_KEYS}
        else:
            views = {k: twice(k) for k in self.STATE_KEYS}
            if plans:
                views['state_image'] = self._augmenter.batch(views['state_image'], plans)
        if vector_inputs == 'zero':
            for k in self.VECTOR_KEYS:
                views[k] = torch.zeros_like(views[k])
        return views

    def representation_plans(self, intensity: float, rng: np.random.Generator, count: int, first_offset: int) -> list:
        """The augmentation plans of one minibatch's views: `count` draws from the call's own generator with consecutive Philox
        offsets (draw_plans, as the shard path of preprocess()); none at intensity 0.  With view_pipeline 'simclr': `count` view
        plans as one record array (draw_view_plans with strength = intensity and the agent's view options; first_offset is unused,
        view plans carry no random stream)."""
        if intensity <= 0.0:
            return []
        if self.view_pipeline == 'simclr':
            from ..rl.augmentations import draw_view_plans
            H, W = self.state_spec['state_image'][-3:-1]
            return draw_view_plans(float(intensity), rng, count, H, W, **self.view_options)
        from ..rl.augmentations import draw_plans
        return draw_plans(float(intensity), rng, count, first_offset=first_offset)

    def representation_minibatch(self, views: dict, temperature: float):
        """One representation step (pass + trunk apply) on a batch of views.  -> the learner engine that ran it."""
        eng = self.network.engine_for(views['state_image'].shape[0])
        eng.repr_step(eng.stage(views, 'representation'), temperature)
        return eng

    def learn_representation(self, epochs=1, batch_size=None, *, traces_dir=None, temperature=0.1, intensity=1.0,
                             vector_inputs='zero', lr=None, shuffle_data=True, max_traces=None, seed=None, close=False):
        """The representation stage of the reference's curriculum (Stage.representation_learning calls this name with its
        `representation` keywords; the reference never defines it): contrastive pre-training of the shared trunk on the states of
        `trace-*.npz` files (imitate()'s data source; actions, rewards and infos are not read).  Objective: NT-Xent (SimCLR, the
        loss rl/augmentations/simclr.py of the reference points to) on the trunk's output, no projection head.
        Each minibatch takes batch_size / 2 rows of one trace, stacks them twice, augments all image stacks with independently drawn
        plans of `intensity`, and takes one trunk-only step (engine.repr_step); a remainder is dropped, a trace with fewer usable
        rows is skipped.  vector_inputs='zero' feeds zeros for road / vehicle / navigation -- they are bit-identical in both views
        and would give the pair away -- 'keep' passes them through.  lr: dynamics_lr during the run (the agent's own comes back
        afterwards, also after an error).  seed: seeds the call's plan / shuffle generator; None: one draw from self.rng.
        Only self.rng advances (that draw and the trace order): the rollout sampler, the re-sampling offset and the rollout
        augmentation's generator and counter stay where they are.  No head changes, so old_policy is not touched.
        traces_dir may be a TraceSet (load_trace_set) in place of the directory: the same loop, every trace's states made from the
        device-resident set by one launch -- the same order, draws and bits.  With a set, shuffle_data='set' mixes the traces: per
        epoch one true permutation of the set's rows from the call's generator, uploaded once; every minibatch's batch_size / 2
        rows come from all traces."""
        if getattr(self, 'data_parallel', False):
            raise RuntimeError('learn_representation() runs on one GPU: pre-train in a single process, save(), and load the weights '
                               'in the data-parallel run')
        if not self.should_update_dynamics:
            raise ValueError('learn_representation() trains the trunk: the agent was created with update_dynamics=False')
        if self.clip_mode == 'global' or self.skip_nonfinite:
            raise ValueError("learn_representation(): the gradient gate (clip_mode='global' / skip_nonfinite=True) is per head and has "
                             'no trunk-only step; pre-train with an agent created without it')
        if vector_inputs not in ('zero', 'keep'):
            raise ValueError(f"vector_inputs must be 'zero' or 'keep', got {vector_inputs!r}")
        batch_size = self.batch_size if batch_size is None else int(batch_size)
        if batch_size < 2 or batch_size % 2:
            raise ValueError(f'learn_representation(batch_size={batch_size}): a batch is two views of batch_size / 2 rows, so it '
                             f'must be even')
        if not float(temperature) > 0.0:
            raise ValueError(f'learn_representation(temperature={temperature}) must be positive')
        path, trace_set, mix_traces = self._trace_source(traces_dir, shuffle_data, 'learn_representation')
        if mix_traces and max_traces is not None:
            raise ValueError(f"learn_representation(shuffle_data='set', max_traces={max_traces}): max_traces is a per-trajectory "
                             f'notion; a mixed minibatch has no trajectory (load the set with max_traces instead)')
        rng_local = np.random.default_rng(int(self.rng.integers(2 ** 63 - 1)) if seed is None else int(seed))
        half, calls = batch_size // 2, 0
        base = self.hyper_parameters()
        run = dict(base) if lr is None else dict(base, dynamics_lr=float(lr))

        def step(rows, kept):
            nonlocal calls
            plans = self.representation_plans(intensity, rng_local, 2 * half, calls + 1)
            calls += 2 * half
            eng = self.representation_minibatch(self.representation_views(rows, plans, vector_inputs), float(temperature))
            kept.append(eng.buffer(_lib.BUF_METRICS_R)[:5].clone())      # copies stay on the device

        def trace_states():
            """One epoch's traces in an order drawn from self.rng: per trace a callable -> (rows, its states on the device)."""
            def from_file(trace):
                n = self._check_trace_states(trace)
                return n, self._trace_states(trace, n)
            if trace_set is None:
                for trace in traces.load_traces(path, max_amount=max_traces, shuffle=True, rng=self.rng):
                    yield lambda trace=trace: from_file(trace)
                return
            for j in trace_set.epoch_order(self.rng, max_traces):
                yield lambda j=j: (trace_set.trace_rows(j)[1], trace_set.trace_states(j))

        try:
            self.network.set_hparams(**run)
            for epoch in range(1, epochs + 1):
                if mix_traces:      # one true permutation of the set's rows per epoch, uploaded once; a ragged tail is dropped
                    t0 = time.time()
                    order, cuts = trace_set.plan_epoch(rng_local, half, True)
                    index, kept = trace_set.upload_index(order), []
                    for offset, rows in cuts:
                        step(trace_set.batch(index, offset, rows, ())['states'], kept)
                    if kept:        # ONE device-to-host copy per epoch
                        for m in torch.stack(kept).cpu().numpy():
                            self.log(**{k: float(m[j]) for j, k in enumerate(self.REPRESENTATION_LOG)})
                    self.write_summaries()
                    print(f'[{epoch}] {len(cuts)} mixed minibatches took {round(time.time() - t0, 3)}s.')
                for i, load in enumerate(() if mix_traces else trace_states()):
                    t0 = time.time()
                    n, states = load()
                    batches = utils.data_to_batches((states,), batch_size=half, shuffle=shuffle_data, seed=int(rng_local.integers(2 ** 31)),
                                                    skip=self.skip_count, num_shards=self.obs_skipping, drop_remainder=True)
                    kept = []
                    for (rows,) in batches:
                        step(rows, kept)
                    if not kept:
                        print(f'[{epoch}] Trace-{i} skipped: {n} rows give no full minibatch of {half}.')
                        continue
                    for m in torch.stack(kept).cpu().numpy():       # ONE device-to-host copy per trace
                        self.log(**{k: float(m[j]) for j, k in enumerate(self.REPRESENTATION_LOG)})
                    self.write_summaries()
                    print(f'[{epoch}] Trace-{i} took {round(time.time() - t0, 3)}s.')
        finally:
            self.network.set_hparams(**base)
            if close:
                self.env.close()

    # -- rollout helpers ------------------------------------------------------------------------------
    def get_memory(self):
        return CARLAMemory(state_spec=self.state_spec, num_actions=self.num_actions, time_horizon=self.env.time_horizon,
                           device=self.device)

    def preprocess(self):
        """Stacks a list of T per-step observation dicts (real CARLAEnv) or passes a dict of (T, ...)
        arrays through, prefixing keys with 'state_' when needed."""
        def prepare(state):
            if isinstance(state, (list, tuple)):
                keys = state[0].keys()
                state = {k: np.stack([np.asarray(s[k], dtype=np.float32) for s in state], axis=0) for k in keys}
            return {(k if k.startswith('state_') else f'state_{k}'): v for k, v in state.items()}

        alpha = self.aug_intensity
        if alpha <= 0.0:
            return prepare

        from ..rl.augmentations import Augmenter, draw_plan, draw_plans

        def augment_fn(state):
            """CARLAgent.augment (core/carla_agent.py:527-579): the image stack of every observation is augmented with
            probability-gated ops of intensity `aug_intensity`, on the device."""
            state = prepare(state)
            if self._augmenter is None:
                self._augmenter = Augmenter(self.device)
            self._aug_calls += 1
            plan = draw_plan(alpha, self._aug_rng, offset=self._aug_calls)
            state['state_image'] = self._augmenter(state['state_image'], plan)
            return state

        def augment_shard(states):
            """`augment_fn` for the E observations of an environment shard at once: one host array and one copy per key, the E plans
            drawn in environment order from the same generator with the same offsets as E augment_fn calls, one batched
            augmentation call."""
            states = [prepare(s) for s in states]
            if self._augmenter is None:
                self._augmenter = Augmenter(self.device)
            plans = draw_plans(alpha, self._aug_rng, len(states), first_offset=self._aug_calls + 1)
            self._aug_calls += len(states)
            out = {}
            for k in states[0]:
                vals = [np.asarray(s[k], dtype=np.float32) for s in states]
                if k == 'state_image':
                    out[k] = self._augmenter.batch(vals, plans)     # gathered into the augmenter's page-locked staging buffer
                else:
                    out[k] = torch.as_tensor(np.stack(vals, axis=0)).to(self.device)
            return out

        if self.batch_augment:
            augment_fn.shard = augment_shard
        return augment_fn

    def evaluate(self, name: str, timesteps: int, trials: int, seeds=None, town='Town03', initial_seed=None, close=False,
                 envs=None, deterministic=False) -> dict:
        """Scores the agent over `trials` trials of at most `timesteps` steps and writes the record -- per result key the list over
        the trials, `<key>_mean` and `<key>_std` -- to `<evaluation_path>/<name>.json`; returns the result lists (collision_rate,
        similarity, waypoint_distance, speed, total_reward, timesteps).  Semantics of the reference (core/carla_agent.py:205-321):
        `initial_seed` goes to set_random_seed, `set_town(town)` is called on environments that have it, the augmentation is off
        for the duration (`aug_intensity` is restored in any case), every trial has its own seed (evaluation.trial_seed), a step is
        predict -> convert_action -> `repeat_action` environment steps (rewards summed, stopped at `done`), the driving metrics
        are read after it (evaluation.evaluation_info), and a trial is recorded when `(done or t == timesteps) and t > 32` -- an
        environment that reports `done` at t <= 32 is stepped on, as the reference does, and `timesteps <= 32`, where the
        reference would never finish, raises ValueError.  `total_reward` is floored at -1000.  Per trial the `eval_*` scalars are
        logged and write_summaries() runs.  `close=True` closes the environments.

        What differs from the reference:
          * `envs` (default `[self.env]`): trials run in WAVES of E = len(envs).  Wave w runs trials w*E .. min((w+1)*E, trials) - 1
            on the first n <= E environments, stepped in lockstep: one observe() and one network.evaluate_step() -- one inference
            forward of the n-environment engine plus one cdrl_beta_act launch -- per step.  An environment whose trial is recorded
            becomes inactive: it keeps its last observation in the batch, is stepped no more and its `active` entry is cleared.
          * seeds: with one environment the trial's seed goes through set_random_seed, as in the reference (which seeds `self.env`;
            a single environment passed in `envs` that is another object gets `env.seed(seed)` as well); with several,
            set_random_seed gets the wave's first seed and every trial's environment gets `env.seed(its seed)`.
          * `deterministic=True` acts with the mode of the Beta policy instead of a sample, and consumes no sampler offset.
          * nothing is appended to a memory (the reference fills one and deletes it); `data_for_dynamics` is a pass-through here.
          * `eval_actions / eval_distribution_mean / eval_distribution_std` are logged once per trial, not once per step: each is
            the mean over the trial's steps and action dimensions, taken from the running sums cdrl_beta_act keeps on the device
            (read once per wave); `eval_values` (the mean value estimate, from the same block) is logged beside them, and
            `eval_rewards` is the trial's mean step reward.  Per step ONE device-to-host copy is made: the actions.
          * the environments' info buffers (`reset_info`, where an environment has it) are emptied at the end, so that the steps
            taken here never reach the auxiliary targets of a following update().
          * no collectives: under data parallelism every rank evaluates on its own and only `is_writer()` writes the JSON file
            and the summaries.
        Parameters, moving statistics, optimizer slots and step counters are not touched."""
        assert trials > 0
        if timesteps <= 32:
            raise ValueError(f'evaluate: timesteps = {timesteps}: a trial is only recorded at t > 32, so this would never finish')
        shard = list(envs) if envs is not None else [self.env]
        E, A = len(shard), self.num_actions
        if isinstance(initial_seed, int):
            self.set_random_seed(seed=initial_seed)
        if town is not None:
            for env in shard:
                if hasattr(env, 'set_town'):
                    env.set_town(town)
        results = {k: [] for k in RESULT_KEYS}
        save_path = os.path.join(self.evaluation_path, f'{name}.json')
        print(save_path)
        aug_intensity = self.aug_intensity
        self.aug_intensity = 0.0            # no data augmentation
        try:
            for first in range(0, trials, E):
                n = min(E, trials - first)
                wave = shard[:n]
                wave_seeds = [trial_seed(seeds, trials, first + i) for i in range(n)]
                if wave_seeds[0] is not None:
                    self.set_random_seed(seed=wave_seeds[0])
                for env, seed in zip(wave, wave_seeds):
                    if seed is not None and (E > 1 or env is not self.env):      # (set_random_seed seeds self.env alone)
                        env.seed(seed)
                preprocess_fn = self.preprocess()
                self.reset()
                observations = [env.reset() for env in wave]
                t0 = time.time()
                stats = torch.zeros((n, act_stats_width(A)), dtype=torch.float64, device=self.device)
                mask, active = [1] * n, None           # (null = every row active, until the first trial of the wave is recorded)
                running = list(range(n))
                total, step_rewards, steps, collided = [0.0] * n, [0.0] * n, [0] * n, [False] * n
                metrics = [[0.0, 0.0, 0.0] for _ in range(n)]          # similarity, speed, waypoint distance: sums over the steps
                batch = self.observe(observations, preprocess_fn)
                for t in range(1, timesteps + 1):
                    action, _ = self.network.evaluate_step(batch, deterministic, active=active, stats=stats)
                    env_actions = np.atleast_2d(self.convert_action(action))
                    recorded = False
                    for e in list(running):
                        reward, done = 0.0, False
                        for _ in range(self.repeat_action):
                            observations[e], reward, done, _ = wave[e].step(env_actions[e])
                            total[e] += reward
                            if done:
                                break
                        similarity, speed, distance, hit = evaluation_info(wave[e])
                        for k, v in enumerate((similarity, speed, distance)):
                            metrics[e][k] += v
                        step_rewards[e] += float(reward)
                        if (done or t == timesteps) and t > 32:        # (t > 32: skips accidental collisions right after the start)
                            steps[e], collided[e], mask[e], recorded = t, hit, 0, True
                            running.remove(e)
                            print(f'Trial-{first + e} terminated after {t} timesteps in {round(time.time() - t0, 3)} '
                                  f'with total reward of {round(total[e], 3)}.')
                    if not running:
                        break
                    if recorded:
                        active = torch.tensor(mask, dtype=torch.int32, device=self.device)
                    batch = self.observe(observations, preprocess_fn)
                sums = stats.cpu().numpy()              # the wave's ONE read of the device sums
                for e in range(n):
                    t = steps[e]
                    assert int(sums[e, 3 * A + 1]) == t, (e, t, sums[e])
                    results['total_reward'].append(-1000.0 if total[e] < -1000.0 else total[e])
                    results['timesteps'].append(t)
                    results['collision_rate'].append(1.0 if collided[e] else 0.0)
                    results['similarity'].append(metrics[e][0] / t)
                    results['speed'].append(metrics[e][1] / t)
                    results['waypoint_distance'].append(metrics[e][2] / t)
                    self.log(eval_actions=float(sums[e, :A].sum()) / (t * A), eval_rewards=step_rewards[e] / t,
                             eval_distribution_mean=float(sums[e, A:2 * A].sum()) / (t * A),
                             eval_distribution_std=float(sums[e, 2 * A:3 * A].sum()) / (t * A), eval_values=float(sums[e, 3 * A]) / t)
                    self.log(**{f'eval_{k}': v[-1] for k, v in results.items()})
                    if self.is_writer():
                        self.write_summaries()
                    else:
                        self.statistics.stats = {}
            if self.is_writer():
                os.makedirs(self.evaluation_path, exist_ok=True)
                with open(save_path, 'w') as f:
                    json.dump(summarize(results), fp=f, indent=2)
        finally:
            self.aug_intensity = aug_intensity
            for env in shard:
                if hasattr(env, 'reset_info'):
                    env.reset_info()
            if close:
                for env in shard:
                    env.close()
        return results

    def explain(self, state, *, grid=(6, 8), per_frame=False, baseline='mean', modalities=True, upsample='nearest', normalize=True,
                chunk=32, row=0) -> dict:
        """Which part of one observation moves the decision: occlusion saliency of the acting network (no reference counterpart,
        DESIGN.md 6.15).  `state` is what predict() takes -- the dict observe([...], preprocess()) returns --, `row` the environment
        looked at when its leading axis is larger than 1.  `grid` = (gh, gw) cuts every frame into gh x gw cells (cell (cy, cx): rows
        [(cy*H)//gh, ((cy+1)*H)//gh), columns alike); one cell at a time is replaced by the `baseline` -- 'mean' (each frame's
        channel mean), 'zero', or a (T, H, W, 3) stack of the caller's, e.g. a blurred one from Augmenter.views -- in all T frames
        at once, or per frame with `per_frame` (F = T sets of cells instead of F = 1).  With `modalities`, four more variants
        occlude the whole image, road, vehicle and navigation (the vectors are zeroed).  Every variant is scored against the
        untouched observation: `kl` = KL(Beta(observation) || Beta(variant)) summed over the actions, `value` = the change of the
        value estimate base * 10^exp, `mean_a` = the signed shift of action a's Beta mean, all in double on the device.
        -> dict(alpha, beta, mean (A,), value (2,) -- the decision itself --, names = ['kl', 'value', 'mean_0', ...],
                scores float64 (F, gh, gw, K), maps {name: float32 (F, H, W)}, grid, frames,
                modalities {'image' | 'road' | 'vehicle' | 'navigation': {name: float}} when asked for).
        maps: 'nearest' gives every pixel the score of its cell (the attribution itself), 'bilinear' a resized grid for display;
        `normalize` divides each name's maps by its largest |score| over all cells (an all-zero name stays zero).  `scores` are
        never normalised.  Tensors stay on the device; the `modalities` floats are the call's one host read (4 x K doubles).

        Cost: N = 1 + F*gh*gw (+ 4) rows in ceil(N / chunk) inference forwards of the `chunk`-row engine, one rows launch per
        chunk, and a baseline, a scores and a maps launch.  First use with a `chunk` builds that engine and the chunk buffers
        (chunk x one observation); both are kept.
        Not touched: parameters, moving statistics, optimizer state, memories, logs, the sampler's stream (`action_index`); the
        forwards are predict()'s (old_policy, BatchNorm moving statistics).  Local to a rank: no collective.
        Not measured: whether the maps of a trained agent point at what a driver would look at -- there is no simulator here and no
        trained agent to look at; occlusion sensitivity depends on the baseline and the cell size, and a cell that scores 0 may
        still matter together with another.
        ValueError: a grid outside 1..H x 1..W, an unknown baseline or upsample name, a baseline of the wrong shape, chunk < 1 (or
        above the 65535 rows one launch takes), `row` outside the batch."""
        image = state['state_image']
        if len(image.shape) != 5:
            raise ValueError(f'explain: state_image must be (E, T, H, W, 3), got {tuple(image.shape)}')
        gh, gw, mode, _ = check_arguments(image.shape, image.shape[0], grid, baseline, upsample, chunk, row)
        row = int(row)
        one = {k: state[k][row] for k in ('state_image', 'state_road', 'state_vehicle', 'state_navigation')}
        stack = torch.as_tensor(one['state_image']).to(self.device, torch.float32).contiguous()
        if mode is None:
            base = torch.as_tensor(baseline).to(self.device, torch.float32).contiguous()
        else:
            base = occlusion_baseline(stack, BASELINES[mode])
        one['state_image'] = stack
        out = self.network.explain_rows(one, (gh, gw), base, per_frame=per_frame, modalities=modalities, upsample=upsample,
                                        normalize=normalize, chunk=int(chunk))
        T, H, W = stack.shape[:3]
        F, A = occlusion_frames(T, per_frame), self.num_actions
        names = score_names(A)
        cells = F * gh * gw
        alpha, beta = out['alpha'][0], out['beta'][0]
        result = dict(alpha=alpha, beta=beta, mean=alpha / (alpha + beta), value=out['value'][0], names=names, grid=(gh, gw), frames=F,
                      scores=out['scores'][:cells].view(F, gh, gw, len(names)),
                      maps={name: out['maps'][k] for k, name in enumerate(names)})
        if modalities:
            extra = out['scores'][cells:cells + 4].cpu().tolist()
            result['modalities'] = {m: dict(zip(names, extra[i])) for i, m in enumerate(MODALITIES)}
        return result

    def record(self, *args, **kwargs):
        raise NotImplementedError('CARLAgent.record drives a CARLA simulator; outside the learner hot path')

    def load_weights(self):
        self.network.load_weights(full=self.load_full)

    def save_config(self):
        self.update_config(dynamics_lr=self.dynamics_lr.serialize())
        super().save_config()


class CARLAMemory(PPOMemory):
    """PPOMemory whose state rows carry the `time_horizon` axis: (N, T, ...)."""

    def __init__(self, state_spec: dict, num_actions: int, time_horizon: int, device='cuda:0'):
        super().__init__(state_spec, num_actions, device=device)
        self.time_horizon = time_horizon

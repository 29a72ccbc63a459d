"""MI355X-native PPO learner hot path of carla-driving-rl-agent (HIP kernels behind a C ABI).

Sub-modules
  _lib      ctypes binding of libcdrl_hip.so (fails loudly when the library is missing)
  engine    LearnerEngine: parameter arenas + workspace as torch tensors, step functions
  synthetic deterministic synthetic rollout buffers
  train_stats  host side of the update diagnostics: ring rows -> the reference's log keys
  learner_state  on-disk container of the full learner state (arenas, optimizer scalars, counters, generators)
  evaluation  host side of CARLAgent.evaluate: driving metrics of an environment, per-trial seeds, the JSON record
  explain  host side of CARLAgent.explain: cell geometry and row order of the occlusion saliency, argument checks
  core, rl  host-side mirror of the reference's CARLAgent / CARLANetwork / PPOMemory API
"""
__version__ = '0.1.0'

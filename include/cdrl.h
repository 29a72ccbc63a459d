/* libcdrl_hip.so -- C ABI of the MI355X-native PPO learner hot path.
 *
 * Drop-in boundary for the learner path of Luca96/carla-driving-rl-agent.  The reference is pure
 * Python/TensorFlow and has no FFI of its own; each entry point below names the
 * reference interface (file:line under the reference repo) whose work it replaces.  Python
 * (ctypes) is the only caller today: carla-driving-rl-agent_amd/_lib.py, see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; cdrl_last_error() gives the message;
 *   - all pointers are DEVICE pointers to float32 unless stated; `stream` is a hipStream_t;
 *   - nothing allocates device memory: the caller passes arenas + a workspace sized by
 *     cdrl_learner_workspace_bytes(); entry points only enqueue work (no host sync);
 *   - observation tensors use the reference layout (B, T, H, W, 3) / (B, T, D), NHWC dense.
 */
#ifndef CDRL_H
#define CDRL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDRL_VERSION 1

typedef struct cdrl_learner cdrl_learner;

/* Network / batch geometry.  Defaults = CARLAgent.DEFAULT_* (core/carla_agent.py:61-68) on the
 * real CARLAEnv spaces (core/carla_env.py:18-24,64). */
typedef struct cdrl_config {
    int32_t B, T, H, W;                    /* minibatch, time_horizon, image height / width     */
    int32_t road, vehicle, navigation, A;  /* feature-vector sizes, num_actions                 */
    int32_t stem;                          /* 24                                                */
    int32_t stage_c[3];                    /* 116, 232, 464 (g = 1.0)                           */
    int32_t stage_n[3];                    /* 4, 8, 4                                           */
    int32_t last;                          /* 768                                               */
    int32_t feat, rnn_image, rnn_small, dyn, head; /* 16, 256, 32, 512, 320                     */
    float exp_scale;                       /* 6.0 (core/networks.py:169)                        */
    int32_t compute;                       /* CDRL_COMPUTE_*: arithmetic of the tower's 1x1 convolutions (default float32) */
    int32_t freeze_trunk;                  /* 0 (default) or 1: frozen trunk, see below; other values fail at create       */
    int32_t optimizer;                     /* CDRL_OPT_* (default CDRL_OPT_ADAM) of all three optimizers; see below         */
    float polyak;                          /* (0, 1], default 1 (off): polyak averaging of the heads; see below            */
    int32_t train_stats;                   /* 0 (default, off) or N > 0: ring of N update-diagnostics rows; see cdrl_train_stats_layout */
    int32_t clip_mode;                     /* CDRL_CLIP_TENSOR (default) or CDRL_CLIP_GLOBAL; other values fail at create; see below   */
    int32_t skip_nonfinite;                /* 0 (default) or 1: skip apply steps with a non-finite gradient; other values fail; see below */
    int32_t trust;                         /* 0 (default) or 1: trust-region guard of the policy steps; other values fail; see cdrl_trust_params */
} cdrl_config;

/* optimizer -- PPOAgent(optimizer=name) (reference rl/utils.py:29-46, rl/agents/ppo.py:105-106, core/carla_agent.py:123-124): one
 * Keras optimizer class for the policy, value and dynamics optimizers, built with the learning rate only, so every other
 * constant is a Keras default.  Fixed at create; unknown values fail there.  Each optimizer keeps at most two per-element slots,
 * in the adam_m / adam_v arenas (layouts unchanged); a slot an optimizer does not use is never written.  g is the gradient after
 * the per-tensor clip (heads) or unclipped (trunk), t the optimizer's step count including this step, lr the step's learning
 * rate, eps / beta1 / beta2 those of cdrl_hparams.  Scalar coefficients are float32, as in TensorFlow.
 *   name      adam_m      adam_v       initial m, v   update
 *   adam      m           v            0, 0           ResourceApplyAdam (unchanged)
 *   sgd       -           -            -              p -= lr g
 *   rmsprop   -           rms          -, 0           rho 0.9: r = rho r + (1 - rho) g^2; p -= lr g / (sqrt(r) + eps)
 *   adagrad   -           accumulator  -, 0.1         a += g^2; p -= lr g / (sqrt(a) + eps)
 *   adadelta  accum_var   accum_grad   0, 0           rho 0.95: a = rho a + (1 - rho) g^2; u = sqrt(d + eps) rsqrt(a + eps) g;
 *                                                     p -= lr u; d = rho d + (1 - rho) u^2
 *   adamax    m           v            0, 0           m += (g - m)(1 - beta1); v = max(beta2 v, |g|); p -= lr / (1 - beta1^t) m / (v + eps)
 *   nadam     m           v            0, 0           schedule decay 0.004: mu_t = beta1 (1 - 0.5 * 0.96^(0.004 t)); S_t = m_cache mu_t
 *                                                     (m_cache: one float per optimizer, starts at 1, becomes S_t every step);
 *                                                     S' = S_t mu_(t+1); m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2;
 *                                                     p -= lr [(1 - mu_t) g / (1 - S_t) + mu_(t+1) m / (1 - S')] / (sqrt(v / (1 - beta2^t)) + eps)
 *   ftrl      linear      accumulator  0, 0.1         lr_power -0.5, l1 = l2 = 0: n' = n + g^2; z += g - (sqrt(n') - sqrt(n)) / lr p;
 *                                                     p = |z| > 0 ? -z / (sqrt(n') / lr) : 0; n = n'
 * The initial slot values are also reported by cdrl_optimizer_slots.  cdrl_learner_reset_optimizer_steps resets the step counters
 * to 0 and the Nadam m_caches to 1; the slots are the caller's arenas.  A frozen trunk's slots, counter and m_cache are untouched.
 *
 * polyak < 1 -- PPOAgent(polyak=a) (reference rl/agents/ppo.py:242-247,268-271, rl/utils.py:105-117): after each head's optimizer
 * step its trainable tensors become a * p_new + c * p_old with a = (float)polyak, c = (float)(1 - (double)polyak), two float32
 * products and one float32 sum, in the same pass as the update.  The trunk is not averaged (the reference's dynamics optimizer
 * has none).  The non-trainable BatchNorm moving statistics are not touched (the reference blends two identical arrays there, a
 * difference of float32 rounding only).  old_policy still receives the pre-update policy.  polyak = 1 is the plain update. */
enum { CDRL_OPT_ADAM = 0, CDRL_OPT_SGD = 1, CDRL_OPT_RMSPROP = 2, CDRL_OPT_ADAGRAD = 3, CDRL_OPT_ADADELTA = 4, CDRL_OPT_ADAMAX = 5,
       CDRL_OPT_NADAM = 6, CDRL_OPT_FTRL = 7 };

/* Gradient gate -- clip_mode and skip_nonfinite, both fixed at create and both off by default: a learner with neither enqueues in
 * its apply steps exactly the launches it enqueues without the feature.  Both rest on the squared norm S of an optimizer's whole
 * gradient LIST (policy head, value head, trunk), known on the device before any element of the list is applied: the sum in
 * double of the squares of the float32 gradient elements of the list's trainable tensors (the padding between tensors is not part
 * of it), as per-1024-element chunk sums folded in a fixed order.
 *
 * clip_mode = CDRL_CLIP_GLOBAL -- tf.clip_by_global_norm(gradients, norm) in place of utils.clip_gradients (per-tensor
 * tf.clip_by_norm; reference rl/utils.py:120-121) in each apply_*_gradients: the policy head's list is clipped with
 * cdrl_hparams.clip_norm_policy in policy_apply, the value head's with clip_norm_value in value_apply, and the trunk's with
 * clip_norm_dynamics in both (not on a frozen trunk, which takes no step).  For a list with threshold c > 0 the scale is
 * s = (float)(c / max(sqrt(S), c)), computed in double and rounded once, and every element becomes g * s, one float32 multiply;
 * sqrt(S) <= c gives s == 1.0f exactly, an update identical bit for bit to the unclipped one.  A list with c <= 0 is not scaled
 * (and its norm not computed unless the guard needs it).  With CDRL_CLIP_TENSOR clip_norm_dynamics is accepted and ignored: the
 * trunk is never clipped, as in the reference.
 *
 * skip_nonfinite = 1 -- before anything is written, the apply step looks at the lists it is about to consume (the head's, and the
 * trunk's unless frozen): if any S is not finite -- exactly when some element is NaN or +-Inf; finite float32 gradients cannot
 * overflow the double sums, so a huge finite gradient is clipped or applied, never skipped -- the whole step is skipped.  A skipped
 * step leaves bit-identical the whole parameter arena (old_policy included), both slot arenas, the three step counters and the
 * Nadam m_caches, and increments the head's skip counter on the device.  Its train-stats row, when the ring is on, is still
 * written and its norms show the non-finite values.  Works in both clip modes.  The decision is a pure function of the gradient
 * arena: data-parallel ranks, whose arenas are identical after the all-reduce, decide alike with no collective.
 *
 * A gated apply enqueues: chunk sums (one launch for the lists involved), the gate (one workgroup: scales, skip flag, counter
 * ticks), trunk update, old_policy copy (policy_apply), head update -- one launch more than the ungated step, no host read, no
 * atomics; it can be captured in a hipGraph like the ungated one. */
enum { CDRL_CLIP_TENSOR = 0, CDRL_CLIP_GLOBAL = 1 };

/* freeze_trunk = 1 -- CARLAgent(update_dynamics=False) (reference core/carla_agent.py:77-80,351-373,430-463): the learner trains the
 * policy and value heads on a fixed trunk.  Fixed at create (the planner then leaves out the trunk-backward scratch:
 * cdrl_learner_workspace_bytes is smaller); parameter tables, region offsets and arena layouts are those of freeze_trunk = 0, so
 * checkpoints and arenas interchange.  Every compute mode is supported.  On a frozen learner:
 *   policy_forward_backward(_resample), policy_backward, value_forward_backward: train-mode trunk forward (batch statistics; every
 *     trunk BatchNorm updates its moving statistics as in a full pass), the head's loss and backward.  No trunk backward runs:
 *     the trunk's slice of the gradient arena is NOT written, and a communication stream set with cdrl_learner_set_comm_stream is
 *     never released mid-pass (the whole arena is final when the pass's own stream is).
 *   policy_apply, value_apply: per-tensor clip and Adam of the head (policy: old_policy <- policy in between) only; the trunk's
 *     parameters, Adam moments and Adam step counter are untouched.
 *   cdrl_learner_tail_offset: the trunk size (no trunk gradient becomes final mid-pass).
 *   predict, update_old_policy, trunk_forward_train: unchanged. */

/* CDRL_COMPUTE_BF16_OPERANDS (BASELINE.json configs[2]): the 1x1 convolutions of the image tower (core/architectures.py:130,140,
 * 170) multiply bf16-rounded operands on v_mfma_f32_32x32x16_bf16 -- forward, backward-data and filter gradient; float32
 * accumulation, float32 tensors in HBM, float32 BatchNorm statistics, bias gradients, optimizer and master weights.
 * CDRL_COMPUTE_BF16_STORAGE (configs[2] in full): the same arithmetic AND bf16 activation storage -- every activation and
 * activation-gradient tensor of the image tower (raw conv outputs, unit outputs, their gradients, the scratch gradients) lives
 * in HBM as bf16 (round-to-nearest-even on store); BatchNorm statistics are those of the stored values; LDS tiles, accumulators,
 * statistics / partial sums (double), coefficients, weights, gradients of weights and everything behind the global average
 * pool stay float32.  Half the activation traffic of the float32 path. */
enum { CDRL_COMPUTE_F32 = 0, CDRL_COMPUTE_BF16_OPERANDS = 1, CDRL_COMPUTE_BF16_STORAGE = 2 };

enum { CDRL_TRUNK = 0, CDRL_POLICY = 1, CDRL_VALUE = 2, CDRL_OLD_POLICY = 3 };

typedef struct cdrl_param_info {
    char name[64];
    int32_t shape[4];
    int32_t ndim;
    int32_t trainable;
    int64_t numel;
    int64_t offset;      /* element offset inside the model's trainable / state region */
} cdrl_param_info;

/* DynamicParameter values of the step (rl/parameters/parameters.py; rl/agents/ppo.py:42,55,61,
 * 101-106; core/carla_agent.py:120-124) + Keras Adam constants. */
typedef struct cdrl_hparams {
    float policy_lr, value_lr, dynamics_lr;
    float clip_ratio, entropy_coef;
    float clip_norm_policy, clip_norm_value;   /* <= 0 disables tf.clip_by_norm */
    float beta1, beta2, eps;
    float clip_norm_dynamics;                  /* threshold of the trunk's list with CDRL_CLIP_GLOBAL (<= 0: off); ignored otherwise */
} cdrl_hparams;

/* One policy minibatch = what CARLAgent.policy_batch_tensors yields (core/carla_agent.py:323-331)
 * plus the Beta samples of PolicyNetwork.call (core/networks.py:96-110). */
typedef struct cdrl_policy_batch {
    const float *image, *road, *vehicle, *navigation;
    const float *advantages;      /* (B)    */
    const float *old_log_prob;    /* (B, A) */
    const float *speed;           /* (B)  info_buffer['speed'] / 100 */
    const float *similarity;      /* (B)    */
    const float *u;               /* (B, A) Beta sample (or stored action) */
    const float *du_dalpha;       /* (B, A) pathwise Jacobian or NULL */
    const float *du_dbeta;        /* (B, A) or NULL */
    const float *anchor;          /* (B, 2, A) alpha0, beta0 of the anchor policy, or NULL; a learner with trust = 1 only (see cdrl_trust_params) */
} cdrl_policy_batch;

/* One value minibatch = CARLAgent.value_batch_tensors (core/carla_agent.py:333-349). */
typedef struct cdrl_value_batch {
    const float *image, *road, *vehicle, *navigation;
    const float *returns;         /* (B, 2) (base, exponent) */
    const float *speed, *similarity;
} cdrl_value_batch;

const char* cdrl_last_error(void);
int cdrl_version(void);
/* Environment switches (no reference counterpart: the reference has no native code).  The library reads its CDRL_* tuning
 * switches from the environment; CDRL_DIAG_* switches skip work or synchronisation (WRONG RESULTS, timing diagnostics only) and
 * are honoured only together with the master switch CDRL_DIAG=1.
 * cdrl_env_overrides: writes "NAME=VALUE NAME=VALUE ..." of every CDRL_* variable of the process environment into buf (truncated
 * to cap bytes, NUL-terminated) and returns their count.  cdrl_diag_active: number of wrong-result switches in effect (0 unless
 * CDRL_DIAG=1): benchmarks must refuse to report when it is non-zero. */
int cdrl_env_overrides(char* buf, int cap);
int cdrl_diag_active(void);
/* CRC-32C (Castagnoli) of `n` host bytes continued from `crc` (0 to start): block and tensor checksums of the
 * TensorFlow checkpoint-V2 files CARLANetwork.save_weights writes (reference core/networks.py:297-300). */
uint32_t cdrl_crc32c(uint32_t crc, const void* data, size_t n);

/* ---- learner object ------------------------------------------------------------------------
 * replaces CARLANetwork.__init__ / dynamics_model / value_network / PolicyNetwork construction
 * (core/networks.py:150-176,223-253) for one minibatch size. */
int cdrl_learner_create(const cdrl_config* cfg, cdrl_learner** out);
void cdrl_learner_destroy(cdrl_learner* l);
void cdrl_config_default(cdrl_config* cfg);
/* Slots of optimizer CDRL_OPT_* `optimizer` (table above): used[0] / used[1] whether it keeps a slot in the adam_m / adam_v arena,
 * init[0] / init[1] the slot's initial value (0 for an unused slot).  -1 for an unknown optimizer.  Host only. */
int cdrl_optimizer_slots(int optimizer, int32_t* used, float* init);

/* variable inventory: Model.trainable_variables / get_weights ordering (core/networks.py:281-285) */
int cdrl_learner_param_count(const cdrl_learner* l, int model);
int cdrl_learner_param_info(const cdrl_learner* l, int model, int index, cdrl_param_info* out);
int64_t cdrl_learner_region_offset(const cdrl_learner* l, int model, int trainable);
int64_t cdrl_learner_region_elems(const cdrl_learner* l, int model, int trainable);
int64_t cdrl_learner_params_total(const cdrl_learner* l);
int64_t cdrl_learner_grads_total(const cdrl_learner* l);
size_t cdrl_learner_workspace_bytes(const cdrl_learner* l);

/* params: [policy_tr | trunk_tr | value_tr | policy_state | trunk_state | value_state | old_policy]
 * grads / adam_m / adam_v: [policy_tr | trunk_tr | value_tr] (one contiguous all-reduce buffer) */
int cdrl_learner_bind(cdrl_learner* l, float* params, float* grads, float* adam_m, float* adam_v, void* workspace,
                      size_t workspace_bytes);
int cdrl_learner_set_hparams(cdrl_learner* l, const cdrl_hparams* hp, void* stream);
/* Makes `l` read its hyper-parameters and Adam step counters from `owner`'s device block (both bound, sharing the same
 * parameter / Adam arenas): a second learner built for the ragged LAST minibatch of an update (the reference's tf.data
 * pipeline keeps it unless drop_remainder is set, rl/utils.py:365-393) then advances the same optimizer.  Fails when the two
 * were created with a different optimizer or polyak, or a different clip_mode or skip_nonfinite (`l` then also uses `owner`'s
 * gate block: one set of skip counters). */
int cdrl_learner_share_hparams(cdrl_learner* l, const cdrl_learner* owner);
/* Data-parallel overlap: `stream` (caller-owned, or NULL to switch off) is made to wait inside every
 * following *_forward_backward call for the point of the backward pass at which the gradients of the head and of the trunk
 * tail (every trunk tensor behind the image tower) are final.  A collective enqueued on that stream after the call has
 * returned runs concurrently with the tower's backward; the tower's gradients are final when the call's own stream is. */
int cdrl_learner_set_comm_stream(cdrl_learner* l, void* stream);
/* Element offset, inside the trunk's trainable region, of the first TAIL tensor: gradients [tail_offset, trunk size) plus the
 * head's are final when the communication stream is released, gradients [0, tail_offset) (the image tower) only when the
 * pass's own stream is.  Equals the trunk size when the stream is never released mid-pass (hipGraph replay, CDRL_GRAPH=1; a learner
 * created with freeze_trunk = 1, which writes no trunk gradient at all). */
int64_t cdrl_learner_tail_offset(const cdrl_learner* l);
/* The instantiations of the 1x1-conv forward / backward-data family that this learner's ops launch, noted while they
 * were built (a learner without device works): one line per distinct plan signature, "nn ok ksm nt pro epi mode acc", "x3 ok form kp nt
 * pro epi" or "x3b ok sh epi acc".  Writes at most n bytes (NUL-terminated) and returns the bytes needed; -1 without a learner. */
int cdrl_learner_pw_signatures(const cdrl_learner* l, char* buf, int n);
/* Step counters to 0 and the Nadam m_caches to 1 (a fresh optimizer; the slots in the arenas are the caller's to reset). */
int cdrl_learner_reset_optimizer_steps(cdrl_learner* l, void* stream);
/* The optimizer's device-side scalars: with the parameter arena and the two slot arenas (the caller's tensors) they are the whole
 * state of the learner, so a caller that saves all four can continue a run bit for bit.  Both calls address the block the learner
 * reads at its steps: the owner's after cdrl_learner_share_hparams.  A frozen trunk's counter and m_cache are read and written like
 * the others (the frozen learner never advances them).
 * _get: copies the six values behind everything enqueued on `stream` and waits for that copy (the one host read of a save).
 * _set: enqueued on `stream` like cdrl_learner_reset_optimizer_steps, no host sync; `in` may be freed when the call returns.  The
 * hyper-parameters of cdrl_learner_set_hparams are not touched.  A negative counter, or an m_cache that is not finite or not
 * positive, is refused with -1 (cdrl_last_error) and nothing is written. */
typedef struct cdrl_optimizer_state {
    int32_t t_policy, t_value, t_dynamics;                        /* steps taken so far */
    float   m_cache_policy, m_cache_value, m_cache_dynamics;      /* Nadam; 1 for a fresh optimizer */
} cdrl_optimizer_state;
int cdrl_learner_get_optimizer_state(const cdrl_learner* l, cdrl_optimizer_state* out, void* stream);
int cdrl_learner_set_optimizer_state(cdrl_learner* l, const cdrl_optimizer_state* in, void* stream);
/* Gradient-gate statistics (see clip_mode / skip_nonfinite above) of the block the learner gates with (the owner's after
 * cdrl_learner_share_hparams).  Index 0 is policy_apply, 1 value_apply.  skipped / applied: apply steps since create or the last
 * _reset.  norm / scale: sqrt(S) (rounded to float32) and s of the head's own list, norm_dynamics / scale_dynamics those of the
 * trunk's list, at the LAST apply of that head; a norm that was not computed reads 0, a list that was not scaled has scale 1.
 * The counters are diagnostics: they are neither part of cdrl_optimizer_state nor of a saved learner state.
 * _stats: ONE device-to-host copy behind everything enqueued on `stream`, and waits for it.  _reset: the four counters to 0,
 * enqueued on `stream`, no host sync.  Both fail with -1 on a learner that has neither option on. */
typedef struct cdrl_gate_stats {
    int32_t skipped[2], applied[2];
    float norm[2], scale[2];
    float norm_dynamics[2], scale_dynamics[2];
} cdrl_gate_stats;
int cdrl_learner_gate_stats(const cdrl_learner* l, cdrl_gate_stats* out, void* stream);
int cdrl_learner_gate_reset(cdrl_learner* l, void* stream);

/* ---- trust-region guard of the policy steps -----------------------------------
 * cdrl_config.trust = 1, fixed at create and off by default: a learner without it enqueues exactly the launches it enqueues without
 * the feature.  The ratio clip of the policy loss zeroes the surrogate's gradient of the rows outside its band; it does not keep the
 * other rows, the entropy term or the auxiliary heads from carrying the policy further.  The guard measures how far the policy of
 * the pass in flight is from an ANCHOR policy -- alpha0, beta0 per row and action, cdrl_policy_batch.anchor -- as the analytic
 * KL(Beta(alpha0, beta0) || Beta(alpha, beta)) of cdrl_beta_kl (below), on the device, and latches when it leaves the region.
 *
 * On a learner with trust = 1:
 *   policy_forward_backward(_resample), policy_backward with b->anchor != NULL: cdrl_beta_kl's kernel runs directly behind the policy
 *     loss, in front of the head's backward.  It adds kl_coef * dKL/dlin to the head's dlin when kl_coef > 0 (and does not touch it
 *     when kl_coef == 0), updates the block's statistics, sets `armed`, and sets the latch `stop` when target_kl > 0 and
 *     !(kl <= kl_stop_factor * target_kl) -- a NaN KL (a broken anchor) stops the run.  The latch stays until _trust_reset.
 *   a policy, clone or representation pass WITHOUT an anchor: one one-thread launch clears `armed`; its apply is never gated by an
 *     old latch.
 *   policy_apply: always the gated sequence of the gradient gate (per-tensor clip with CDRL_CLIP_TENSOR); the gate additionally
 *     skips when armed && stop.  A skipped step leaves bit-identical what a skip_nonfinite skip leaves: the parameter arena
 *     (old_policy included), the slot arenas, the three step counters, the Nadam m_caches -- the trunk's step is left out with the
 *     head's -- and counts in `skipped` (and in cdrl_gate_stats.skipped[0]).  With finite gradients and no latch the step writes the
 *     bits of the ungated step.  cdrl_learner_gate_stats / _gate_reset still fail unless clip_mode / skip_nonfinite ask for the gate.
 *   value_apply: never decided by the latch (ungated unless clip_mode / skip_nonfinite gate it).
 *   joint_forward_backward(_resample), clone_forward_backward with returns, joint_apply: -1 (gating half of a joint apply is not
 *     defined).  An anchor handed to a learner WITHOUT trust: -1.  Both before any launch.
 *   cdrl_learner_share_hparams: the two learners then also share the trust block (one latch); -1 when they disagree on trust.
 * No pass or apply reads anything back to the host; all of them can be captured in a hipGraph.
 *
 * cdrl_learner_set_trust_params: the block's host-written head, enqueued on `stream` like cdrl_learner_set_hparams (of which it is
 * the trust learner's extension: cdrl_hparams keeps its size).  Defaults at create: target_kl 0 (measure only, never latch),
 * kl_stop_factor 1.5, kl_coef 0.  -1 for a negative or NaN value, a kl_stop_factor <= 0, or a learner without trust.
 * cdrl_learner_trust_stats: ONE device-to-host copy of the block behind everything on `stream`, and waits for it.
 * cdrl_learner_trust_reset: latch, counters and sums to their initial values (stop_pass -1), enqueued on `stream`, no host sync; the
 * head stays.  The block is a diagnostic and a safeguard: it is neither part of cdrl_optimizer_state nor of a saved learner state. */
typedef struct cdrl_trust_params {
    float target_kl;        /* <= 0: never latch */
    float kl_stop_factor;   /* the latch sets above kl_stop_factor * target_kl */
    float kl_coef;          /* weight of the KL penalty's gradient; 0: none */
} cdrl_trust_params;
typedef struct cdrl_trust_stats {
    float target_kl, kl_stop_factor, kl_coef;   /* as last set */
    float kl_last, kl_max;                      /* KL of the last measured pass; largest since the reset */
    int32_t passes;                             /* measured passes since the reset */
    int32_t stop, stop_pass;                    /* the latch; index among the measured passes of the one that set it, -1 before */
    int32_t armed;                              /* the last pass measured a KL */
    int32_t skipped;                            /* policy applies the latch skipped since the reset */
    double kl_sum;                              /* sum of kl_last over the measured passes */
} cdrl_trust_stats;
int cdrl_learner_set_trust_params(cdrl_learner* l, const cdrl_trust_params* tp, void* stream);
int cdrl_learner_trust_stats(const cdrl_learner* l, cdrl_trust_stats* out, void* stream);
int cdrl_learner_trust_reset(cdrl_learner* l, void* stream);

/* ---- update diagnostics (train stats) --------------------------------------------------------
 * The scalars PPOAgent.update / CARLAgent.update log per minibatch (reference rl/agents/ppo.py:209-225; core/carla_agent.py:382,
 * 423-426,461,483-484), produced on the device.  A learner created with cdrl_config.train_stats = N > 0 keeps a ring of N rows in
 * its workspace; every cdrl_learner_policy_apply / _value_apply appends ONE row behind its updates (three small launches; two on
 * a frozen trunk).  The row index is a device-side counter, so a replayed hipGraph of the apply step writes successive rows, and
 * nothing is read back per step: the host copies the ring once per update().  With train_stats = 0 nothing is allocated and the
 * apply steps enqueue exactly the launches they enqueue without the feature.
 * The buffer is `header` int32 words -- [0] rows written since the last reset, [1] rows overwritten before a reset (the ring is
 * full: the oldest row goes) -- followed by `rows` rows of `width` float32; row r of the current sequence sits at index
 * r % rows.  Fields of a row, as offsets in floats (kind, t_head, t_dynamics hold int32 bit patterns):
 *   kind           0 policy_apply, 1 value_apply
 *   t_head         step count of the head's optimizer INCLUDING this step; t_dynamics: the trunk's (frozen: unchanged)
 *   lr             learning rate of the head in force (cdrl_hparams policy_lr / value_lr); lr_dynamics; clip_ratio; entropy_coef
 *   speed          mean over the B rows of 2 * sigmoid(lin) of the head's speed output (CDRL_BUF_LIN_P column 2A + 1, _V column 2);
 *   similarity     mean of tanh(lin) of its similarity output (column 2A, _V column 3) -- float64 sums, fixed order
 *   metrics        the 16 floats of CDRL_BUF_METRICS_P (kind 0) or _V (kind 1) of the pass in front of the apply, verbatim
 *   norms          n_policy (kind 0) or n_value (kind 1) floats: L2 norm of every trainable tensor's gradient of the head, in
 *                  parameter-table order; trunk_norms: n_trunk floats, the trunk's (n_trunk = 0 with freeze_trunk = 1, as the
 *                  reference logs no dynamics norms with update_dynamics=False).  Unused slots of a row are 0.
 * The norms are those of the gradient arena at the apply: after grad_scale and any all-reduce the caller ran, BEFORE the per-tensor
 * clip (the reference logs the lists get_*_gradients returned; tf.clip_by_norm runs on a copy).  Squared sums are accumulated in
 * float64 in two deterministic stages (1024-element chunks, then per tensor; the heads reuse the clip path's chunk sums), then
 * sqrt in float64 and one rounding to float32.
 * cdrl_learner_share_hparams also makes `l` append to `owner`'s ring when both have one (same train_stats and freeze_trunk
 * required), so that the rows of a ragged last minibatch land in order.
 * cdrl_learner_train_stats_layout: host only, valid after create (rows = 0 and all fields 0 when off).  _buffer: device pointer
 * and byte size of header + rows of a bound learner (the owner's after share_hparams).  _reset: both counters to 0, enqueued on
 * `stream` like every other entry point (no host sync). */
typedef struct cdrl_train_stats_layout {
    int32_t rows, width, header;
    int32_t kind, t_head, t_dynamics;
    int32_t lr, lr_dynamics, clip_ratio, entropy_coef, speed, similarity;
    int32_t metrics, norms, trunk_norms;
    int32_t n_policy, n_value, n_trunk;
} cdrl_train_stats_layout;
int cdrl_learner_train_stats_layout(const cdrl_learner* l, cdrl_train_stats_layout* out);
int cdrl_learner_train_stats_buffer(const cdrl_learner* l, void** ptr, int64_t* bytes);
int cdrl_learner_train_stats_reset(cdrl_learner* l, void* stream);

/* CARLAgent.get_policy_gradients (core/carla_agent.py:351-373): train-mode trunk forward,
 * policy_objective (:394-428), gradients w.r.t. policy and trunk variables.  grad_scale = 1 /
 * world_size for data-parallel averaging. */
int cdrl_learner_policy_forward_backward(cdrl_learner* l, const cdrl_policy_batch* b, float grad_scale, void* stream);
/* The same step split at the Beta sample: PolicyNetwork.call re-samples an action
 * from the NEW Beta(alpha, beta) (core/networks.py:96-110).  policy_forward runs the train-mode
 * forward and leaves (alpha, beta, mean, std) in CDRL_BUF_AUX_P; the caller draws u and its
 * pathwise Jacobians; policy_backward evaluates the loss on them and back-propagates. */
int cdrl_learner_policy_forward(cdrl_learner* l, const float* image, const float* road, const float* vehicle,
                                const float* navigation, void* stream);
int cdrl_learner_policy_backward(cdrl_learner* l, const cdrl_policy_batch* b, float grad_scale, void* stream);
/* Fully on-device form of the re-sampling step: forward, u ~ Beta(alpha, beta) of the new policy drawn
 * by cdrl_beta_sample with pathwise Jacobians (what TFP's reparameterised Beta provides to
 * PolicyNetwork.call, core/networks.py:96-110,136-137), backward.  b->u / du_* are ignored.
 * (seed, offset) select the Philox stream; the drawn sample is left in CDRL_BUF_SAMPLE. */
int cdrl_learner_policy_forward_backward_resample(cdrl_learner* l, const cdrl_policy_batch* b, uint64_t seed,
                                                 uint64_t offset, float grad_scale, void* stream);
/* Brackets a SEQUENCE of learner calls enqueued from one stream with nothing of the caller's own between them -- the four calls of
 * one minibatch of PPOAgent.update on one GPU (rl/agents/ppo.py:190-226: policy gradients, apply, value gradients, apply).  Each
 * learner call orders the engine's streams behind `stream` on entry and `stream` behind them on return; inside a sequence that
 * happens once, in begin and in end.  Between the two, work the caller enqueues on `stream` is NOT ordered against the learner calls
 * (collectives between a pass and its apply: do not bracket them).  Calls on other streams are unaffected.  No nesting. */
int cdrl_learner_sequence_begin(cdrl_learner* l, void* stream);
int cdrl_learner_sequence_end(cdrl_learner* l, void* stream);
/* CARLAgent.apply_policy_gradients (core/carla_agent.py:375-388) + PPOAgent.apply_policy_gradients
 * (rl/agents/ppo.py:238-252): trunk Adam, per-tensor clip, old_policy <- policy, policy Adam (freeze_trunk = 1: no trunk Adam).
 * With another cdrl_config.optimizer, that optimizer's step in place of Adam's; polyak < 1 averages the policy after its step.
 * With clip_mode = CDRL_CLIP_GLOBAL or skip_nonfinite = 1: the gated sequence (gradient gate, above). */
int cdrl_learner_policy_apply(cdrl_learner* l, void* stream);
/* CARLAgent.get_value_gradients / apply_value_gradients (core/carla_agent.py:430-463;
 * rl/agents/ppo.py:264-275). */
int cdrl_learner_value_forward_backward(cdrl_learner* l, const cdrl_value_batch* b, float grad_scale, void* stream);
int cdrl_learner_value_apply(cdrl_learner* l, void* stream);
/* ---- joint policy + value update (opt-in; no reference counterpart) ---------------------------
 * The reference (and the four calls above) runs the whole trunk twice per minibatch: a train-mode forward and a full backward for
 * the policy loss, and again for the value loss, with a trunk optimizer step behind each.  The joint step sums the two losses on ONE
 * shared-trunk forward and back-propagates once.  What differs from the reference:
 *   - ONE trunk optimizer step per minibatch with dynamics_lr, where the reference takes two (t_dynamics advances once);
 *   - the trunk's BatchNorm moving statistics are updated once per minibatch, not twice;
 *   - the loss is policy total loss + value total loss, each exactly as policy_forward_backward / value_forward_backward form it
 *     (no extra weight); the value head sees the trunk BEFORE the policy's step of the same minibatch, not after it.
 * Nothing is configured at create: a learner may mix joint and separate steps, and learners sharing hyper-parameters
 * (cdrl_learner_share_hparams) work unchanged.
 *
 * cdrl_learner_joint_forward_backward: the stored-action / injected-Jacobian loss (b->u, b->du_dalpha, b->du_dbeta as in
 * cdrl_learner_policy_forward_backward) plus the value loss on `returns` (B, 2: base, exponent); the value loss takes b->speed and
 * b->similarity (the agent gives both heads the same targets).  Order: train-mode trunk forward once, policy head forward, value
 * head forward, policy loss, policy head backward, value loss, value head backward, then ONE launch (cdrl_bn_small_bwd_pair) that
 * finishes the first BatchNorm of both heads and writes d(policy loss)/d(dynamics) + d(value loss)/d(dynamics), then the trunk
 * backward once.  The gradients of both heads, CDRL_BUF_METRICS_P / _V and CDRL_BUF_AUX_P / _V are bit-identical to those of the
 * separate passes on the same parameters; the trunk's gradient is the sum of theirs up to float32 rounding.  The communication
 * stream (cdrl_learner_set_comm_stream) is released where the separate passes release it: both heads' gradients and the trunk
 * tail's are final there, and cdrl_learner_tail_offset is unchanged.  freeze_trunk = 1: no trunk backward, the trunk's gradient
 * slice is not written.  Captured and replayed as a hipGraph like policy_forward_backward.
 * _resample: the same with u ~ Beta(alpha, beta) of the new policy drawn on the device behind the policy head's forward, as
 * cdrl_learner_policy_forward_backward_resample (sample left in CDRL_BUF_SAMPLE; eager, not replayed).
 * LIMIT (deliberate): both fail with -1 (cdrl_last_error names the limit) on a learner with B > 2048, where the heads' first
 * BatchNorm is not in the single-launch form; there is no joint form above it.
 *
 * cdrl_learner_joint_apply: the optimizer steps of a joint pass.  Ungated: trunk update ONCE (not with freeze_trunk = 1), per-tensor
 * norms of the policy head (they tick t_policy and t_dynamics), old_policy <- policy, policy head update, per-tensor norms of the
 * value head (they tick t_value only), value head update.  Nadam m_caches advance with the counters they belong to.
 * Gradient gate (clip_mode / skip_nonfinite): the gated policy_apply as it is, trunk included, then the gated value_apply WITHOUT
 * the trunk.  Skip rule: the trunk and the policy head (and old_policy) are decided together, from the trunk's and the policy's
 * list -- a non-finite element in either skips both, and counts as skipped[0]; the value head is decided from its own list alone
 * (skipped[1]).  Clip rule with CDRL_CLIP_GLOBAL: each of the three lists is clipped once, by its own threshold (clip_norm_policy,
 * clip_norm_dynamics, clip_norm_value); norm_dynamics[1] reads 0 and scale_dynamics[1] reads 1 after a joint apply.
 * Train stats: two rows per joint apply, the policy's (kind 0), then the value's (kind 1); both carry the norms of the one joint
 * trunk gradient and the same t_dynamics. */
int cdrl_learner_joint_forward_backward(cdrl_learner* l, const cdrl_policy_batch* b, const float* returns, float grad_scale,
                                       void* stream);
int cdrl_learner_joint_forward_backward_resample(cdrl_learner* l, const cdrl_policy_batch* b, const float* returns, uint64_t seed,
                                                uint64_t offset, float grad_scale, void* stream);
int cdrl_learner_joint_apply(cdrl_learner* l, void* stream);
/* ---- behaviour cloning (supervised pre-training on expert traces) --------------
 * The reference's curriculum calls agent.imitation_learning in front of the reinforcement stage but never defines it for CARLAgent;
 * the definition here is the project's own: maximum likelihood of the expert's action under the policy's Beta(alpha, beta).
 *
 * cdrl_learner_clone_forward_backward: train-mode trunk forward, policy head forward (and value head forward with b->returns), then
 * the loss of cdrl_beta_clone_loss (below) in the place of the policy loss, with entropy_coef read from the device hyper-parameters
 * like the policy loss reads it; policy head backward; with b->returns the value loss and the joint tail exactly as in
 * cdrl_learner_joint_forward_backward (same order, same B <= 2048 limit), otherwise the policy pass's tail.  Writes
 * CDRL_BUF_METRICS_P (slots 0..7, table at cdrl_beta_clone_loss) and CDRL_BUF_AUX_P; with returns also CDRL_BUF_METRICS_V / _AUX_V.
 * policy_weight and value_weight scale GRADIENTS only: the d(loss)/d(lin) of the clone loss is multiplied by grad_scale *
 * policy_weight, that of the value loss by grad_scale * value_weight; every metric stays unscaled.  aux_weight multiplies the
 * speed / similarity terms of the clone loss (total and gradient).  freeze_trunk = 1: no trunk backward, the trunk's gradient slice
 * is not written.  Captured and replayed as a hipGraph like the stored-action policy pass; the three weights are part of the key.
 * There is no apply of its own: a pass without returns is followed by cdrl_learner_policy_apply, one with returns by
 * cdrl_learner_joint_apply, so optimizers, polyak, the gradient gate and the train-stats rows work as they are.  Both applies copy
 * old_policy <- policy BEFORE the step: end a cloning run with cdrl_learner_update_old_policy, or the policy that acts lags one
 * step behind the one that was trained. */
typedef struct cdrl_clone_batch {
    const float *image, *road, *vehicle, *navigation;
    const float *u;            /* (B, A) expert action, unit interval */
    const float *weight;       /* (B) or NULL */
    const float *speed, *similarity;   /* (B) each; both NULL = no auxiliary targets (then returns must be NULL too) */
    const float *returns;      /* (B, 2) (base, exponent) or NULL = policy only */
} cdrl_clone_batch;
int cdrl_learner_clone_forward_backward(cdrl_learner* l, const cdrl_clone_batch* b, float policy_weight, float value_weight,
                                        float aux_weight, float grad_scale, void* stream);
/* ---- expert demonstrations inside the PPO update -------------------------------
 * A policy minibatch of fresh rows and demonstration rows through ONE trunk pass: the policy pass with the loss of
 * cdrl_beta_mixed_policy_loss (below, where its definitions stand) in the place of the policy loss.  demo_u (B, A) is the expert
 * action in the unit interval, demo_w (B) the row's weight: row b is a DEMONSTRATION row iff demo_w[b] > 0 and a PPO row otherwise.
 * With ND demonstration rows and NP = B - ND PPO rows the objective is
 *   sum_{PPO rows} surrogate_b / NP  +  sum_{demo rows} demo_w[b] * (-mean_a log Beta(clip(demo_u[b,a]); alpha, beta)) / ND
 *   - entropy_coef * entropy + speed_loss + sim_loss,      the last three over all B rows as in the policy loss;
 * a term whose row count is 0 is 0.  advantages, old_log_prob, u, du_dalpha and du_dbeta of a demonstration row are never read (they
 * may hold anything, NaN included); speed / similarity of such a row are its trace's targets.
 *
 * cdrl_learner_demo_forward_backward / _resample: trunk forward, head forward, head and trunk backward, freeze_trunk, compute modes,
 * the train-stats ring and the gradient gate are those of cdrl_learner_policy_forward_backward / _resample; the re-sampled form
 * draws u for all B rows with the same Philox offsets as the policy pass (the draw of a demonstration row is ignored).  The
 * stored-action form is captured and replayed as a hipGraph; batch pointers, demo_u, demo_w, grad_scale and the demonstration block
 * are the key.  Writes CDRL_BUF_METRICS_P slots 0..10 and CDRL_BUF_AUX_P.  With demo_w all zero the pass writes the bits of the
 * policy pass.  -1: a null demo_u / demo_w, a batch with an anchor (the trust-region sweep has no demonstration rows).  On a
 * learner with trust = 1 the pass clears the latch's `armed`, like every pass without an anchor.  The apply is
 * cdrl_learner_policy_apply as it is.
 *
 * cdrl_learner_set_demo_block: a caller-owned device block (cdrl_demo_stats, 40 bytes, 8-byte aligned, zeroed by the caller) that
 * every later demonstration pass of this learner adds to -- metrics slots 7..10 as rounded to float, and a pass count -- by one
 * thread behind the loss, in stream order, without atomics; NULL: none (the default).  Read it with one copy when the passes of an
 * update are enqueued.  Learners of several minibatch sizes may be given the same block. */
typedef struct cdrl_demo_stats {
    double loss_sum;           /* sum over the passes of the demonstration term (metrics[7]) */
    double log_prob_sum;       /* ... of the demonstration rows' mean log-probability (metrics[8]) */
    double mode_error_sum;     /* ... of their mean absolute mode error (metrics[9]) */
    double rows_sum;           /* ... of ND (metrics[10]) */
    int64_t passes;
} cdrl_demo_stats;
int cdrl_learner_set_demo_block(cdrl_learner* l, cdrl_demo_stats* device_block);
int cdrl_learner_demo_forward_backward(cdrl_learner* l, const cdrl_policy_batch* b, const float* demo_u, const float* demo_w,
                                       float grad_scale, void* stream);
int cdrl_learner_demo_forward_backward_resample(cdrl_learner* l, const cdrl_policy_batch* b, const float* demo_u, const float* demo_w,
                                                uint64_t seed, uint64_t offset, float grad_scale, void* stream);
/* ---- contrastive pre-training of the trunk ------------------------------------
 * The reference's curriculum calls agent.learn_representation and never defines it; rl/augmentations/simclr.py names the objective.
 * The definition here is the project's own: NT-Xent (table at the loss entry, below) on the trunk's output, B = 2N rows, rows i and
 * i + N being two views of one observation.  No projection head: no parameter is added.
 *
 * The pass: train-mode trunk forward (moving statistics move once), the loss on CDRL_BUF_DYNAMICS, the trunk's backward.  No head op
 * runs: the heads' gradient slices, CDRL_BUF_LIN_*, _METRICS_P / _V and _AUX_* are not written.  Writes the trunk's gradient slice
 * and CDRL_BUF_METRICS_R.  grad_scale multiplies the gradient only.  Captured and replayed as a hipGraph; the four pointers,
 * temperature and grad_scale are the key.  -1: freeze_trunk = 1, B odd, B > 2048, temperature <= 0.
 *
 * The apply: the trunk's optimizer step alone (cdrl_config.optimizer, learning rate lr_dynamics, unclipped), one tick of the trunk's
 * step counter (Nadam: and of its m_cache).  The parameters, slots and counters of both heads, old_policy, the gate block and the
 * train-stats ring stay as they are.  -1: freeze_trunk = 1; clip_mode = global or skip_nonfinite = 1 (the gate's decisions and
 * counters are per head). */
int cdrl_learner_repr_forward_backward(cdrl_learner* l, const float* image, const float* road, const float* vehicle,
                                       const float* navigation, float temperature, float grad_scale, void* stream);
int cdrl_learner_trunk_apply(cdrl_learner* l, void* stream);
/* CARLANetwork.update_old_policy (core/networks.py:281-285). */
int cdrl_learner_update_old_policy(cdrl_learner* l, void* stream);
/* CARLANetwork.predict deterministic part (core/networks.py:181-193): inference-mode trunk,
 * old_policy -> dist (B,4A: alpha, beta, mean, std), value heads -> (B,4: base, exp, speed, sim). */
int cdrl_learner_predict(cdrl_learner* l, const float* image, const float* road, const float* vehicle,
                         const float* navigation, float* dist_out, float* value_out, float* dynamics_out, void* stream);
/* CARLANetwork.dynamics_predict_train (core/networks.py:210-212). */
int cdrl_learner_trunk_forward_train(cdrl_learner* l, const float* image, const float* road, const float* vehicle,
                                     const float* navigation, void* stream);

enum {
    CDRL_BUF_DYNAMICS = 0,   /* (B, dyn)  trunk output                       */
    CDRL_BUF_IMG_FEAT = 1,   /* (T*B, last) tower output, frame = t*B + b    */
    CDRL_BUF_METRICS_P = 2,  /* 16 floats: total, policy, entropy, speed, sim, ratio, log_prob (last pass only; per-step history: train stats) */
    CDRL_BUF_METRICS_V = 3,  /* 16 floats: total, value, speed, sim           */
    CDRL_BUF_AUX_P = 4,      /* (B, 4A) alpha, beta, log_prob, entropy        */
    CDRL_BUF_AUX_V = 5,      /* (B, 2) value (base, exp)                      */
    CDRL_BUF_LIN_P = 6,      /* (B, 2A+2) linear head outputs                 */
    CDRL_BUF_LIN_V = 7,      /* (B, 4)                                        */
    CDRL_BUF_SAMPLE = 8,     /* (B, A) Beta sample drawn by ..._resample       */
    CDRL_BUF_METRICS_R = 9   /* 16 floats of the last representation pass: loss, top-1 accuracy, pair cosine, negatives' cosine, mean norm, temperature */
};
int cdrl_learner_get_buffer(const cdrl_learner* l, int which, float** ptr, int64_t* elems);
/* Named internal tensors of a bound learner, for parity tests: "<bn>.x" (raw BatchNorm input, dense NHWC rows with frames
 * f = t*B + b), "<bn>.stats" ([4][T][C]: mean, invstd, scale, shift of the last training forward), "<dense>.z" (dense
 * pre-activation), "img.stem.pool.argmax" (one byte ky*3+kx per pooled element).  The discrete decisions of the last forward
 * (ReLU6 region = region of fmaf(scale, x, shift); max-pool argmax) are reconstructed from them, so that the float64 oracle
 * can be evaluated on the SAME decisions (reference core/architectures.py:47,161 are the sites). */
int cdrl_learner_named_buffer(const cdrl_learner* l, const char* name, void** ptr, int64_t* bytes);
/* Out-of-bounds canaries of the workspace (sanitizer row; there is no GPU AddressSanitizer on this pool and the
 * kernels address the workspace through raw buffer descriptors).  A learner created with CDRL_GUARD=1 in the environment plans its
 * workspace with a 64 KB band behind EVERY tensor (cdrl_learner_workspace_bytes grows accordingly) and cdrl_learner_bind fills the
 * bands with a pattern; this call checks them on `stream` (synchronises): *bad_bands = number of bands that no longer hold the pattern,
 * *first_bad_offset = byte offset (inside the workspace) of the first one, -1 if none.  Without CDRL_GUARD=1 it fails with -1. */
int cdrl_learner_check_guards(cdrl_learner* l, void* stream, int64_t* bad_bands, int64_t* first_bad_offset);

/* ---- rollout-buffer post-processing ---------------------------------------------------------
 * PPOMemory.compute_returns + compute_advantages (rl/agents/ppo.py:699-727), utils.gae /
 * discount_cumsum / decompose_number / tf_sp_norm (rl/utils.py:57-84,140-151,344-349).
 * rewards (N+1) and values_be (N+1, 2) already hold the bootstrap entry of end_trajectory
 * (rl/agents/ppo.py:692-697).  scratch: >= 2*(N+1)+2 doubles. */
int cdrl_gae_returns(const float* rewards, const float* values_be, int N, double gamma, double lambda, float scale,
                     float* returns, float* returns_be, float* adv_raw, float* adv, double* scratch, void* stream);
/* The same for S trajectories ("segments", N rows in all) in ONE launch, one 256-thread workgroup per segment -- an environment shard
 * with auto-reset closes E x (resets + 1) trajectories per rollout.  seg_off: DEVICE array of S + 1 row offsets, seg_off[0] = 0,
 * seg_off[S] = N, every n_s = seg_off[s+1] - seg_off[s] >= 1.  Inputs are padded with each segment's own bootstrap entry: segment s reads
 * rewards[seg_off[s] + s .. + n_s] (n_s + 1 values) and the values_be rows of the same range, so rewards holds N + S values and values_be
 * (N + S, 2).  Outputs are packed: segment s writes rows [seg_off[s], seg_off[s+1]) of returns (N), returns_be (N, 2), adv_raw (N) and
 * adv (N).  Scratch of segment s: 2 * (n_s + 1) doubles from 2 * (seg_off[s] + s); in all 2 * (N + S) doubles, which
 * cdrl_gae_segments_scratch_doubles returns.  Per-segment quantities stay per segment (scan carries start from 0, the sp-norm takes
 * max / min over that segment's advantages): every output equals, bit for bit, what cdrl_gae_returns gives for the segment alone.
 * A segment whose offsets are malformed (n_s <= 0, or outside [0, N]) is skipped and nothing of it is written.  Errors: null pointer,
 * S < 1, N < S, N + S beyond 32 bits. */
int cdrl_gae_returns_segments(const float* rewards, const float* values_be, const int32_t* seg_off, int S, int N,
                              double gamma, double lambda, float scale,
                              float* returns, float* returns_be, float* adv_raw, float* adv,
                              double* scratch, void* stream);
int64_t cdrl_gae_segments_scratch_doubles(int N, int S);
/* V-trace targets (Espeholt et al. 2018) for S REPLAYED trajectories in ONE launch, one 256-thread workgroup per segment: the rows were
 * collected by an older policy, so the TD errors are weighted by truncated importance ratios.  seg_off, rewards (N + S) and values_be
 * (N + S, 2) are laid out as for cdrl_gae_returns_segments; values_be holds the CURRENT value head's estimates.  alpha, beta (N, A): the
 * current policy's Beta parameters; actions (N, A): the stored actions in [0, 1]; log_prob_old (N, A): the stored behaviour
 * log-densities; A in 1..8.  Per row: V = base * 10^exp (float32), log pi = sum_a log Beta(u; alpha, beta) in float64 with u clipped
 * to [eps, 1 - eps], eps = 1.1920929e-07f (the clip of cdrl_beta_sample_logp), ratio = exp(log pi - sum_a log_prob_old) -- the JOINT
 * ratio over the A actions --, rho = min(rho_bar, ratio), c = min(c_bar, ratio), td = r + gamma V' - V, and two float64 recurrences
 * from carries 0:
 *   x_i = rho_i td_i + gamma lambda c_i x_{i+1},   adv_raw_i = td_i + gamma lambda x_{i+1}   (no rho factor: PPO's ratio supplies it)
 *   y_i = rho_i td_i + gamma c_i y_{i+1},          returns_i = V_i + y_i                     (lambda = 1: the rewards-to-go form)
 * then the tail of cdrl_gae_returns: returns_be = decompose_number(returns), adv = tf_sp_norm(adv_raw) * scale over the segment's own
 * max / min.  rho (N): the UNCLIPPED ratio, for diagnostics (inf where it overflows float32; the clipped weights stay finite).  With
 * every ratio >= 1 and rho_bar = c_bar = 1 the outputs are cdrl_gae_returns_segments' up to the float32 rounding of its deltas.
 * Scratch: 4 * n_s doubles per segment from 4 * seg_off[s], 4 * N in all, which cdrl_vtrace_segments_scratch_doubles returns.  Every
 * segment's outputs are the bits it gets when launched alone.  A segment whose offsets are malformed is skipped and nothing of it is
 * written.  Errors (-1, nothing launched): null pointer, S < 1, N < S, A outside 1..8, N + S beyond 32 bits, rho_bar or c_bar < 0. */
int cdrl_vtrace_segments(const float* rewards, const float* values_be, const float* alpha, const float* beta, const float* actions,
                         const float* log_prob_old, const int32_t* seg_off, int S, int N, int A,
                         double gamma, double lambda, double rho_bar, double c_bar, float scale,
                         float* returns, float* returns_be, float* adv_raw, float* adv, float* rho,
                         double* scratch, void* stream);
int64_t cdrl_vtrace_segments_scratch_doubles(int N, int S);

/* tfp.distributions.Beta(alpha, beta).sample() with reparameterisation gradients (core/networks.py:
 * 136-137): u = g1/(g1+g2), g ~ Gamma via Marsaglia-Tsang on a Philox-4x32-10 stream, du/dalpha and
 * du/dbeta by implicit differentiation of the Gamma CDF.  Element (row, col) reads alpha[row*ld + col]. */
int cdrl_beta_sample(const float* alpha, const float* beta, int rows, int A, int ld, uint64_t seed, uint64_t offset,
                     float* u, float* du_dalpha, float* du_dbeta, void* stream);
/* Rollout form (CARLANetwork.predict, core/networks.py:181-193 -> PolicyNetwork.call :96-103): the sample and the
 * log-density of the sample clipped to [eps, 1 - eps], no Jacobians. */
int cdrl_beta_sample_logp(const float* alpha, const float* beta, int rows, int A, int ld, uint64_t seed, uint64_t offset,
                          float* u, float* log_prob, void* stream);
/* Evaluation form (CARLAgent.evaluate, core/carla_agent.py:254-291): the action of every row of the block cdrl_learner_predict
 * writes -- dist [rows][4][A]: alpha, beta, mean, std -- and its log-density, in one launch, one thread per (row, a), no atomics.
 *   mode 0: the sample; action and log_prob are bit-identical to cdrl_beta_sample_logp on the same (alpha, beta, seed, offset)
 *           (Philox element index row * A + a, sample clipped to [eps, 1 - eps] with eps = 1.1920929e-07f for the log-density).
 *   mode 1: the mode of the Beta, action = (float)((alpha - 1) / (alpha + beta - 2)) evaluated in double (the policy head gives
 *           alpha, beta >= 1.01); log_prob is the same expression at that action.  seed and offset are not used.
 * action and log_prob (dense [rows][A]) are written for every row.  stats (may be null): [rows][CDRL_ACT_STATS(A)] doubles of
 * running sums, read-modify-written for the rows with active[row] != 0 (active: [rows] on the device, null = every row) and left
 * untouched for the others: slots a, A + a, 2A + a += action, mean, std of column a; slot 3A += base * 10^exp of value
 * ([rows][4]: base, exp, speed, similarity; may be null when stats is null); slot 3A + 1 += 1 (the step count).
 * Errors (-1, before any launch): null dist / action / log_prob, rows < 1 (or > 2^24), A < 1 or > 8, mode not 0 or 1, stats
 * without value. */
#define CDRL_ACT_STATS(A) (3 * (A) + 2)
int cdrl_beta_act(const float* dist, const float* value, int rows, int A, int mode, uint64_t seed, uint64_t offset,
                  const int32_t* active, float* action, float* log_prob, double* stats, void* stream);
/* bf16 ACTIVATION STORAGE at op level (configuration 3): the op-level entry points that have a bf16-storage form -- cdrl_bn_train_fwd /
 * _bwd (y, out, dout, dy), cdrl_dwconv_bn_fwd / _bwd (x, y, dout, dx), cdrl_pwconv_fused_packed and cdrl_pwconv_bn_bwd(_packed) with
 * packed_bf16 = 1 (a, c, epi_y; dout, y, x, dx), cdrl_pwconv_bwd_fused (+ _workspace), cdrl_gemm_tn (A, D), cdrl_gemm_x3 (A, C),
 * cdrl_maxpool_bn_fwd (y, p), cdrl_stem_fwd_stats (y), cdrl_stem_block_bwd(_pooled) (y, dp) -- take the element type of those ACTIVATION
 * tensors as an explicit argument `int act_type` in front of the stream: 0 float32, 1 bf16 (same pointer spelling, element strides and
 * offsets; round-to-nearest-even on store).  Statistics, coefficient blocks, partial sums, weights and weight gradients stay float32 /
 * double.  The library keeps no mode of its own (rounds 3-5 had a thread-local switch, cdrl_set_op_activation_type); cdrl_learner_* is
 * not concerned (Config::compute selects its storage). */
int cdrl_gamma_implicit_grad(const double* a, const double* g, int n, double* out, void* stream);
/* Test hook: the two Gamma draws (g1 ~ Gamma(alpha), g2 ~ Gamma(beta)) behind the sample u = g1 / (g1 + g2) of the same
 * (seed, offset) stream -> gammas[rows * A][2] doubles.  Lets a test check du/dalpha, du/dbeta sample by sample. */
int cdrl_beta_sample_gammas(const float* alpha, const float* beta, int rows, int A, int ld, uint64_t seed, uint64_t offset,
                            double* gammas, void* stream);
/* Test hook: the first `nblocks` raw Philox-4x32-10 blocks of the streams (seed, offset, idx0 + i), i < n -> out[n][nblocks][4].
 * (seed, offset) selects a stream: streams of different offsets are DISJOINT for any number of blocks per element (the block
 * counter lives in the top 16 bits of the element-index word, not in the offset). */
int cdrl_philox_words(uint64_t seed, uint64_t offset, uint64_t idx0, int n, int nblocks, uint32_t* out, void* stream);

/* Float32 1x1 convolution on the bf16 matrix pipe (exact three-way bf16 split of both operands, six bf16 MFMAs per K = 16
 * step; float32 in / out, float32-accurate, not bit-identical to an fmaf chain).  W_packed: cdrl_pwconv_x3_packed_bytes(K)
 * bytes written by cdrl_pwconv_x3_pack from B(k, n) = W[k * sbk + n * sbn].  Same prologue / epilogue contract as
 * cdrl_pwconv_fused (pro_stats: BN-apply on load; part: statistics partials, cdrl_pwconv_x3_partial_rows rows per group).
 * K, N <= 128: K, lda, a_coff even (the A chunks are 16-byte buffer loads at dword alignment; columns beyond K are zeroed: the
 * 58-channel convs of stage 0 qualify since round 6); 128 < K or N <= 256: K, lda, a_coff multiples of 4.  K or N above 128 (the 232-channel convs of stage 2, core/architectures.py:130,140 at
 * num_channels 464): W_packed holds one block per 128 output columns -- cdrl_pwconv_x3_packed_bytes_n(K, N) bytes -- and the kernel
 * takes one 32-row tile per workgroup (one statistics row per tile). */
int64_t cdrl_pwconv_x3_packed_bytes(int K);
int64_t cdrl_pwconv_x3_packed_bytes_n(int K, int N);
int cdrl_pwconv_x3_partial_rows(int G, int Mg, int N, int K);
int cdrl_pwconv_x3_pack(const float* W, int K, int N, int sbk, int sbn, void* packed, void* stream);
int cdrl_pwconv_x3(const float* A, int lda, int a_coff, const float* pro_stats, const void* W_packed, const float* bias, float* C,
                   int ldc, int c_coff, int G, int Mg, int N, int K, double* part, void* stream);
/* Backward-data of those wide convs (128 < Cin or Cout <= 256, Cout % 4 == 0) with the BatchNorm backward of the BatchNorm behind the conv
 * applied on load (core/architectures.py:130-141 under tape.gradient): da[G*Mg][ldda] (+ da_coff; += when accumulate) = dy W^T with
 * dy = k1 (mask dz - k2 - xhat(y) k3); dz [G*Mg][ld_dz] (+ dz_coff, gathered through the channel shuffle of dz_shuffle channels when
 * non-zero, ReLU6-masked from the BatchNorm output when act), y [G*Mg][Cout] raw conv output, stats [4][G][Cout] / coef [3][G][Cout].
 * W_packed: cdrl_pwconv_x3_pack(W, Cout, Cin, 1, Cout, ...) with cdrl_pwconv_x3_packed_bytes_n(Cout, Cin) bytes.  part2 (or NULL):
 * [G][rows][Cout] column sums of dy (the conv's bias gradient partials), rows = cdrl_pwconv_x3_wide_bwd_rows(Mg) (one per 32-row tile).
 * ey / epi_stats / part (all or none; not with accumulate): (sum da, sum da xhat(ey)) of the BatchNorm whose raw input is ey [G*Mg][Cin],
 * part [G][rows][2][Cin].  float32 tensors only. */
int cdrl_pwconv_x3_wide_bwd_rows(int Mg);
int cdrl_pwconv_x3_wide_bwd(const float* dz, int ld_dz, int dz_coff, int dz_shuffle, int act, const float* y, const float* stats,
                            const float* coef, const void* W_packed, float* da, int ldda, int da_coff, int accumulate, int G, int Mg,
                            int Cin, int Cout, double* part2, const float* ey, const float* epi_stats, double* part, void* stream);


/* Backward of the unit's 1x1 convolution + BatchNorm (core/architectures.py:130-141 under tape.gradient, core/carla_agent.py:
 * 364-365) as ONE pass over its operands: dy = BatchNorm-backward(dz, y) on load, da = dy W^T, dW = a^T dy, db = column sums of
 * dy.  dz [G*Mg][ld_dz] (+ dz_coff, gathered through the channel shuffle of dz_shuffle channels when non-zero, ReLU6-masked from
 * the BatchNorm output when act == 1), y [G*Mg][N] raw conv output, stats [4][G][N] / coef [3][G][N] of that BatchNorm.
 * a [G*Mg][lda] (+ a_coff) conv input; a_stats ([4][G][K], or NULL): a is the raw input of a BatchNorm (no activation) applied on
 * load, and that BatchNorm's dgamma / dbeta [K] and backward coefficients a_coef [3][G][K] are produced as well (from the filter
 * product, no pass over da).  W [K][N]; W_packed: cdrl_pwconv_x3_pack(W, N, K, 1, N, ...) (the transposed operand).
 * da [G*Mg][ldda] (+ da_coff; += when accumulate).  Workspaces: qpart cdrl_pwconv_bwd_fused_workspace(G, Mg, N, K, 0) floats,
 * dbpart (..., 1) doubles.  K, N <= 128 and padded alike (both <= 64 or both > 64), even; float32-accurate.
 * act_type = 1: dz, y, a, da are bf16 (bf16 activation storage: one bf16 plane per MFMA operand, i.e. dy,
 * xhat / a and W rounded to nearest even; leading dimensions / offsets even); workspaces sized under the same setting. */
int64_t cdrl_pwconv_bwd_fused_workspace(int G, int Mg, int N, int K, int which, int act_type);
int cdrl_pwconv_bwd_fused(const float* dz, int ld_dz, int dz_coff, int dz_shuffle, int act, const float* y, const float* stats,
                          const float* coef, const float* a, int lda, int a_coff, const float* a_stats, const float* a_gamma,
                          const float* a_beta, float* a_dgamma, float* a_dbeta, float* a_coef, const float* W, const void* W_packed,
                          float* da, int ldda, int da_coff, int accumulate, float* dW, float* db, float* qpart, double* dbpart, int G,
                          int Mg, int N, int K, int act_type, void* stream);

/* General float32 GEMM C (+)= A B + bias on the bf16 matrix pipe (three-way operand split; the 464 -> 768 head conv of
 * core/architectures.py:170 and its backward-data product).  B_packed: cdrl_gemm_x3_packed_bytes(N, K) bytes written by
 * cdrl_gemm_x3_pack from B(k, n) = B[k * sbk + n * sbn].  K, lda, a_coff multiples of 4, A 16-byte aligned. */
int64_t cdrl_gemm_x3_packed_bytes(int N, int K);
int cdrl_gemm_x3_pack(const float* B, int K, int N, int sbk, int sbn, void* packed, void* stream);
int cdrl_gemm_x3(const float* A, int lda, int a_coff, const void* B_packed, const float* bias, float* C, int ldc, int c_coff, int M,
                 int N, int K, int accumulate, int act_type, void* stream);

/* bf16 path (BASELINE.json configuration 3), first kernel: the unit's 1x1 convolution (core/architectures.py:130,140) with
 * bf16 activations in HBM, float32 master weights / bias, v_mfma_f32_32x32x16_bf16 with float32 accumulate.  A [G*Mg][lda]
 * bf16 (+ a_coff), C [G*Mg][ldc] bf16; pro_stats ([4][G][K] float32 or NULL): BatchNorm-apply of the previous layer on load;
 * part ([G][rows][2][N] double or NULL, rows = cdrl_pwconv_bf16_partial_rows): (sum, sum of squares) of the ROUNDED outputs
 * per channel for the following BatchNorm.  K, N <= 128; K, lda, a_coff multiples of 4.
 * W_packed (optional): the weights as bf16 MFMA fragments, written once per weight version by cdrl_pwconv_bf16_pack
 * (cdrl_pwconv_bf16_packed_elems(K) bf16 elements); with it a workgroup's weight prologue is 8 x 16-byte loads per lane. */
int cdrl_f32_to_bf16(const float* x, void* y, int64_t n, void* stream);
int cdrl_bf16_to_f32(const void* x, float* y, int64_t n, void* stream);
int cdrl_pwconv_bf16_partial_rows(int G, int Mg, int N, int K);
int64_t cdrl_pwconv_bf16_packed_elems(int K);
int cdrl_pwconv_bf16_pack(const float* W, int K, int N, void* packed, void* stream);
int cdrl_pwconv_bf16(const void* A, int lda, int a_coff, const float* pro_stats, const float* W, const void* W_packed,
                     const float* bias, void* C, int ldc, int c_coff, int G, int Mg, int N, int K, double* part, void* stream);

/* One time step of the Keras GRU v2 cell (reset_after=True, gates z, r, h; reference core/networks.py:47-50 ->
 * keras.layers.GRU(unroll=True)) as ONE kernel per direction.  xp = x K + b0 of the step [B][3u], hprev [B][u], R [u][3u],
 * b1 [3u]; saved for the backward: z, r, hh [B][u] and hp = hprev R + b1 [B][3u].  Backward: dh [B][ld_dh] gradient w.r.t.
 * the step's output, RT = R^T [3u][u]; outputs dxp (gradient w.r.t. xp), dhp (gradient w.r.t. hp), dhprev (may be null). */
int cdrl_gru_step_fwd(const float* xp, const float* hprev, const float* R, const float* b1, float* z, float* r, float* hh,
                      float* hp, float* hnew, int B, int u, void* stream);
int cdrl_gru_step_bwd(const float* dh, int ld_dh, const float* z, const float* r, const float* hh, const float* hp,
                      const float* hprev, const float* RT, float* dxp, float* dhp, float* dhprev, int B, int u, void* stream);

/* Minibatch assembly: utils.data_to_batches' tf.data gather of the shuffled rollout rows
 * (rl/utils.py:365-393); dst[i, :] = src[idx[i], :], idx = int32 device array of row numbers. */
int cdrl_gather_rows(const float* src, const int32_t* idx, float* dst, int nrows, int64_t row_elems, void* stream);

/* Minibatches from a device-resident trace set (rl/trace_set.py): ONE launch writes `rows` output rows of up to 8
 * keys.  A key's source is an array of slots, slot s at src + s * src_stride elements, row_elems (<= src_stride) elements of it
 * read; one slot is one time step's row.  code: CDRL_TRACE_F32 the floats themselves; CDRL_TRACE_F16 IEEE halves, widened exactly
 * (a NaN keeps its sign and its ten payload bits); CDRL_TRACE_U8 bytes that index `palette`, 256 float32 bit patterns (device
 * memory; -0.0 and +0.0 are two entries, NaN payloads survive: a lookup, no arithmetic).  dst: [rows][T][row_elems] float32.
 * With r = index[offset + i], frame t of output row i is slot max(slot[r] - (T - 1 - t), lo[r]): slot[r] the slot of the row's own
 * step, lo[r] the lowest slot its window may reach (the first slot of its trace: the first frame repeats, as traces.window_index;
 * slot[r] - (T - 1) for a trace stored with its time axis as T slots per row).  direct != 0: the key is indexed by r itself (a
 * matrix of per-row columns, or with src_stride > row_elems a column range of one), T must be 1 and slot / lo are not read.
 * index, slot, lo: device int32; duplicates allowed.  An index outside 0 .. set_rows - 1 is clamped into it so that no read
 * leaves the tables: the kernel cannot report it, the caller checks indices before it uploads them.  16-byte loads and stores per
 * key when row_elems and src_stride are multiples of 4 (float32), 8 (half), 16 (bytes) and src and dst are 16-byte aligned;
 * element accesses otherwise.  No host synchronisation.
 * -1 and cdrl_last_error, before any launch: a null keys / index / src / dst (palette for a byte key; slot / lo with a key that is
 * not direct), nkeys outside 1..8, rows outside 1..65535, T outside 1..16, an unknown code, row_elems < 1 or > src_stride,
 * set_rows < 1, offset < 0, a direct key with T != 1. */
enum { CDRL_TRACE_F32 = 0, CDRL_TRACE_F16 = 1, CDRL_TRACE_U8 = 2 };
typedef struct cdrl_traceset_key {
    const void *src;
    const float *palette;
    float *dst;
    int64_t row_elems;
    int64_t src_stride;
    int32_t code;
    int32_t T;
    int32_t direct;
    int32_t reserved;
} cdrl_traceset_key;
int cdrl_traceset_batch(const cdrl_traceset_key* keys, int nkeys, const int32_t* slot, const int32_t* lo, const int32_t* index,
                        int64_t offset, int rows, int set_rows, void* stream);

/* ---- op-level entry points (Keras layer call -> one launch; used by the parity tests) -------- */
/* Conv2D(k=1) / Dense forward: C[M,N] (+)= A[M,K] B[K,N] + bias (core/architectures.py:130,134,140,170) */
int cdrl_gemm_nn(const float* A, int lda, int a_coff, const float* B, int sbk, int sbn, const float* bias, float* C,
                 int ldc, int c_coff, int M, int N, int K, int accumulate, void* stream);
int64_t cdrl_gemm_tn_workspace_elems(int M, int N, int K);
int cdrl_gemm_tn(const float* A, int lda, int a_coff, const float* D, int ldd, int d_coff, float* out, int M, int N,
                 int K, float* workspace, int accumulate, int act_type, void* stream);
/* Conv2D(24, 3, strides=2) stem (core/architectures.py:159) */
int cdrl_stem_fwd(const float* x, const float* w, const float* bias, float* y, int B, int T, int H, int W, int Cout,
                  void* stream);
/* The same conv with the statistics of the BatchNorm behind it in the epilogue (what the engine runs in training; conv.hip
 * stem_fwd_band_kernel: the image band staged in LDS, or the window form with CDRL_STEM_FWD_BAND=0): y bit-identical to cdrl_stem_fwd,
 * part [T][rows][2][Cout] doubles = per-workgroup (sum y, sum y^2) per time slice, rows = cdrl_stem_fwd_stats_rows(), the layout
 * cdrl_bn_train_fwd's finalize consumes.  Cout % 4 == 0, <= 64; y 16-byte aligned.  Replaces Conv2D(stem) + the moments of its
 * BatchNormalization (core/architectures.py:159-160). */
int cdrl_stem_fwd_stats_rows(int B, int T, int H, int W, int Cout);
int cdrl_stem_fwd_stats(const float* x, const float* w, const float* bias, float* y, double* part, int B, int T, int H, int W, int Cout,
                        int act_type, void* stream);
int64_t cdrl_stem_bwd_workspace_doubles(int B, int T, int H, int W, int Cout);
int cdrl_stem_bwd_filter(const float* x, const float* dy, float* dw, float* db, int B, int T, int H, int W, int Cout,
                         double* workspace, void* stream);
/* DepthwiseConv2D(3, strides, 'same') (core/architectures.py:132,138) */
int cdrl_dwconv_fwd(const float* a, const float* w, const float* bias, float* y, int N, int H, int W, int C, int stride,
                    void* stream);
int cdrl_dwconv_bwd_data(const float* dy, const float* w, float* da, int N, int H, int W, int C, int stride, void* stream);
int64_t cdrl_dwconv_bwd_workspace_doubles(int N, int H, int W, int C, int stride);
int cdrl_dwconv_bwd_filter(const float* a, const float* dy, float* dw, float* db, int N, int H, int W, int C, int stride,
                           double* workspace, void* stream);
/* Pointwise Conv2D(k=1) of the ShuffleNet unit (core/architectures.py:130,140) as a persistent skinny GEMM for
 * K, N <= 128 with the neighbouring per-time-slice BatchNormalization folded in.  Rows: G groups of Mg rows.
 *   pro_stats != NULL (4*G*K block of the previous BN): a <- scale[g][k]*a + shift[g][k] on load;
 *   epilogue 1: part[g][b][2][N] = (sum c, sum c^2) of the output -> statistics of the following BN;
 *   epilogue 2: part[g][b][2][N] = (sum c, sum c*xhat) with xhat = (epi_y - mean)*invstd from epi_stats (4*G*N):
 *               BN-backward sums when c is the gradient w.r.t. that BN's output (backward-data GEMM, B = W^T via
 *               sbk/sbn as in cdrl_gemm_nn).
 * b < cdrl_pwconv_fused_partial_rows(G, Mg, N, K); returns -1 (cdrl_last_error) for unsupported shapes/alignment. */
int cdrl_pwconv_fused_partial_rows(int G, int Mg, int N, int K);
int cdrl_pwconv_fused(const float* a, int lda, int a_coff, const float* pro_stats, const float* w, int sbk, int sbn,
                      const float* bias, float* c, int ldc, int c_coff, int accumulate, int G, int Mg, int N, int K,
                      int epilogue, const float* epi_y, const float* epi_stats, double* part, void* stream);
/* Same operator with the weights pre-packed in MFMA fragment order (cdrl_pwconv_pack: cdrl_pwconv_pack_elems(N, K) floats of
 * space, written once per weight version from B(k, n) = W[k * sbk + n * sbn]).  packed_bf16 = 0: float32 fragments, results
 * bit-identical to cdrl_pwconv_fused.  packed_bf16 = 1 (cdrl_pwconv_pack(..., bf16 = 1)): the bf16-OPERAND compute mode of
 * configuration 3 (BASELINE.json configs[2]) -- both MFMA operands are rounded to bf16 (round-to-nearest-even: A after the
 * prologue on its way into LDS, W at pack time), the product runs as v_mfma_f32_32x32x16_bf16 with float32 accumulation;
 * tensors in HBM, bias, statistics and epilogues stay float32.  Reference layer: core/architectures.py:130,140. */
int64_t cdrl_pwconv_pack_elems(int N, int K);
int cdrl_pwconv_pack(const float* W, int K, int N, int sbk, int sbn, float* packed, int bf16, void* stream);
int cdrl_pwconv_fused_packed(const float* a, int lda, int a_coff, const float* pro_stats, const float* w, int sbk, int sbn,
                             const float* bias, float* c, int ldc, int c_coff, int accumulate, int G, int Mg, int N, int K,
                             int epilogue, const float* epi_y, const float* epi_stats, double* part, const float* w_packed,
                             int packed_bf16, int act_type, void* stream);
/* Backward of [Conv2D(k=1) -> BatchNormalization(training, per time slice) (+ReLU6) (+channel_shuffle on the store)]
 * (core/architectures.py:130-131,140-145) without materialising the gradient w.r.t. the conv output: the BN-backward
 * "apply" runs as the operand prologue of the two GEMMs.  dout: gradient w.r.t. the BN output (view ld/coff, read through
 * the shuffle map when shuffle_ctot != 0); y: raw conv output [G*Mg][N]; stats: that BN's 4*G*N block; x: conv input
 * view [G*Mg][K]; x_pro_stats != NULL: the conv input is BN-apply(x) with those statistics (4*G*K) as in
 * cdrl_pwconv_fused.  Outputs: dgamma, dbeta, coef (3*G*N scratch), dx (view, accumulate flag), dw (K x N), db (N).
 * workspace: cdrl_pwconv_bn_bwd_workspace_bytes().  Shapes as cdrl_pwconv_fused (K, N <= 128, even). */
int64_t cdrl_pwconv_bn_bwd_workspace_bytes(int G, int Mg, int N, int K);
int cdrl_pwconv_bn_bwd(const float* dout, int dout_ld, int dout_coff, int shuffle_ctot, int relu6, const float* y,
                       const float* stats, const float* x, int x_ld, int x_coff, const float* x_pro_stats, const float* w,
                       int G, int Mg, int N, int K, float* dgamma, float* dbeta, float* coef, float* dx, int dx_ld,
                       int dx_coff, int accumulate, float* dw, float* db, void* workspace, int act_type, void* stream);
/* ... with the backward-data operand W^T pre-packed: cdrl_pwconv_pack(W, N, K, 1, N, wt_packed, bf16) packs
 * B(k = n_out, n = k_in) = W[k_in * N + n_out]; packed_bf16 = 1 runs the backward-data GEMM AND the filter-gradient GEMM in the
 * bf16-operand mode (dz rounded to bf16 after the BatchNorm-backward prologue, x after its BatchNorm-apply prologue); db,
 * dgamma, dbeta are float32 reductions. */
int cdrl_pwconv_bn_bwd_packed(const float* dout, int dout_ld, int dout_coff, int shuffle_ctot, int relu6, const float* y,
                              const float* stats, const float* x, int x_ld, int x_coff, const float* x_pro_stats, const float* w,
                              int G, int Mg, int N, int K, float* dgamma, float* dbeta, float* coef, float* dx, int dx_ld,
                              int dx_coff, int accumulate, float* dw, float* db, void* workspace, const float* wt_packed,
                              int packed_bf16, int act_type, void* stream);
/* Fused depthwise block of the ShuffleNet unit: [BatchNormalization + ReLU6 of the previous 1x1 conv, applied on
 * load] -> DepthwiseConv2D(3, stride, 'same') -> statistics of the BatchNormalization that follows
 * (core/architectures.py:130-139; per-time-slice BN :44-57).  Whole frames are staged in LDS; the normalised
 * depthwise input is never written to memory.  x: [G*B frames][H][W][C] raw output of the previous conv
 * (pre_stats = that BN's 4*G*C statistics block from cdrl_bn_train_fwd / this function) or, with pre_stats = NULL,
 * an activation tensor used as is.  Outputs: y (raw depthwise output), post_stats (4*G*C) of the following BN
 * (moving statistics updated as in cdrl_bn_train_fwd). */
int64_t cdrl_dwconv_bn_workspace_doubles(int G, int B, int H, int W, int C, int stride);
int cdrl_dwconv_bn_fwd(const float* x, const float* pre_stats, const float* w, const float* bias, float* y, int G, int B,
                       int H, int W, int C, int stride, const float* gamma, const float* beta, float* moving_mean,
                       float* moving_var, int bessel, float* post_stats, double* workspace, int act_type, void* stream);
/* Backward of the same block.  dout: gradient w.r.t. the OUTPUT of the following BatchNormalization (no activation);
 * y: raw depthwise output.  Produces dw (3,3,C,1), db, the following BN's dgamma/dbeta (+ coef_post, 3*G*C scratch)
 * and dx = gradient w.r.t. x; with pre_stats != NULL the previous BN(+ReLU6) is back-propagated too
 * (dgamma_pre, dbeta_pre, coef_pre 3*G*C scratch) so that dx is the gradient w.r.t. the raw conv output x. */
int cdrl_dwconv_bn_bwd(const float* x, const float* pre_stats, const float* dout, const float* y, const float* post_stats,
                       const float* w, int G, int B, int H, int W, int C, int stride, float* dx, float* dw, float* db,
                       float* dgamma_post, float* dbeta_post, float* coef_post, float* dgamma_pre, float* dbeta_pre,
                       float* coef_pre, double* workspace, int act_type, void* stream);
/* Read-only query of the plan cdrl_dwconv_bn_fwd / _bwd launch from for (G, B, H, W, C, stride): which kernel instantiation runs,
 * with which loop structure, grid and LDS.  Launches nothing and changes nothing.  Writes the first min(n_out, count) of these
 * int32 fields to `out` (host memory) and returns their count, or -1 for a bad stride, a bad shape or a null `out`.
 * cdrl_dwconv_bn_plan reports fields 0..21 (count 22, as its callers size their arrays), cdrl_dwconv_bn_plan_ex all of them (31):
 *    0 vec        forward: channels per thread (1 | 2 | 4)
 *    1 nch        forward and pixel-mapped backward: channel chunks per frame
 *    2 cchunk     channels per chunk
 *    3 cy         forward: pixel lanes per workgroup
 *    4 fpb        forward (and pixel-mapped backward): frames looped per workgroup
 *    5 nb         forward: partial rows per group (B / fpb)
 *    6 vec_bwd    pixel-mapped backward: channels per thread (1 | 2)
 *    7 fpb_bwd    backward: frames looped per workgroup
 *    8 nb_bwd     backward: partial rows per group (B / fpb_bwd)
 *    9 form       backward form: 0 pixel-mapped, 1 stride-1 strips, 2 stride-2 strips
 *   10 strip_sw   strip form: pixels per strip (8 | 4); fields 10..14, 21..23 and 28 are 0 in the pixel-mapped form
 *   11 strip_R    strips per thread and tile batch (1 | 2 | 3; stride 2: 1)
 *   12 strip_F    frames sharing one tile batch (1 | 2 | 4 | 8)
 *   13 strip_nch  channel chunks per frame
 *   14 strip_cy   strip lanes per workgroup (threads = strip_cx * strip_cy)
 *   15 pl         left 'same' padding of a stride-2 row, same_pad_before(W, 2): picks the stride-2 strip kernel's PL
 *   16 lds_bwd_over    1: the pixel-mapped backward's tile exceeds the LDS limit -- with form 0, cdrl_dwconv_bn_bwd refuses the shape
 *   17 lds_fwd_over    1: the forward's tile exceeds the LDS limit -- cdrl_dwconv_bn_fwd refuses the shape
 *   18 cx         forward: channel lanes per workgroup
 *   19 cx_bwd, 20 cy_bwd   pixel-mapped backward: channel / pixel lanes per workgroup
 *   21 strip_cx   strip form: channel-pair lanes per workgroup
 *   22 strip_cchunk    strip form: channels per chunk (2 * strip_cx)
 *   23 strip_S    strip form: strips per pixel row
 *   24 lds_fwd    forward: dynamic LDS bytes
 *   25 lds_bwd    backward, the form that runs: dynamic LDS bytes
 *   26 grid_fwd, 27 grid_bwd   workgroups of the forward / of the backward form that runs
 *   28 strip_tile strip form: bytes of the gradient tile (without the coefficient table behind it)
 *   29 refusal_fwd, 30 refusal_bwd   0, or why cdrl_dwconv_bn_fwd / _bwd refuse the shape: 2 the tile exceeds the LDS limit (fields
 *                 17 / 16 with form 0), 3 strip form with a gradient view of 2 GB or more (never with the dense dx of these entries) */
int cdrl_dwconv_bn_plan(int G, int B, int H, int W, int C, int stride, int32_t* out, int n_out);
int cdrl_dwconv_bn_plan_ex(int G, int B, int H, int W, int C, int stride, int32_t* out, int n_out);
/* MaxPooling2D(3, 2, 'same') (core/architectures.py:161) */
int cdrl_maxpool_fwd(const float* a, float* p, uint8_t* argmax, int N, int H, int W, int C, void* stream);
int cdrl_maxpool_bwd(const uint8_t* argmax, const float* dp, float* da, int N, int H, int W, int C, void* stream);
/* BatchNormalization(training=True) per time slice + optional ReLU6 + optional channel_shuffle on
 * the store (core/architectures.py:44-57,109-118).  stats: 4*G*C floats, workspace: G*256*2*C doubles. */
int cdrl_bn_train_fwd(const float* y, int G, int Mg, int C, const float* gamma, const float* beta, float* moving_mean,
                      float* moving_var, int bessel, int relu6, float* out, int out_ld, int out_coff, int shuffle_ctot,
                      float* stats, double* workspace, int act_type, void* stream);
/* Single-group BatchNorm over a few hundred rows (the dense BatchNorms of the trunk tail and of control_branch,
 * core/networks.py:59-66, :53-54) as ONE launch per direction: statistics + moving-average update + apply (forward),
 * sums + coefficients + apply (backward).  y / out / dout / dx dense [M][C]; stats 4*C, coef 3*C floats. */
int cdrl_bn_small_fwd(const float* y, int M, int C, const float* gamma, const float* beta, float* moving_mean,
                      float* moving_var, float* stats, float* out, void* stream);
int cdrl_bn_small_bwd(const float* dout, const float* y, int M, int C, const float* stats, float* dgamma, float* dbeta,
                      float* coef, float* dx, void* stream);
/* Backward of TWO such BatchNorms A and B that normalise the same input y (pi.bn0 and v.bn0 of the joint update, both over the
 * trunk output) as one launch: dgamma / dbeta / coef of either are bit-identical to a cdrl_bn_small_bwd call on it alone (same
 * geometry, same fixed reduction order, no atomics), and dx[r][c] = dxA + dxB, each term formed exactly as cdrl_bn_small_bwd
 * forms it and the two joined by one float32 addition.  All tensors dense; statsA / statsB as cdrl_bn_small_fwd leaves them. */
int cdrl_bn_small_bwd_pair(const float* doutA, const float* doutB, const float* y, int M, int C, const float* statsA,
                           const float* statsB, float* dgammaA, float* dbetaA, float* coefA, float* dgammaB, float* dbetaB,
                           float* coefB, float* dx, void* stream);
/* The linear output heads of a control branch (core/networks.py:128-137, :267-275: up to 4 Dense(K -> n_h) layers on the
 * same [B][K] activation, 8 outputs in total) as one launch per direction.  w[h]: [K][n[h]], b[h]: [n[h]];
 * lin / dlin: [B][sum n]; backward: da [B][K] (overwritten), dw[h], db[h]. */
int cdrl_linear_heads_fwd(const float* a, int nheads, const int* n, const float* const* w, const float* const* b, float* lin,
                          int B, int K, void* stream);
int cdrl_linear_heads_bwd(const float* a, int nheads, const int* n, const float* const* w, const float* dlin, float* da,
                          float* const* dw, float* const* db, int B, int K, void* stream);
int cdrl_bn_train_bwd(const float* dout, int dout_ld, int dout_coff, int shuffle_ctot, const float* y, int G, int Mg,
                      int C, const float* stats, int relu6, float* dgamma, float* dbeta, float* dy, float* coef,
                      double* workspace, int act_type, void* stream);
/* ---- The BatchNorm family with the argument forms the engine runs it with (csrc/bn.hip: bn_apply, bn_bwd_reduce, bn_bwd_finalize,
 * bn_bwd_apply, bn_act_gap_fwd, gather_view, bn_inference_stats_many).  Thin wrappers; every one takes `act_type` explicitly where the
 * host function has one.
 * A view: element (row r, channel c) of the tensor lives at p[r*ld + coff + c], ld and coff counted in elements of the tensor's type
 * (float32, or bf16 with act_type = 1).  A view written or read "through the shuffle" of a ctot-channel tensor maps concat index
 * i = coff + c to column (i & 1) * (ctot / 2) + (i >> 1) (channel_shuffle, core/architectures.py:109-118). */
typedef struct cdrl_view {
    void* p;
    int32_t ld, coff;
} cdrl_view;
/* out = [relu6](scale * y + shift) of the stats block (4*G*C: mean, invstd, scale, shift), stored plain (shuffle_ctot = 0) or through the
 * shuffle; pass_src / pass_dst (both or neither): a second tensor of the same C channels copied through the same store (the unit's
 * identity half).  stats = NULL: copy only, float32, no activation. */
int cdrl_bn_apply(const cdrl_view* y, int G, int Mg, int C, const float* stats, int relu6, const cdrl_view* out, int shuffle_ctot,
                  const cdrl_view* pass_src, const cdrl_view* pass_dst, int act_type, void* stream);
/* Backward of the same: sums -> dgamma, dbeta, coef (3*G*C) -> dy (dense [G*Mg][C]).  dout is read plain or through the shuffle;
 * pass_gsrc (read through the same shuffle) -> pass_gdst (plain): the identity half's gradient, copied in the same pass.
 * bcast_rows > 0: dout is a float32 tensor with ONE row per bcast_rows rows of y, divided by bcast_rows on load (the gradient of a
 * global average pool; Mg % bcast_rows == 0, no shuffle, no pass-through).
 * workspace: 3*G*nb*C doubles, nb = field 16 of cdrl_bn_plan (<= 128): [G][nb][2][C] partial (sum dz, sum dz*xhat), then [G][nb][C]
 * partial column sums of dy. */
int cdrl_bn_bwd(const cdrl_view* dout, int shuffle_ctot, const cdrl_view* y, int G, int Mg, int C, const float* stats, int relu6,
                float* dgamma, float* dbeta, float* dy, float* coef, double* workspace, const cdrl_view* pass_gsrc,
                const cdrl_view* pass_gdst, int bcast_rows, int act_type, void* stream);
/* What the launchers of cdrl_bn_apply / cdrl_bn_bwd dispatch on for these arguments (they call the same host functions): launches
 * nothing, reads no memory (the views' pointers only count for their alignment).  Writes min(n_out, 30) int32 fields and returns 30:
 * three plans of 10 fields -- 0-9 forward apply, 10-19 backward reduce, 20-29 backward apply:
 *   +0 form   0: generic kernel (vcolreduce skeleton), 1: fast kernel (bn_apply_shuf_kernel, bn_bwd_reduce_shuf_kernel,
 *             bn_bwd_apply_fast_kernel)
 *   +1 vec    channels per thread: 4 (C % 4 == 0), 2 (C even), 1
 *   +2 cx     channel lanes per workgroup, min(C / vec, 256)
 *   +3 cy     row lanes per workgroup, max(256 / cx, 1)
 *   +4 nloop  channel-lane passes, > 1 when C / vec > 256 (generic kernel only)
 *   +5 rb     rows per workgroup (a multiple of cy, at least 2 cy)
 *   +6 nb     workgroups per group: the partial rows of the backward
 *   +7..+9    alignment flags handed to the generic kernel -- apply: y, out, pass_src; reduce: dout, y, pass_gdst;
 *             backward apply: dout, y, dy (form 0 refuses a dy that is not aligned) */
int cdrl_bn_plan(const cdrl_view* y, const cdrl_view* out, const cdrl_view* dout, int shuffle_ctot, int G, int Mg, int C, int has_stats,
                 int relu6, const cdrl_view* pass_src, const cdrl_view* pass_dst, const cdrl_view* pass_gsrc, const cdrl_view* pass_gdst,
                 const float* dy, int bcast_rows, int act_type, int32_t* fields, int n_out);
/* ---- The fused 1x1-conv backward (cdrl_pwconv_bwd_fused above) with the argument forms the engine runs it with.
 * cdrl_pwconv_bwd_plan: what the launchers dispatch on for these arguments (they call the same host function) -- launches nothing, reads
 * no memory: the views' pointers count for their alignment, the other pointers for being null or not (any non-null value probes).
 * Writes min(n_out, 18) int32 fields and returns 18 (-1: no view struct, bad act_type):
 *    0 ok       1: the call would run; 0: refused, field 1 says why and cdrl_last_error() holds the sentence
 *    1 refusal  1 shape (K, N even in 8..128, not padded 128 -> 64; G, Mg >= 1), 2 parity / alignment (even ld / coff, 8-byte aligned
 *               pointers), 3 bf16 storage with K and N padded differently, 4 an operand of 2 GB or more, 5 G > 8, 6 finalize-on-load
 *               under bf16 storage / fin_nb < 1 / without fin_tot / without o_dgamma, o_dbeta, 7 a_stats without gamma, beta or an output
 *    2 form     0 float32 tensors, 1 bf16 storage
 *    3 kp  4 np padded input / output channels (64 | 128)     5 bm rows per tile (64 for 64/64, else 32)     6 tiles = ceil(Mg / bm)
 *    7 nbpg     workgroups (partial tiles) per group: min(tiles, 256 / G), or 512 / G under bf16 storage once tiles >= 6 * (512 / G)
 *    8 wp_ks    K = 16 steps per plane of W_packed (2 for N <= 32, 4 for N <= 64, 8)
 *    9 shuf  10 anorm  11 acc  the kernel instantiation      12 fin finalize-on-load     13 coef_needed (0 with fin: coef may be NULL)
 *   14 lds_bytes  15 qpart floats  16 dbpart doubles  17 spart_offset: doubles into dbpart where the directly accumulated BatchNorm sums
 *               of the bf16-storage form with a_stats start (0 otherwise) */
int cdrl_pwconv_bwd_plan(const cdrl_view* dz, int dz_shuffle, const cdrl_view* a, const cdrl_view* da, int accumulate, int G, int Mg, int N,
                         int K, const float* a_stats, const float* a_gamma, const float* a_beta, const float* a_dgamma, const float* a_dbeta,
                         const float* a_coef, const double* fin_part, int fin_nb, const double* fin_tot, const float* o_dgamma,
                         const float* o_dbeta, int act_type, int32_t* fields, int n_out);
/* cdrl_pwconv_bwd_fused with dz, a, da as views, plus FINALIZE-ON-LOAD (float32 tensors; the engine's default): fin_part != NULL holds the
 * [G][fin_nb][2][N] backward sums (sum mask dz, sum mask dz xhat(y)) of the BatchNorm behind the conv; the kernel folds them into
 * k2 = mean, k3 = mean itself, takes k1 from the scale row of `stats` (coef may be NULL), leaves the group totals in fin_tot [G][2][N]
 * doubles, and the reduce writes that BatchNorm's o_dgamma / o_dbeta [N].  Every view must keep its channels inside its rows (dz: through
 * the shuffle when dz_shuffle != 0); a refused call launches nothing. */
int cdrl_pwconv_bwd_fused_fin(const cdrl_view* dz, int dz_shuffle, int act, const float* y, const float* stats, const float* coef,
                              const cdrl_view* a, const float* a_stats, const float* a_gamma, const float* a_beta, float* a_dgamma,
                              float* a_dbeta, float* a_coef, const float* W, const void* W_packed, const cdrl_view* da, int accumulate,
                              float* dW, float* db, float* qpart, double* dbpart, const double* fin_part, int fin_nb, double* fin_tot,
                              float* o_dgamma, float* o_dbeta, int G, int Mg, int N, int K, int act_type, void* stream);
/* ---- The filter-gradient GEMM family  out[K][N] (+)= sum_m a'[m][K]^T d'[m][N]  (cdrl_gemm_tn above is its plain G = 1 form) with the
 * whole contract of the engine's calls: rows in G equal groups; a' = scale[g][k] a + shift[g][k] from a_stats [4][G][K] (or a);
 * d' = k1 (mask(dz) - k2 - xhat(y) k3) with dz = view d (gathered through the channel shuffle of a shuffle_ctot-channel tensor when
 * shuffle_ctot != 0), y dense [M][N], mean / invstd / scale / shift from dpro_stats [4][G][N], k1..k3 from dpro_coef [3][G][N], the
 * ReLU6 mask 0 < fmaf(scale, y, shift) < 6 with relu6 (or d' = d when dpro_y is NULL).  bf16_operands: a' and d' are rounded to bf16 after
 * their float32 prologues; act_type 1 (a, d, y are bf16 tensors) needs it.
 * cdrl_gemm_tn_plan: what gemm_tn dispatches on for these arguments (the launcher calls the same host function) -- launches nothing, reads
 * no memory: only ld / coff of the views count.  Writes min(n_out, 21) int32 fields and returns 21 (-1: bad act_type, no field array):
 *    0 ok       1: the call would run; 0: refused, field 1 says why and cdrl_last_error() holds the sentence
 *    1 refusal  1 G < 1 or M not a multiple of G, 2 act_type 1 without bf16_operands, 3 an operand of 2 GB or more (M * ld * 4 bytes),
 *               4 a view whose channels do not fit its rows, or shuffle / relu6 without the D prologue
 *    2 kernel   0 tn_direct_kernel, 1 tn_direct_tr_kernel (exactly with the D prologue), 2 tn_lds_kernel (K, N >= 96, even ld / coff / K /
 *               N, shuffle_ctot / 2 even); -1: M, N or K < 1, nothing to launch
 *    3 mode     direct: 0 float32, 1 bf16 operands, 2 bf16 tensors; LDS: 0 float32 MFMA (CDRL_TN_LDS_F32=1), 1 bf16 operands, 2 bf16
 *               tensors, 3 three bf16 planes per operand (float32 tensors, the default)
 *    4 apro  5 dpro  6 NJW  7 WK  8 NSPL  9 RS  10 RS2  11 U   the instantiation and wave mapping of the direct kernels (6..11 are 0 for LDS)
 *   12 gy  13 gz  14 nspg  15 nsplit = G * nspg (grid x)  16 rows_per workgroup  17 part_slots  18 part_elems = part_slots * K * N
 *   19 reduce_form (cdrl_reduce_partials_plan, 16-byte aligned workspace)  20 dhalf: an LDS-kernel thread gathers the pair (s - 1, s) */
int cdrl_gemm_tn_plan(const cdrl_view* a, const cdrl_view* d, int M, int N, int K, int G, int has_a_stats, int has_dpro, int shuffle_ctot,
                      int relu6, int bf16_operands, int act_type, int32_t* fields, int n_out);
/* floats of workspace cdrl_gemm_tn_ex needs for any prologue / operand type (0 for a shape it refuses) */
int64_t cdrl_gemm_tn_ex_workspace_elems(int M, int N, int K, int G);
int cdrl_gemm_tn_ex(const cdrl_view* a, const float* a_stats, const cdrl_view* d, const float* dpro_y, const float* dpro_stats,
                    const float* dpro_coef, int shuffle_ctot, int relu6, float* out, int M, int N, int K, int G, float* workspace,
                    int accumulate, int bf16_operands, int act_type, void* stream);
/* out[i] (+)= float(sum_p part[p * stride + i]), i < n: the reduce behind every split-M float partial (double sums, fixed order).
 * The plan writes min(n_out, 4) fields and returns 4: form (0 few partials, float4; 1 / 2 / 3 float4 with 16 / 4 / 1 column lanes;
 * 4 / 5 scalar with 16 / 4 column lanes -- any alignment), grid, block x, block y.  -1: nparts < 1, n < 1 or stride < n. */
int cdrl_reduce_partials_plan(uint64_t part_addr, int nparts, int64_t n, int64_t stride, int32_t* fields, int n_out);
int cdrl_reduce_partials_f32(const float* part, int nparts, int64_t n, int64_t stride, float* out, int accumulate, void* stream);

/* ---- The dense GEMM family  c[M][N] (+)= a[M][K] B(k, n) + bias[n],  B(k, n) = B[k * sbk + n * sbn]  (cdrl_gemm_nn above is its form without
 * workspace), with the whole contract of the engine's calls: a and c are views; workspace (cdrl_gemm_nn_workspace_elems floats, or NULL)
 * allows split-K; act_out (dense [M][N], or NULL) with act (0 none, 1 relu6, 2 swish6, 3 tanh, 4 sigmoid) and act_done (or NULL): when
 * the product goes through split-K and act_done is given, the reduce also writes act(c) to act_out and sets *act_done = 1; otherwise
 * *act_done = 0, act_out is not touched and the caller runs cdrl_act_fwd.  Refused (-1, cdrl_last_error) before any launch: a view
 * whose columns do not fit its rows, null a / B / c, act_out without workspace, an act outside 0..4.
 * cdrl_gemm_nn_plan: what gemm_nn dispatches on for these arguments (the launcher calls the same host function) -- launches nothing,
 * reads no memory: only the address bits, ld and coff count.  Writes min(n_out, 14) int32 fields and returns 14 (-1: no field array, or
 * the K columns of a do not fit its rows):
 *    0 kernel   -1 M or N < 1: nothing to launch; 0 gemm_nn_kernel; 1 gemm_nn_rt_kernel (M >= 2048, N >= 129, K >= 64, a16 and b16);
 *               2 split-K (workspace, M <= 2048, K >= 256, even NT, gz >= 2): gemm_nn_kernel over gz slabs, then splitk_reduce_kernel
 *    1 NT  2 WR  3 BT  4 VEC   the instantiation gemm_nn_kernel<NT, BT, VEC, WR>, (NT, WR) one of (1, 4), (3, 4), (2, 2), (4, 2); BT: sbn != 1;
 *               VEC: 8-byte loads of a (K, ld, coff even, pointer 8-byte aligned).  Kernel 1: gemm_nn_rt_kernel<NT = 3, BT>, WR = VEC = 0
 *    5 gx  6 gy  7 gz (K splits; 1 without split-K)  8 kchunk (K range of one split, a multiple of 32; 1 << 30 without split-K)
 *    9 ws_elems = gz * M * N floats the split writes (0 without)  10 reduce_grid  11 act_fused (the reduce can write act_out)
 *   12 a16  13 b16   16-byte alignment of the rows of a (K, ld, coff multiples of 4, pointer) / of the weight rows */
int cdrl_gemm_nn_plan(const cdrl_view* a, uint64_t b_addr, int sbk, int sbn, int M, int N, int K, int has_workspace, int32_t* fields,
                      int n_out);
int64_t cdrl_gemm_nn_workspace_elems(int M, int N, int K);
int cdrl_gemm_nn_ex(const cdrl_view* a, const float* B, int sbk, int sbn, const float* bias, const cdrl_view* c, int M, int N, int K,
                    int accumulate, float* workspace, float* act_out, int act, int* act_done, void* stream);
/* ---- The 1x1-conv forward / backward-data family: the plans cdrl_pwconv_fused[_packed] / cdrl_pwconv_bn_bwd (pw_nn), cdrl_pwconv_x3 and
 * cdrl_pwconv_x3_wide_bwd launch from (the launchers call the same host functions).  The queries launch nothing and read no memory: only
 * the address bits, ld and coff of the views count, and whether an operand is given.  Each takes an array of EXACTLY its number of int32
 * fields, writes all of them, and returns 0 when the call would be launched, -1 with the refusal sentence in cdrl_last_error when it
 * would be refused (field 1 then holds the refusal code) or when a view / the field array is missing.
 * cdrl_pwconv_plan (19 fields): a = the operand view (pro == 2: the dz view, and y_addr the address of that prologue's raw BatchNorm
 * input), pro 0 none / 1 BatchNorm apply / 2 BatchNorm backward, epi 0 / 1 statistics / 2 BatchNorm backward sums.
 *    0 ok  1 refusal: 1 G, Mg, N < 1 or K < 2; 2 K or N above 256, K odd; 3 a (ksm, nt) pair that is not instantiated; 4 alignment;
 *      5 prologue / epilogue pair; 6 epilogue without partial buffer; 7 an operand of 2 GB or more; 8 bf16 storage without packed bf16 weights
 *    2 ksm  3 nt  4 pro  5 epi  6 mode  7 acc   pw_nn_kernel<KSM, NT, PRO, EPI, MODE, ACC>
 *    8 wc  9 wr  10 bm (rows per tile)  11 tiles_g  12 nbpg (workgroups = partial rows per group)  13 tpb (most tiles per workgroup)
 *   14 gx  15 gy  16 occ  17 lds_bytes  18 packed_elems
 * cdrl_pwconv_x3_plan (13 fields): nbpg 0 = the kernel's own count, > 0 = the caller's (honoured inside [1, tiles_g], else refused).
 *    0 ok  1 refusal: 1 G, Mg, N < 1; 2 shape; 3 alignment; 4 no packed weights; 5 2 GB; 6 nbpg
 *    2 form (0 persistent, 1 wide)  3 kp  4 nt  5 pro  6 epi  7 bm  8 tiles_g  9 nbpg  10 gx  11 gy  12 packed_bytes
 * cdrl_pwconv_x3_wide_bwd_plan (8 fields): N = conv input channels, K = conv output channels.
 *    0 ok  1 refusal: 1 G, Mg < 1; 2 shape; 3 alignment; 4 operands missing; 5 epilogue and accumulate are not instantiated together; 6 2 GB
 *    2 sh  3 epi  4 acc   pw_x3_wide_bwd_kernel<SH, EPI, ACC>   5 rows (partial rows per group)  6 gx  7 gy */
int cdrl_pwconv_plan(const cdrl_view* a, const cdrl_view* c, uint64_t y_addr, int G, int Mg, int N, int K, int pro, int epi, int accumulate,
                     int packed, int packed_bf16, int act_type, int has_part, int32_t* fields, int n_fields);
/* pw_nn with its whole contract (cdrl_pwconv_fused[_packed] are its forms without the BatchNorm-backward prologue): bwd_y != NULL
 * selects prologue 2 -- a is then the dz view (gathered through the channel shuffle of a bwd_shuffle-channel tensor when != 0, masked by
 * ReLU6 of the BatchNorm output when bwd_relu6), bwd_y that BatchNorm's raw input [G*Mg][K] dense, pro_stats its [4][G][K] statistics,
 * bwd_coef its [3][G][K] backward coefficients, part2 (or NULL) [G][nbpg][K] doubles: column sums of the transformed operand.  Refused
 * (-1, cdrl_last_error) before any launch: whatever cdrl_pwconv_plan refuses, a null tensor, a prologue 2 or epilogue 2 without its operands. */
int cdrl_pwconv_ex(const cdrl_view* a, const float* pro_stats, const float* bwd_y, const float* bwd_coef, int bwd_shuffle, int bwd_relu6,
                   double* part2, const float* w, int sbk, int sbn, const float* bias, const cdrl_view* c, int accumulate, int G, int Mg, int N,
                   int K, int epilogue, const float* epi_y, const float* epi_stats, double* part, const float* w_packed, int packed_bf16,
                   int act_type, void* stream);
int cdrl_pwconv_x3_plan(const cdrl_view* a, const cdrl_view* c, int G, int Mg, int N, int K, int pro, int epi, int packed, int nbpg,
                        int32_t* fields, int n_fields);
int cdrl_pwconv_x3_wide_bwd_plan(const cdrl_view* dz, const cdrl_view* c, int G, int Mg, int N, int K, int dz_shuffle, int epi, int accumulate,
                                 int operands, int32_t* fields, int n_fields);
/* a = act(z), dz = da * act'(z) on dense float32 arrays of n elements (act as above; relu6 gradient 1 strictly inside (0, 6), swish6 =
 * min(z sigmoid(z), 6) with gradient 0 where z sigmoid(z) >= 6) */
int cdrl_act_fwd(const float* z, float* a, int64_t n, int act, void* stream);
int cdrl_act_bwd(const float* z, const float* da, float* dz, int64_t n, int act, void* stream);
/* Bias gradient: part [cdrl_colsum_partial_rows(rows, C)][C] doubles = column sums of row blocks of the view x; cdrl_reduce_partials
 * folds them: out1[i] (+)= float(sum_p part[p * stride + i]) for i < n1, out2[i - n1] likewise for n1 <= i < n1 + n2 (n2 = 0: out2
 * unused).  cdrl_reduce_partials_cx: outputs per block (16 or 4) of the kernel form that call launches. */
int cdrl_colsum_partial_rows(int rows, int C);
int cdrl_colsum(const cdrl_view* x, int rows, int C, double* part, void* stream);
int cdrl_reduce_partials_cx(int nparts, int n1, int n2);
int cdrl_reduce_partials(const double* part, int nparts, int n1, int n2, int64_t stride, float* out1, float* out2, int accumulate,
                         void* stream);
/* (B, T, D) -> (T, B, D): dst[(t * B + b) * D + d] = src[(b * T + t) * D + d] */
int cdrl_permute_bt(const float* src, float* dst, int B, int T, int D, void* stream);
/* out[n][c] (float32) = mean over the P rows of frame n of [relu6](scale * y + shift); y dense [G*frames_per_group*P][C] */
int cdrl_bn_act_gap_fwd(const float* y, const float* stats, float* out, int G, int frames_per_group, int P, int C, int relu6,
                        int act_type, void* stream);
/* dst (plain) = or += src read through the shuffle (shuffle_ctot = 0: plain); float32 */
int cdrl_gather_view(const cdrl_view* src, int shuffle_ctot, int rows, int C, const cdrl_view* dst, int accumulate, void* stream);
/* Inference-mode stats blocks (moving statistics, eps 1e-3) of n layers in one launch.  Host arrays of n device pointers / sizes;
 * stats[i]: 4*G[i]*C[i] floats; table_dev: cdrl_bn_inference_stats_table_bytes(n) bytes of device memory, 8-byte aligned.  The call
 * waits for the table copy (it synchronises the stream once). */
int64_t cdrl_bn_inference_stats_table_bytes(int n);
int cdrl_bn_inference_stats(int n, const float* const* gamma, const float* const* beta, const float* const* moving_mean,
                            const float* const* moving_var, float* const* stats, const int* G, const int* C, void* table_dev,
                            void* stream);
/* Fused stem block (core/architectures.py:160-161): BatchNorm-apply + ReLU6 + MaxPooling2D(3,2,'same') on the
 * raw conv output (stats from cdrl_bn_train_fwd), and the BatchNorm backward that gathers its incoming
 * gradient from the pooled gradient `dp` through the saved argmax.  argmax codes: ky * 3 + kx of the winning window position in bits 0-3;
 * bit 7 is set where the winning activation is clamped (ReLU6 closed: no gradient flows); decoders mask it away. */
int cdrl_maxpool_bn_fwd(const float* y, const float* stats, int G, int frames_per_group, float* p, uint8_t* argmax,
                        int N, int H, int W, int C, int act_type, void* stream);
int cdrl_bn_train_bwd_pooled(const uint8_t* argmax, const float* dp, int H, int W, const float* y, int G, int Mg, int C,
                             const float* stats, float* dgamma, float* dbeta, float* dy, float* coef, double* workspace,
                             void* stream);
/* Backward of the whole stem block Conv2D(3x3,s2,valid) -> BatchNormalization+ReLU6 -> MaxPooling2D(3,2,'same')
 * (core/architectures.py:159-161) from the POOLED gradient dp, without materialising any pre-pool gradient: the BN sums
 * are taken in scatter form over dp (one gathered y per pooled element), the BN-backward apply and the pool gather run
 * inside the operand load of the filter-gradient GEMM.  x: observations (B,T,H,W,3); y: raw conv output
 * [(t*B+b)][Ho][Wo][Cout]; stats: the BN's 4*T*Cout block; argmax/dp: [T*B][Hp][Wp][Cout].  Outputs dgamma, dbeta, coef
 * (3*T*Cout scratch), dw (3,3,3,Cout), db.  workspace: cdrl_stem_block_bwd_workspace_doubles().  Cout % 4 == 0, <= 32.
 * Any number of rows per time slice is handled: a filter-gradient workgroup owns rows_per >= 128 consecutive rows and stages the
 * statistics of two time slices; where B * Ho * Wo is so small that its rows come from three or more slices (field 31 of cdrl_stem_plan
 * above 2), the host selects a form of the kernel that reads each row's own slice (field 28). */
int64_t cdrl_stem_block_bwd_workspace_doubles(int B, int T, int H, int W, int Cout);
int cdrl_stem_block_bwd(const float* x, const float* y, const float* stats, const uint8_t* argmax, const float* dp, int B, int T,
                        int H, int W, int Cout, float* dgamma, float* dbeta, float* coef, float* dw, float* db,
                        double* workspace, int act_type, void* stream);
/* Same, with the pooled ACTIVATED output `pooled` of cdrl_maxpool_bn_fwd (null = the form above; element type as y / dp): the
 * BatchNorm sums then take the ReLU6 decision and xhat from it instead of gathering the pre-pool value through the argmax (a dense
 * read of a tensor a quarter the size; what the engine does).  Channels with |gamma * invstd| < 0.05 keep the gather.  With bf16
 * storage xhat comes from the ROUNDED pooled value: bf16-level agreement with the gather form, not bit-wise. */
int cdrl_stem_block_bwd_pooled(const float* x, const float* y, const float* stats, const uint8_t* argmax, const float* dp,
                               const float* pooled, int B, int T, int H, int W, int Cout, float* dgamma, float* dbeta, float* coef,
                               float* dw, float* db, double* workspace, int act_type, void* stream);
/* cdrl_stem_plan: what the launchers of the stem block dispatch on for this shape (they call the same host function) -- launches nothing,
 * reads no memory.  pooled: a pooled activated output is given (cdrl_stem_block_bwd_pooled); db_adjacent: db == dw + 27 * Cout;
 * y_aligned: y is 16-byte aligned.  Writes min(n_out, 36) int32 fields and returns 36 (-1: bad act_type, no field array, B, T or Cout < 1,
 * H or W < 3):
 *    0 Ho  1 Wo (conv output)  2 Hp  3 Wp (pooled output)
 *    4 cdrl_stem_fwd: 1 four channels per thread, 0 the scalar kernel (Cout % 4 != 0 or y unaligned)
 *    5 cdrl_stem_fwd_stats refusal: 0 runs, 1 Cout (% 4 != 0 or > 64), 3 alignment of y
 *    6 form: 0 band (a workgroup walks (frame, band of R rows) units staged in LDS), 1 window (image of 2 GB or more, a band of one row
 *      wider than 6144 floats -- W > 682 --, Cout < 4, or CDRL_STEM_FWD_BAND=0)
 *    7 R  8 NB bands per frame  9 nbpg workgroups per time slice  10 px 16-byte chunks per thread of a band (2, 4, 6)  11 NP pixels per
 *      thread and iteration  12 LDS bytes  13 units the busiest workgroup walks  14 rows of the [T][rows][2][Cout] partials
 *   15 vec  16 cx  17 cy  18 nloop  19 rb  20 nb   of cdrl_maxpool_bn_fwd
 *   21 BatchNorm sums over the pooled gradient: 1 the four-channel kernel, 0 the generic column reduce   22 1: it reads the pooled
 *      activated output   23 nb partial rows per time slice
 *   24 cdrl_stem_bwd_filter: 0 MFMA kernel, 2 column reduce (Cout > 32)
 *   25 fused filter gradient refusal: 0 runs, 1 Cout (% 4 != 0 or > 32), 2 conv output of 2 GB or more   26 1 fused MFMA kernel, -1 refused
 *   27 NCH 16-byte channel chunks per lane (3: Cout <= 24, 4; 1 unfused)  28 1: the form that reads each row's own time slice
 *   29 rows_per workgroup  30 workgroups  31 the most time slices the rows of one workgroup come from  32 1: one reduce over dw and db
 *   33 workspace doubles the filter gradient writes  34 cdrl_stem_bwd_workspace_doubles  35 doubles of the BatchNorm partials in front */
int cdrl_stem_plan(int B, int T, int H, int W, int Cout, int act_type, int pooled, int db_adjacent, int y_aligned, int32_t* fields,
                   int n_out);

/* Rollout-time image augmentation of one observation stack (CARLAgent.augment, core/carla_agent.py:545-577; ops of
 * rl/augmentations/augmentations.py and simclr.color_jitter): color jitter (brightness -> contrast -> saturation -> hue ->
 * clip) -> random-kernel blur -> salt & pepper -> gaussian noise -> per-image min-max normalisation -> cutout -> coarse
 * dropout.  The plan says which ops fire and with which scalars (the host draws it, as tf_chance / tf.image.random_* do in
 * the reference); per-pixel random fields are Philox-4x32-10 streams of (seed, offset).  in/out: [T][H][W][3] floats on
 * the device (may not alias); workspace: cdrl_augment_workspace_floats(T, H, W) floats. */
typedef struct {
    int jitter;                 /* 1: color jitter with the four scalars below */
    float brightness, contrast, saturation, hue;
    int blur_size;              /* 0 (off), 3 or 5 */
    float blur_kernel[75];      /* [k][k][3], used [0, 3*k*k) */
    int salt_pepper;            /* 1: tf_salt_and_pepper_batch(amount, prob) */
    float sp_amount, sp_prob;
    int gauss_noise;            /* 1: tf_gaussian_noise_batch(amount, std) */
    float gn_amount, gn_std;
    int normalize;              /* 1: tf_normalize_batch */
    int cutout_size, cutout_cell;   /* size 0 = off; the zeroed cell (row-major index in the size x size grid) */
    int dropout_size;           /* 0 = off; size x size Bernoulli(1 - amount) grid, nearest-neighbour upsampled */
    float dropout_amount;
    uint64_t seed, offset;
} cdrl_aug_plan;
int64_t cdrl_augment_workspace_floats(int T, int H, int W);
int cdrl_augment_images(const float* in, float* out, int T, int H, int W, const cdrl_aug_plan* plan, float* workspace,
                        void* stream);
/* The same for a shard of E stacks in a fixed five launches: in/out [E][T][H][W][3] (may not alias; `in` is only read), plans_dev:
 * E plans IN DEVICE MEMORY, one per stack -- ops may fire for some stacks and not for others.  out[e] receives exactly the bytes
 * cdrl_augment_images(in + e * T*H*W*3, ..., &plans[e], ...) writes; the Philox streams stay keyed by stack e's own (seed, offset)
 * and the element index within that stack.  The plans cannot be read by the host here: the caller validates blur_size before
 * the upload, and the kernels treat a size outside {0, 3, 5} as 0.  E <= 65535.  workspace:
 * cdrl_augment_batch_workspace_floats(E, T, H, W) floats (0 for a bad shape). */
int64_t cdrl_augment_batch_workspace_floats(int E, int T, int H, int W);
int cdrl_augment_images_batch(const float* in, float* out, int E, int T, int H, int W, const cdrl_aug_plan* plans_dev,
                              float* workspace, void* stream);
/* Contrastive views (the SimCLR view pipeline the reference's rl/augmentations/simclr.py:pipeline states: crop + resize + flip ->
 * colour jitter -> colour drop -> blur), one plan per view, shared by the T frames of its stack; scalars only, drawn by the host.
 * rows [N][T][H][W][3] -> out [V][T][H][W][3]; view v reads row v % N (no doubled copy of the rows); any V >= 1, 1 <= N <= V.
 *   1 crop window -> bilinear resize to H x W (tf.image.resize: half-pixel centres, no antialias; source (d + 0.5) * crop / full
 *     - 0.5 clamped to [0, crop - 1], taps floor and min(floor + 1, crop - 1), x first, then y) -> horizontal flip; a full-size
 *     crop without flip returns the input's bits
 *   2 colour jitter as cdrl_augment_images (the contrast mean is that of the resized, brightness-shifted frame; fixed-order sums)
 *   3 colour drop: 0.2989 r + 0.5870 g + 0.1140 b on all three channels
 *   4 separable blur with blur_w, horizontal then vertical, replicate edge
 * Four launches for any V; the same plans give the same bytes.  plans_dev: V plans IN DEVICE MEMORY; their contents are validated
 * by the caller before the upload (the kernels clamp a crop window into the frame and treat a tap count that is even or outside
 * 3..15 as 0).  Refused: null pointers, H or W < 2, V < 1, N outside [1, V], a workspace that overlaps rows or out.  workspace:
 * cdrl_views_workspace_floats(V, T, H, W) floats (0 for a bad shape). */
typedef struct cdrl_view_plan {
    int32_t crop_y, crop_x, crop_h, crop_w;     /* crop window inside H x W; crop_h == H && crop_w == W: no crop */
    int32_t flip;                               /* horizontal */
    int32_t jitter;
    float brightness, contrast, saturation, hue;
    int32_t drop;                               /* colour drop */
    int32_t blur_taps;                          /* 0, or odd, 3..15 */
    float blur_w[16];                           /* 1-D weights, sum 1, drawn up by the host */
} cdrl_view_plan;
int64_t cdrl_views_workspace_floats(int V, int T, int H, int W);
int cdrl_views_batch(const float* rows, int N, float* out, int V, int T, int H, int W, const cdrl_view_plan* plans_dev,
                     float* workspace, void* stream);
/* Occlusion saliency of one decision: the acting network on N variants of ONE observation -- image [T][H][W][3],
 * road [T][Dr], vehicle [T][Dv], navigation [T][Dn] -- each with one part replaced by a neutral baseline.  A grid (gh, gw),
 * 1 <= gh <= H, 1 <= gw <= W, cuts every frame into cells: cell (cy, cx) covers rows [(cy*H)/gh, ((cy+1)*H)/gh) and columns
 * [(cx*W)/gw, ((cx+1)*W)/gw) (integer division: no cell is empty, the cells partition the frame).  F = T when per_frame, else 1
 * (a cell is then occluded in all T frames at once).  N = 1 + F*gh*gw + (modalities ? 4 : 0) rows:
 *   row 0                          the observation, bit for bit
 *   row 1 + (f*gh + cy)*gw + cx    the pixels of cell (cy, cx) of frame f (every frame when F = 1) taken from the baseline
 *   then, with modalities          the whole image taken from the baseline; road zeroed; vehicle zeroed; navigation zeroed
 * Whatever a row does not occlude keeps its bits.
 *   cdrl_occlusion_baseline  baseline [T][H][W][3] from the image: mode 0 zeros, mode 1 the mean of each frame and channel
 *                            (fixed-order double sums, one rounding: the same input gives the same bytes).  One launch.
 *   cdrl_occlusion_rows      rows [first, first + count) of the N rows into out_image [count][T][H][W][3] and out_road /
 *                            out_vehicle / out_navigation [count][T][D*]; a row index >= N is written as a copy of row 0, so every
 *                            chunk is written in full.  baseline: any stack of the image's shape.  One launch, the row is the
 *                            grid's y dimension; 16-byte accesses when T*H*W*3 is a multiple of 4 and image, baseline and out_image
 *                            are 16-byte aligned, 4-byte accesses otherwise.  count <= 65535; the chunk may not overlap the image
 *                            or the baseline.
 *   cdrl_occlusion_scores    alpha, beta [N][A], value [N][2] (base, exponent) -> scores [N-1][2 + A] doubles for rows 1 .. N-1
 *                            against row 0, in double arithmetic: [0] sum_a KL(Beta(alpha_0, beta_0) || Beta(alpha_g, beta_g)) (the
 *                            analytic form of cdrl_beta_kl, the anchor first), [1] base_g * 10^exp_g - base_0 * 10^exp_0,
 *                            [2 + a] alpha_g / (alpha_g + beta_g) - alpha_0 / (alpha_0 + beta_0), signed.  A row equal to row 0
 *                            scores exactly 0.  N >= 2, A <= 8.  One launch.
 *   cdrl_occlusion_maps      the first F*gh*gw rows of scores [.][K] -> maps [K][F][H][W] floats.  upsample 0 (nearest): a pixel
 *                            takes the score of its cell; 1 (bilinear, for display): the gh x gw grid of a frame resized to H x W
 *                            with the half-pixel rule of cdrl_views_batch (a grid equal to (H, W) returns the scores).  normalize:
 *                            a column's maps are divided by its largest |score| over all F*gh*gw cells (in double, before the one
 *                            rounding to float); a column whose largest |score| is 0 gives zeros.  K <= 10.  One launch.
 * No entry reads anything back, allocates or synchronises.  -1 and cdrl_last_error: null pointers, shapes or grids out of range. */
int cdrl_occlusion_baseline(const float* image, float* baseline, int T, int H, int W, int mode, void* stream);
int cdrl_occlusion_rows(const float* image, const float* baseline, const float* road, const float* vehicle, const float* navigation,
                        int T, int H, int W, int Dr, int Dv, int Dn, int gh, int gw, int per_frame, int modalities, int first,
                        int count, float* out_image, float* out_road, float* out_vehicle, float* out_navigation, void* stream);
int cdrl_occlusion_scores(const float* alpha, const float* beta, const float* value, int N, int A, double* scores, void* stream);
int cdrl_occlusion_maps(const double* scores, int K, int F, int gh, int gw, int H, int W, int upsample, int normalize, float* maps,
                        void* stream);
/* Scoring the acting policy on held-out expert rows: the outputs of cdrl_learner_predict for one chunk of rows --
 * dist [rows][4][A] (alpha, beta, mean, std; the two float columns mean and std are not read), value [rows][4] (base, exp, speed,
 * similarity) -- against what a trace recorded for the first `count` <= rows of them (the tail of a padded last chunk is ignored):
 * u [count][A] the expert actions in the unit interval, returns_be [count][2] (base, exp) or NULL, speed and similarity [count]
 * (both or neither).  One launch of one workgroup; transcendentals and sums in double; fixed reduction order, no atomics: the same
 * rows in the same chunks give the same bits.  `block` is read-modify-written: the caller zeroes it, a sweep is one launch per
 * chunk and one host read at the end.  CDRL_SCORE_BLOCK(A) doubles (a count is a double too, exact up to 2^53):
 *   head   [0] rows scored  [1] rows of the launches with returns  [2] rows of the launches with speed / similarity
 *          [3] elements (row, action) with a non-finite alpha or beta: left out of EVERY sum below, their pit entry NaN
 *          [4] elements whose PIT reached the iteration cap: left out of the histogram and the two coverage counts, pit entry NaN
 *          [5..7] unused (0)
 *   value  [8] sum (V - R)  [9] sum (V - R)^2  [10] sum R  [11] sum R^2, V = base * 10^exp of the value head, R = rbase * 10^rexp
 *          of returns_be; written only with returns_be
 *   aux    [12] sum (value[.][2] - speed)^2  [13] sum (value[.][3] - similarity)^2; written only with speed / similarity
 *          [14..15] unused (0)
 *   action a, at CDRL_SCORE_HEAD + a * CDRL_SCORE_PER_ACTION, with x = clip(u, eps, 1 - eps) (float32 machine epsilon, as
 *   cdrl_beta_clone_loss) and alpha, beta widened to double:
 *          [+0] elements summed  [+1] sum log Beta(x; alpha, beta)  [+2] sum |mode - x|, mode = (alpha - 1) / (alpha + beta - 2)
 *          [+3] sum (mean - x)  [+4] sum (mean - x)^2, mean = alpha / (alpha + beta)
 *          [+5] sum of the predicted variance alpha beta / ((alpha + beta)^2 (alpha + beta + 1))  [+6] sum of the entropy
 *          [+7] elements with 0.25 <= F <= 0.75  [+8] elements with 0.05 <= F <= 0.95
 *          [+9 .. +9 + CDRL_SCORE_BINS) histogram of F over equal bins, bin min(BINS - 1, floor(F * BINS))
 *   F = I_x(alpha, beta), the Beta CDF at the expert action (probability integral transform, PIT): the continued fraction with
 *   modified Lentz steps, directly for x < (alpha + 1) / (alpha + beta + 2), as 1 - I_{1-x}(beta, alpha) beyond; prefactor
 *   exp(lgamma(a+b) - lgamma(a) - lgamma(b) + a log x + b log1p(-x)); stops when a step's factor is within 1e-15 of 1 or after
 *   256 steps (alpha = beta = 1e6, x = 0.5 would need 526: counted in [4]).  pit: [count][A] doubles or NULL, every entry written.
 * -1 and cdrl_last_error, before any launch: a null dist / value / u / block, rows < 1, count < 1 or > rows, A < 1 or > 8, exactly
 * one of speed / similarity. */
#define CDRL_SCORE_BINS 10
#define CDRL_SCORE_HEAD 16
#define CDRL_SCORE_PER_ACTION (9 + CDRL_SCORE_BINS)
#define CDRL_SCORE_BLOCK(A) (CDRL_SCORE_HEAD + CDRL_SCORE_PER_ACTION * (A))
int cdrl_beta_score(const float* dist, const float* value, const float* u, const float* returns_be, const float* speed,
                    const float* similarity, int rows, int count, int A, double* block, double* pit, void* stream);
/* CARLAgent.policy_objective / value_objective on linear head outputs (core/carla_agent.py:394-428,
 * 469-486); writes d(loss)/d(lin) and 16 metric floats. */
int cdrl_beta_ppo_loss(const float* lin, const float* adv, const float* old_logp, const float* speed,
                       const float* similarity, const float* u, const float* du_da, const float* du_db, float clip_ratio,
                       float entropy_coef, int B, int A, float grad_scale, float* dlin, float* metrics, float* aux,
                       float* hp_scratch16, void* stream);
int cdrl_value_loss(const float* lin, const float* returns, const float* speed, const float* similarity, int B,
                    float exp_scale, float grad_scale, float* dlin, float* metrics, float* values, void* stream);
/* Analytic KL between an anchor Beta policy and the Beta head on linear head outputs lin (B, 2A+2, as cdrl_beta_clone_loss): anchor
 * (B, 2, A) = alpha0, beta0; alpha = softplus(lin) + 1.01 (beta likewise).  Per row and action
 *   KL(Beta(a0,b0) || Beta(a,b)) = lnB(a,b) - lnB(a0,b0) + (a0-a) psi(a0) + (b0-b) psi(b0) + (a-a0+b-b0) psi(a0+b0);
 * a row's KL is the sum over its actions (the joint distribution), kl = mean over the rows.  metrics: [0] max(kl, 0) (rounding can put
 * a true zero slightly negative) [1] the largest row KL [2] metrics[0] / A.  A NaN in the anchor gives NaN in all three.
 * kl_coef > 0: dlin (B, 2A+2) += grad_scale * kl_coef * d kl / d lin on the 2A distribution columns, one rounding per element
 * (unclamped); kl_coef == 0: dlin is not read or written and may be NULL.  One workgroup; transcendentals and sums in double.
 * A <= 8, kl_coef >= 0 (-1 and cdrl_last_error otherwise). */
int cdrl_beta_kl(const float* lin, const float* anchor, int B, int A, float kl_coef, float grad_scale, float* dlin, float* metrics,
                 void* stream);
/* Behaviour-cloning loss of the Beta head on linear head outputs lin (B, 2A+2: A alpha, A beta, similarity, speed columns) and
 * expert actions u (B, A) in the unit interval.  alpha = softplus(lin) + 1.01 (beta likewise); x = clip(u, eps, 1 - eps) with the
 * float32 machine epsilon, no gradient through x; clone = mean_b w_b * (-mean_a log Beta(x; alpha, beta)), weight (B) or NULL = 1;
 * entropy = mean over B*A; speed_loss = 0.5 * mean (2 sigmoid(lin_speed) - speed)^2, sim_loss = 0.5 * mean (tanh(lin_sim) -
 * similarity)^2 (speed and similarity both NULL: the two terms and their dlin columns are 0);
 * total = clone - entropy_coef * entropy + aux_weight * (speed_loss + sim_loss); dlin (B, 2A+2) = grad_scale * d total / d lin,
 * every entry written.  metrics: [0] total [1] clone [2] entropy [3] speed_loss [4] sim_loss [5] sum(w) / B [6] unweighted mean
 * log-probability [7] unweighted mean over B*A of |mode - x|, mode = (alpha - 1) / (alpha + beta - 2): the error of the action a
 * deterministic evaluation takes.  aux (B, 4A) or NULL: alpha, beta, log-probability, entropy, as cdrl_beta_ppo_loss writes them.
 * One workgroup; transcendentals and sums in double, one rounding per output.  A <= 8 (-1 and cdrl_last_error above). */
int cdrl_beta_clone_loss(const float* lin, const float* u, const float* weight, const float* speed, const float* similarity,
                         float entropy_coef, float aux_weight, int B, int A, float grad_scale, float* dlin, float* metrics, float* aux,
                         void* stream);
/* Mixed policy loss on linear head outputs lin (B, 2A+2): the arguments of cdrl_beta_ppo_loss plus demo_u (B, A),
 * demo_w (B) and an optional device block.  Row b is a demonstration row iff demo_w[b] > 0, a PPO row otherwise; ND and NP = B - ND
 * are counted in a block reduction in front of the row loop.
 *   PPO term   = that of cdrl_beta_ppo_loss (same clipped action, same rule for the pathwise Jacobians, same mean-over-actions ratio
 *                and routing of the minimum), summed over the PPO rows and divided by NP; 0 when NP = 0.
 *   demo term  = sum_b demo_w[b] * (-mean_a log Beta(x; alpha, beta)) / ND, x = clip(demo_u, eps, 1 - eps), no gradient through x;
 *                adv, old_logp, u, du_da, du_db of such a row are not read; 0 when ND = 0.
 *   entropy, speed_loss, sim_loss: over all B rows, as cdrl_beta_ppo_loss has them.
 * dlin (B, 2A+2) = grad_scale * d total / d lin, every entry of every row written.  metrics: [0] total including the demo term
 * [1] PPO term [2] entropy [3] speed_loss [4] sim_loss [5] mean ratio and [6] mean log-probability of the PPO rows [7] demo term
 * [8] mean log-probability of the demonstration rows [9] their mean |mode - x| (as cdrl_beta_clone_loss slot 7) [10] ND.
 * demo_block (device, or NULL): thread 0 adds slots 7..10 and one pass, see cdrl_learner_set_demo_block.
 * With demo_w all zero, dlin and metrics[0..6] are bit-identical to cdrl_beta_ppo_loss on the same inputs, with and without
 * du_da / du_db.  One workgroup of 256 threads; transcendentals and sums in double, one rounding per output.
 * -1 (and cdrl_last_error): A outside 1..8, B < 1, a null lin / u / demo_u / demo_w / dlin / metrics. */
int cdrl_beta_mixed_policy_loss(const float* lin, const float* adv, const float* old_logp, const float* speed,
                                const float* similarity, const float* u, const float* du_da, const float* du_db, const float* demo_u,
                                const float* demo_w, float clip_ratio, float entropy_coef, int B, int A, float grad_scale, float* dlin,
                                float* metrics, float* aux, float* hp_scratch16, cdrl_demo_stats* demo_block, void* stream);
/* NT-Xent, the normalised-temperature cross-entropy over pairs of views, on embeddings z (B, D), B = 2N: rows i and
 * pair(i) = (i + N) mod B are the two views of one observation.
 *   zn_i = z_i / max(||z_i||, 1e-12);  s_ij = zn_i . zn_j / temperature;  l_i = log sum_{j != i} exp(s_ij) - s_{i,pair(i)};
 *   L = mean_i l_i;  dz (B, D) = grad_scale * dL/dz, through both roles of every s_ij and through the normalisation; every entry
 * written; dz may not be z.  metrics (16 floats, unscaled by grad_scale): [0] L  [1] share of rows whose positive logit is strictly
 * above that of every other j != i (1 for B = 2)  [2] mean cosine of the pairs  [3] mean cosine over j != i, pair(i) (0 for B = 2)
 * [4] mean ||z_i||  [5] temperature  [6..15] 0.
 * workspace: the number of floats the first entry returns (16-byte aligned); all scratch lives there.  Deterministic (no atomics,
 * fixed reduction order), no host read, no allocation: capturable.  The similarity matrix is never stored; row sums in double.
 * -1 (and cdrl_last_error, naming the argument): B odd, B < 2, B > 2048, D < 1, temperature <= 0. */
int64_t cdrl_ntxent_workspace_floats(int B, int D);
int cdrl_ntxent_loss(const float* z, int B, int D, float temperature, float grad_scale, float* dz, float* metrics, float* workspace,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CDRL_H */

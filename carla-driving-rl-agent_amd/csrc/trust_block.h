// Trust-region block: one per learner created with cdrl_config.trust = 1, in its workspace, shared between learners
// like the gate block (share_hp).  Plain C++ without the HIP runtime: the host layout check (tests/host/trust_layout.cpp) includes it.
#pragma once
#include <stdint.h>

namespace cdrl {

struct TrustBlock {
    // host-written head (cdrl_learner_set_trust_params, by value through a one-thread launch); nothing behind it is written by the
    // host after bind
    float target_kl;            // <= 0: the KL is measured, the latch never sets
    float kl_stop_factor;       // the latch sets when !(kl <= kl_stop_factor * target_kl): a NaN KL sets it
    float kl_coef;              // > 0: d(kl_coef * KL)/dlin is added to the policy head's dlin; == 0: dlin is not touched
    // device-owned, written by thread 0 of beta_kl_kernel (armed: also by the disarm node, skipped: by the gate)
    float kl_last;              // KL of the last measured pass, clamped below at 0
    float kl_max;               // largest kl_last since the last reset (NaN once a pass measured NaN)
    int32_t passes;             // measured passes since the last reset
    int32_t stop;               // the latch
    int32_t stop_pass;          // index (among the measured passes) of the pass that set it; -1 before
    int32_t armed;              // the pass in flight measured a KL: its policy_apply obeys the latch
    int32_t skipped;            // policy applies the latch skipped since the last reset
    double kl_sum;              // sum of kl_last over the measured passes
};

constexpr int TRUST_HOST_WORDS = 3;     // floats at the head of the block that are the host's

}  // namespace cdrl

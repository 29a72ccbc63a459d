// Layout check of the trust-region guard's structs, plain host C++ with its own main (tests/test_trust_host.py builds
// and runs it, also under -fsanitize=address,undefined): the fields appended to the C ABI structs sit BEHIND the old ones, whose
// offsets are the ones every earlier caller was compiled with; cdrl_hparams keeps its size; the device TrustBlock, its C ABI mirror
// cdrl_trust_stats and the host-written head cdrl_trust_params agree field by field.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../carla-driving-rl-agent_amd/csrc/trust_block.h"
#include "../../include/cdrl.h"

static int failures = 0;

#define EXPECT(cond)                                             \
    do {                                                         \
        if (!(cond)) {                                           \
            printf("FAIL %s (line %d)\n", #cond, __LINE__);      \
            ++failures;                                          \
        }                                                        \
    } while (0)

// offsets of the structs as they were before the guard (32-bit fields from 0, pointers 8 bytes)
static void check_old_offsets() {
    EXPECT(offsetof(cdrl_config, B) == 0 && offsetof(cdrl_config, A) == 28 && offsetof(cdrl_config, stem) == 32);
    EXPECT(offsetof(cdrl_config, stage_c) == 36 && offsetof(cdrl_config, stage_n) == 48 && offsetof(cdrl_config, last) == 60);
    EXPECT(offsetof(cdrl_config, head) == 80 && offsetof(cdrl_config, exp_scale) == 84 && offsetof(cdrl_config, compute) == 88);
    EXPECT(offsetof(cdrl_config, freeze_trunk) == 92 && offsetof(cdrl_config, optimizer) == 96 && offsetof(cdrl_config, polyak) == 100);
    EXPECT(offsetof(cdrl_config, train_stats) == 104 && offsetof(cdrl_config, clip_mode) == 108);
    EXPECT(offsetof(cdrl_config, skip_nonfinite) == 112);
    EXPECT(offsetof(cdrl_config, trust) == 116 && sizeof(cdrl_config) == 120);          // appended
    EXPECT(offsetof(cdrl_hparams, policy_lr) == 0 && offsetof(cdrl_hparams, eps) == 36 && offsetof(cdrl_hparams, clip_norm_dynamics) == 40);
    EXPECT(sizeof(cdrl_hparams) == 44);                                                 // unchanged: the guard's values travel in cdrl_trust_params
    EXPECT(offsetof(cdrl_policy_batch, image) == 0 && offsetof(cdrl_policy_batch, advantages) == 4 * sizeof(void*));
    EXPECT(offsetof(cdrl_policy_batch, u) == 8 * sizeof(void*) && offsetof(cdrl_policy_batch, du_dbeta) == 10 * sizeof(void*));
    EXPECT(offsetof(cdrl_policy_batch, anchor) == 11 * sizeof(void*) && sizeof(cdrl_policy_batch) == 12 * sizeof(void*));       // appended
}

#define SAME(field) EXPECT(offsetof(cdrl::TrustBlock, field) == offsetof(cdrl_trust_stats, field))

static void check_trust_block() {
    using cdrl::TrustBlock;
    EXPECT(sizeof(TrustBlock) == 48 && sizeof(cdrl_trust_stats) == sizeof(TrustBlock));
    EXPECT(offsetof(TrustBlock, target_kl) == 0 && offsetof(TrustBlock, kl_stop_factor) == 4 && offsetof(TrustBlock, kl_coef) == 8);
    EXPECT(offsetof(TrustBlock, kl_last) == cdrl::TRUST_HOST_WORDS * sizeof(float));   // the device's fields start behind the host's
    EXPECT(offsetof(TrustBlock, kl_sum) % 8 == 0);
    SAME(target_kl); SAME(kl_stop_factor); SAME(kl_coef); SAME(kl_last); SAME(kl_max); SAME(passes); SAME(stop); SAME(stop_pass);
    SAME(armed); SAME(skipped); SAME(kl_sum);
    EXPECT(sizeof(cdrl_trust_params) == cdrl::TRUST_HOST_WORDS * sizeof(float));
    EXPECT(offsetof(cdrl_trust_params, target_kl) == 0 && offsetof(cdrl_trust_params, kl_stop_factor) == 4 &&
           offsetof(cdrl_trust_params, kl_coef) == 8);
    // the head as cdrl_trust_params spells it: TRUST_HOST_WORDS floats over the front of a block on the heap, nothing behind them
    TrustBlock* dev = static_cast<TrustBlock*>(malloc(sizeof(TrustBlock)));
    memset(dev, 0, sizeof(TrustBlock));
    dev->stop_pass = -1;
    dev->kl_sum = 0.25;
    dev->skipped = 7;
    const cdrl_trust_params tp = {0.01f, 1.5f, 0.5f};
    float stage[cdrl::TRUST_HOST_WORDS];
    memcpy(stage, &tp, sizeof(stage));
    memcpy(dev, stage, sizeof(stage));
    EXPECT(dev->target_kl == 0.01f && dev->kl_stop_factor == 1.5f && dev->kl_coef == 0.5f);
    EXPECT(dev->kl_last == 0.0f && dev->stop_pass == -1 && dev->skipped == 7 && dev->kl_sum == 0.25);
    cdrl_trust_stats out;
    memcpy(&out, dev, sizeof(out));
    EXPECT(out.target_kl == 0.01f && out.stop_pass == -1 && out.skipped == 7 && out.kl_sum == 0.25);
    free(dev);
}

int main() {
    check_old_offsets();
    check_trust_block();
    if (failures) return 1;
    printf("OK\n");
    return 0;
}

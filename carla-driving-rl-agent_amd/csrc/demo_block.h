// Demonstration block: running sums of the mixed policy loss's demonstration statistics over the passes of one
// update().  The caller owns the memory (cdrl_learner_set_demo_block) and zeroes it; thread 0 of mixed_policy_loss_kernel adds to
// it.  Plain C++ without the HIP runtime.
#pragma once
#include <stdint.h>

namespace cdrl {

struct DemoBlock {
    double loss_sum;            // sum over the passes of metrics[7], the demonstration term
    double logp_sum;            // ... of metrics[8], the demonstration rows' mean log-probability
    double mode_sum;            // ... of metrics[9], their mean absolute mode error
    double rows_sum;            // ... of metrics[10], the number of demonstration rows
    int64_t passes;             // launches that added to the block
};

constexpr int DEMO_BLOCK_BYTES = 40;
static_assert(sizeof(DemoBlock) == DEMO_BLOCK_BYTES, "cdrl_demo_stats (include/cdrl.h) mirrors this layout");

}  // namespace cdrl

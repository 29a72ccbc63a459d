// Score block: the running sums cdrl_beta_score adds to, all doubles (a count is exact up to 2^53).  The same
// numbers as the CDRL_SCORE_* macros of include/cdrl.h and SCORE_LAYOUT of engine.py (tests/test_score_host.py compares the three).
// Plain C++ without the HIP runtime.
#pragma once

namespace cdrl {

constexpr int SCORE_BINS = 10;                  // equal bins of the PIT histogram
enum {
    // head
    SCORE_ROWS = 0,                             // rows scored
    SCORE_ROWS_RETURNS,                         // ... of launches that were given returns
    SCORE_ROWS_AUX,                             // ... of launches that were given speed / similarity
    SCORE_NONFINITE,                            // elements with a non-finite alpha or beta (left out of every sum)
    SCORE_UNCONVERGED,                          // elements whose PIT reached the iteration cap (left out of histogram and coverage)
    // value, V = base * 10^exp against R = rbase * 10^rexp
    SCORE_V_ERR = 8,                            // sum (V - R)
    SCORE_V_ERR2,                               // sum (V - R)^2
    SCORE_V_RET,                                // sum R
    SCORE_V_RET2,                               // sum R^2
    // auxiliary heads
    SCORE_SPEED_ERR2 = 12,                      // sum (speed_pred - speed)^2
    SCORE_SIM_ERR2,                             // sum (similarity_pred - similarity)^2
    SCORE_HEAD = 16                             // doubles in front of the per-action groups
};
enum {                                          // per action a, at SCORE_HEAD + a * SCORE_PER_ACTION
    SCORE_A_COUNT = 0,                          // elements summed (finite alpha and beta)
    SCORE_A_LOGP,                               // sum log Beta(x; alpha, beta)
    SCORE_A_MODE_ERR,                           // sum |mode - x|
    SCORE_A_ERR,                                // sum (mean - x)
    SCORE_A_ERR2,                               // sum (mean - x)^2
    SCORE_A_VAR,                                // sum of the predicted variance
    SCORE_A_ENTROPY,                            // sum of the entropy
    SCORE_A_COVER50,                            // elements with 0.25 <= PIT <= 0.75
    SCORE_A_COVER90,                            // elements with 0.05 <= PIT <= 0.95
    SCORE_A_HIST,                               // SCORE_BINS counts
    SCORE_PER_ACTION = SCORE_A_HIST + SCORE_BINS
};

constexpr int score_block_doubles(int A) { return SCORE_HEAD + SCORE_PER_ACTION * A; }

}  // namespace cdrl

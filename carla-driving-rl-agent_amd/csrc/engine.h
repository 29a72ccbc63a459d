// Learner engine: owns the layer graph of CARLANetwork (trunk + policy / old-policy / value
// heads), the flat parameter-arena layout and the workspace plan for one batch size.
#pragma once
#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "cdrl_kernels.h"
#include "sched.h"

namespace cdrl {

struct Config {
    int B = 1, T = 4, H = 90, W = 120;
    int road = 9, vehicle = 4, navigation = 5, A = 2;
    int stem = 24;
    int stage_c[3] = {116, 232, 464};
    int stage_n[3] = {4, 8, 4};
    int last = 768;
    int feat = 16;
    int rnn_image = 256, rnn_small = 32;
    int dyn = 512;
    int head = 320;
    float exp_scale = 6.0f;
    int compute = 0;        // 0: float32 products; 1: bf16 MFMA operands in the tower's 1x1 convolutions (configuration 3);
                            // 2: 1 + bf16 ACTIVATION STORAGE: every activation / activation-gradient tensor of the image tower
                            //    is bf16 in HBM (statistics, partials, coefficients, weights, accumulators stay float32 / double)
    int freeze_trunk = 0;   // 1: the passes train the heads only on a fixed trunk (reference CARLAgent(update_dynamics=False)): train-mode
                            //    trunk forward (batch statistics, moving statistics updated), no trunk backward, no trunk Adam step
    int optimizer = 0;      // CDRL_OPT_* of the policy, value and dynamics optimizers (include/cdrl.h table)
    float polyak = 1.0f;    // < 1: polyak averaging of the heads after their optimizer step
    int train_stats = 0;    // N > 0: device-resident ring of N update-diagnostics rows, one per apply step (include/cdrl.h)
    int clip_mode = 0;      // CDRL_CLIP_TENSOR: per-tensor clip of the heads; CDRL_CLIP_GLOBAL: every optimizer's list by its global norm
    int skip_nonfinite = 0; // 1: an apply step whose gradients hold a NaN / Inf writes nothing (include/cdrl.h, gradient gate)
    int trust = 0;          // 1: trust-region guard of the policy steps (include/cdrl.h): policy passes with an anchor measure
                            //    the Beta KL on the device, policy_apply takes the gated forms and obeys the block's latch
};

enum Model : int { M_TRUNK = 0, M_POLICY = 1, M_VALUE = 2, M_OLD_POLICY = 3 };

struct ParamInfo {
    std::string name;
    int shape[4] = {1, 1, 1, 1};
    int ndim = 1;
    int64_t numel = 0;
    int trainable = 1;
    int model = 0;
    int64_t off = 0;      // element offset inside the model's trainable / state region
};

struct Buffers {
    float* params = nullptr;     // [policy_tr | trunk_tr | value_tr | policy_st | trunk_st | value_st | old_tr | old_st]
    float* grads = nullptr;      // [policy_tr | trunk_tr | value_tr]
    float* adam_m = nullptr;
    float* adam_v = nullptr;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
};

struct PolicyBatch {
    const float *image, *road, *vehicle, *navigation;       // (B,T,...) reference layout
    const float *adv, *old_logp, *speed, *similarity, *u, *du_da, *du_db;
    const float* anchor;                                    // (B,2,A) alpha0, beta0 of the anchor policy, or null (trust learners only)
};
struct ValueBatch {
    const float *image, *road, *vehicle, *navigation;
    const float *returns, *speed, *similarity;
};
struct CloneBatch {                                         // behaviour cloning: expert actions in place of adv / old_logp
    const float *image, *road, *vehicle, *navigation;
    const float *u, *weight, *speed, *similarity, *returns; // weight, (speed, similarity), returns: optional
};

struct Op {
    std::function<int(hipStream_t, int)> fwd;
    std::function<int(hipStream_t)> bwd;
};

// Identity half of a ShuffleNet unit carried by the unit's last BatchNorm op: forward = copy through the concat + shuffle
// store of the BN-apply kernel, backward = gather of its gradient inside the BN-backward reduction (no separate launches)
struct Passthrough {
    View fsrc{nullptr, 0, 0}, fdst{nullptr, 0, 0};     // forward: X[:, :C] -> out (shuffled, channel offset 0)
    View gsrc{nullptr, 0, 0}, gdst{nullptr, 0, 0};     // backward: out.g (shuffled) -> X.g[:, :C]
    // global average pool fused behind the BatchNorm (head of the tower): the forward writes mean_p act(BN(x)) to gap_out
    // [frames][C] instead of the activated tensor, the backward reads the pooled gradient gap_dout [frames][C] (broadcast / P)
    float* gap_out = nullptr;
    const float* gap_dout = nullptr;
    int gap_rows = 0;                                   // P pixels per frame
};

class Learner {
public:
    const std::string& build_error() const { return build_err_; }
    explicit Learner(const Config& cfg);
    ~Learner();

    const Config& config() const { return cfg_; }
    const std::vector<ParamInfo>& params(int model) const { return infos_[model]; }
    int64_t trainable_elems(int model) const { return tr_size_[model]; }
    int64_t state_elems(int model) const { return st_size_[model]; }
    // element offsets of the regions inside Buffers::params / grads
    int64_t tr_offset(int model) const;
    int64_t st_offset(int model) const;
    int64_t params_total() const;
    int64_t grads_total() const { return tr_size_[0] + tr_size_[1] + tr_size_[2]; }
    size_t workspace_bytes() const { return ws_bytes_; }
    const std::set<std::string>& pw_signatures() const { return pw_sigs_; }

    int bind(const Buffers& b);
    DevHP* host_hp() { return &hp_host_; }
    int upload_hp(hipStream_t st);          // host hp block (lr, clip...) -> device, keeps device counters
    int reset_counters(hipStream_t st);
    // the device block's three step counters and three Nadam m_caches (the owner's block after share_hp): get copies them behind
    // everything on `st` and waits for the copy; set validates, then enqueues one one-thread kernel (no host sync)
    int get_counters(int t[3], float m_cache[3], hipStream_t st);
    int set_counters(const int t[3], const float m_cache[3], hipStream_t st);

    int policy_forward_backward(const PolicyBatch& b, float inv_world, hipStream_t st);
    // split form for the re-sampling loss (F8): forward -> (host samples u from alpha, beta) -> backward
    int policy_forward(const float* image, const float* road, const float* vehicle, const float* navigation,
                       hipStream_t st);
    int policy_backward(const PolicyBatch& b, float inv_world, hipStream_t st);
    // forward -> on-device Beta re-sampling (u, du/dalpha, du/dbeta) -> backward; batch.u / du_* are ignored
    int policy_forward_backward_resample(const PolicyBatch& b, uint64_t seed, uint64_t offset, float inv_world,
                                         hipStream_t st);
    float* sample_buffer() const { return sample_u_; }
    // Demonstration-augmented policy pass: the policy pass with mixed_policy_loss where policy_loss stands.  Rows with
    // demo_w > 0 are demonstration rows (maximum likelihood of demo_u), the others PPO rows; everything else -- trunk and head forward,
    // the re-sampling with its Philox offsets, head and trunk backward, freeze_trunk, the graph -- is the policy pass's.  Refuses a
    // batch with an anchor (the anchor sweep has no demonstration rows).  Followed by policy_apply.
    int demo_forward_backward(const PolicyBatch& b, const float* demo_u, const float* demo_w, float inv_world, hipStream_t st);
    int demo_forward_backward_resample(const PolicyBatch& b, const float* demo_u, const float* demo_w, uint64_t seed, uint64_t offset,
                                       float inv_world, hipStream_t st);
    // caller-owned device block the demonstration passes add their statistics to (null: none); part of their graph key
    void set_demo_block(DemoBlock* d) { demo_block_ = d; }
    int policy_apply(hipStream_t st);
    // a sequence of calls on ONE caller stream: the hand-overs happen once, around the whole sequence
    int sequence_begin(hipStream_t caller) { return sched_.sequence_begin(caller); }
    int sequence_end(hipStream_t caller) { return sched_.sequence_end(caller); }
    int value_forward_backward(const ValueBatch& b, float inv_world, hipStream_t st);
    int value_apply(hipStream_t st);
    // Joint policy + value update (opt-in): ONE train-mode trunk forward (moving statistics updated once), both heads'
    // forwards, policy loss + policy head backward and value loss + value head backward each without the head's bn0, then one launch
    // (bn_small_bwd_pair) that finishes both bn0 and leaves d(policy loss + value loss)/d(dynamics) in the trunk output gradient, then
    // ONE trunk backward.  The value loss takes the policy batch's speed / similarity.  Frozen trunk: no trunk backward.
    // Both refuse (-1) a learner whose heads' bn0 is not in the single-launch form (B > 2048): there is no joint form above it.
    int joint_forward_backward(const PolicyBatch& b, const float* returns, float inv_world, hipStream_t st);
    int joint_forward_backward_resample(const PolicyBatch& b, const float* returns, uint64_t seed, uint64_t offset, float inv_world,
                                        hipStream_t st);
    // The apply of a joint pass: the trunk steps ONCE (its counter advances once), then the policy head (old_policy <- policy in
    // front), then the value head.  Gated: trunk + policy head are decided together from the trunk's and the policy's list, the value
    // head from its own list; CDRL_CLIP_GLOBAL clips each of the three lists once, by its own threshold.  Train stats: the policy
    // row, then the value row, both with the norms of the one joint trunk gradient.
    int joint_apply(hipStream_t st);
    // Behaviour-cloning pass: pass_forward as it is, then the clone loss in the place of the policy loss; with
    // returns the value loss and the joint tail as in a joint pass (and its B <= 2048 limit).  policy_weight / value_weight scale the
    // two losses' dlin (through their grad_scale, next to inv_world), nothing else.  Followed by policy_apply, or joint_apply with returns.
    int clone_forward_backward(const CloneBatch& b, float policy_weight, float value_weight, float aux_weight, float inv_world,
                               hipStream_t st);
    // Representation pass: train-mode trunk forward, the NT-Xent loss on the trunk's output (rows i and i + B/2: two
    // views of one observation), the trunk's backward.  No head op runs; the heads' gradient slices, lin_*, metrics_p / metrics_v and
    // the aux buffers are not written.  Refuses a frozen learner, an odd B and B > 2048.  Followed by trunk_apply.
    int repr_forward_backward(const float* image, const float* road, const float* vehicle, const float* navigation, float temperature,
                              float inv_world, hipStream_t st);
    // The trunk's optimizer step alone (lr_dynamics, unclipped), then one tick of t_dynamics (Nadam: and of m_cache_dynamics) by a
    // one-thread launch of the chunk-norm kernel's tick (tick_steps).  Nothing of either head, old_policy, the gate block or the
    // train-stats ring is touched.  Refuses a frozen learner and one with the gradient gate (clip_mode = global / skip_nonfinite).
    int trunk_apply(hipStream_t st);
    int update_old_policy(hipStream_t st);
    // inference: trunk (moving stats) + old_policy + value heads
    int predict(const float* image, const float* road, const float* vehicle, const float* navigation,
                float* dist_out /*[B][4A]*/, float* value_out /*[B][4]*/, float* dyn_out /*[B][dyn] or null*/,
                hipStream_t st);
    // training-mode forward only (parity tests): returns pointers inside the workspace
    int trunk_forward_train(const float* image, const float* road, const float* vehicle, const float* navigation,
                            hipStream_t st);
    float* dyn_out() const { return dyn_.p; }
    float* img_feat() const { return feat_.p; }
    float* metrics_policy() const { return metrics_p_; }
    float* metrics_value() const { return metrics_v_; }
    float* metrics_repr() const { return metrics_r_; }
    float* policy_aux() const { return aux_p_; }
    float* value_aux() const { return aux_v_; }
    float* policy_lin() const { return lin_p_.p; }
    float* value_lin() const { return lin_v_.p; }
    DevHP* dev_hp() const { return hp_dev_; }
    // Use another (bound) learner's device hyper-parameter block -- learning rates, clip, AND the Adam step counters -- so
    // that engines built for different minibatch sizes over the same parameter arenas behave as one optimizer.
    // ... and, when both keep a train-stats ring, the owner's ring: the rows of all minibatch sizes land in one sequence.
    void share_hp(const Learner& owner) {
        hp_dev_ = owner.hp_dev_;
        if (stats_ring_ && owner.stats_ring_) stats_ring_ = owner.stats_ring_;
        if (gate_dev_ && owner.gate_dev_) gate_dev_ = owner.gate_dev_;      // one gate block: one set of counters
        if (trust_dev_ && owner.trust_dev_) trust_dev_ = owner.trust_dev_;  // one trust block: one latch
        drop_graphs();      // (captured kernel arguments name the block)
    }
    // Train-stats ring (cfg.train_stats rows; include/cdrl.h): STATS_HEADER int32 words -- [0] rows written since the last reset,
    // [1] rows overwritten before they were read -- then the rows.
    static constexpr int STATS_HEADER = 64, STATS_SCALARS = STATS_NSCALARS, STATS_METRICS = 16;
    int stats_rows() const { return cfg_.train_stats; }
    // tensors of `model` a row carries a norm for (counted from the parameter table: the planner asks before the chunk tables exist)
    int stats_tensors(int model) const {
        int n = 0;
        if (cfg_.train_stats > 0 && !(model == M_TRUNK && frozen()))
            for (const ParamInfo& pi : infos_[model]) n += pi.trainable ? 1 : 0;
        return n;
    }
    int stats_off_norms() const { return STATS_SCALARS + STATS_METRICS; }
    int stats_off_trunk() const { return stats_off_norms() + std::max(stats_tensors(M_POLICY), stats_tensors(M_VALUE)); }
    int stats_width() const { return cfg_.train_stats > 0 ? (stats_off_trunk() + stats_tensors(M_TRUNK) + 3) / 4 * 4 : 0; }
    size_t stats_bytes() const { return ((size_t)STATS_HEADER + (size_t)stats_rows() * stats_width()) * sizeof(float); }
    float* stats_ring() const { return stats_ring_; }
    int stats_reset(hipStream_t caller);
    // Data-parallel overlap: `s` (a caller-owned stream, or null) is made to wait, in the middle of every backward pass, for
    // the point where the gradients of the heads and of the trunk tail (GRUs, feature nets, concat BN + Dense) are final --
    // a collective enqueued on `s` after the pass has been enqueued then runs UNDER the tower's backward.
    void set_comm_stream(hipStream_t s) { sched_.set_comm(s); }
    // First element (inside the trunk's trainable region) of the TAIL tensors: everything registered behind the image tower,
    // i.e. exactly the gradients that are final at the point the communication stream is released.  Fixed by the op list.
    // Frozen trunk: no trunk gradient is ever written and the stream is never released; the whole trunk counts as "not final".
    int64_t tail_offset() const { return frozen() ? tr_size_[M_TRUNK] : tail_off_; }
    bool frozen() const { return cfg_.freeze_trunk != 0; }
    // Gradient gate (clip_mode = global and / or skip_nonfinite): the apply steps take the gated launch sequence (gated_apply)
    bool gate_on() const { return cfg_.clip_mode != 0 || cfg_.skip_nonfinite != 0; }
    GateBlock* host_gate() { return &gate_host_; }
    // Trust-region guard (cfg.trust).  policy_apply of such a learner always takes the gated sequence (skip-only
    // when neither gate option is on); value_apply, joint-free by construction, is never decided by the latch.
    bool trust_on() const { return cfg_.trust != 0; }
    TrustBlock* host_trust() { return &trust_host_; }
    int upload_trust(hipStream_t st);       // the block's host-written head (target_kl, kl_stop_factor, kl_coef) -> device
    // one device-to-host copy of the block behind everything on `st` (waits for it); the device-owned fields to their initial
    // values, enqueued on `st`
    int trust_stats(TrustBlock* out, hipStream_t st);
    int trust_reset_block(hipStream_t st);
    // one device-to-host copy of the block behind everything on `st` (waits for it); counters to zero, enqueued on `st`
    int gate_stats(GateBlock* out, hipStream_t st);
    int gate_reset(hipStream_t st);
    bool graphs_enabled() const { return sched_.graphs(); }
    // Named internal tensors (parity tests: the raw BatchNorm inputs, statistics blocks, max-pool argmax codes and dense
    // pre-activations from which the discrete ReLU6 / max-pool decisions of the last forward are reconstructed)
    // CDRL_GUARD=1: 64 KB canary bands behind every workspace tensor (filled at bind); counts the bands that lost their pattern
    int check_guards(hipStream_t st, int64_t* bad, int64_t* first_off);
    bool named_buffer(const std::string& name, void** p, int64_t* bytes) const {
        auto it = named_.find(name);
        if (it == named_.end()) return false;
        *p = it->second.first;
        *bytes = it->second.second;
        return true;
    }

private:
    struct Tens {
        float* p = nullptr;
        float* g = nullptr;
        int rows = 0, C = 0;
        View v(int coff = 0) const { return make_view(p, C, coff); }
        View gv(int coff = 0) const { return make_view(g, C, coff); }
    };
    struct PRef {
        float* p = nullptr;
        float* g = nullptr;
    };
    // reduction scratch of the ops on the main stream / of the auxiliary ops (feature nets + small GRUs) / of the shortcut branch of a
    // stride-2 unit, which run concurrently on other streams and therefore need their own
    struct Scratch {
        double* part = nullptr;
        double* part2 = nullptr;
        float* tn = nullptr;
    };
    // One BatchNorm of the graph: its parameters and blocks (make_bn).  They exist before any op is emitted, so the conv in front of
    // it, its own op and the ops behind it all refer to the same record.
    struct BnRec {
        std::string name;
        int G = 0, Mg = 0, C = 0, nb = 0;  // nb: partial rows per group of its own reductions
        View x{nullptr, 0, 0};             // its raw input
        int act = 0;
        int at = 0;                        // x is a bf16 tensor (tower BatchNorm of a bf16-storage build)
        bool batched_inf = false;          // trunk: the inference-mode statistics block comes from the batched launch
        PRef gamma, beta, mm, mv;
        float* stats = nullptr;            // [4][G][C] of this BatchNorm
        float* coef = nullptr;             // [3][G][C] backward coefficients
        Scratch* scr = nullptr;            // partials of the stream the BatchNorm runs on
        int bwd_nb = 0;                    // partial rows per group its backward sums are left in (set by whoever plans their producer)
        explicit operator bool() const { return C > 0; }
    };
    // Backward form of a 1x1 conv of the tower
    enum class PwBwd {
        Plain,      // dy materialised by the BatchNorm behind the conv; backward-data + filter gradient as two GEMMs
        Prologue,   // BatchNorm-backward apply as operand prologue of those two GEMMs (persistent float32 / bf16 kernel)
        Wide,       // the same with backward-data on the one-tile-per-workgroup split-precision kernel (stage 2, float32)
        Fused,      // one kernel for backward-data + filter + bias gradient (gemm_pw_bwd.hip)
        FusedFin    // ... which also finalizes the BatchNorm behind the conv on load (float32)
    };
    static bool pw_fused(PwBwd f) { return f == PwBwd::Fused || f == PwBwd::FusedFin; }
    // GEMM entry of a 1x1 conv's forward / backward-data: split-precision pw_x3 (forward only), persistent pw_nn, gemm_x3, gemm_nn
    enum class PwGemm { X3, PwNN, GemmX3, GemmNN };
    // A 1x1 conv of the tower as its builder describes it (plan_pw, add_pw)
    struct PwConv {
        std::string name;                    // parameter prefix
        View in{nullptr, 0, 0};
        int rows = 0, Cin = 0, Cout = 0;
        float* y = nullptr;                  // raw output [rows][Cout]
        View din{nullptr, 0, 0};
        int din_acc = 0;
        // forms != Plain (dy is never materialised): the gradient w.r.t. the output of the BatchNorm behind the conv.  ld == 0: the current
        // scratch slot (dense), left there by the op upstream; else the conv's backward claims the rotating slot itself (nobody upstream did)
        View dz{nullptr, 0, 0};
        int dz_shuffle = 0, dz_act = 0;
    };
    // Every kernel choice of one 1x1 conv, decided before any op of its unit is emitted (plan_pw).  The unit builder asks once and hands
    // the same value to add_pw and to the BatchNorm ops around the conv (BnOp::conv, DwBlock::pre_conv / post_conv).
    struct ConvPlan {
        PwGemm fwd = PwGemm::GemmNN;
        PwBwd bwd = PwBwd::Plain;
        PwGemm dgrad = PwGemm::GemmNN;       // backward-data GEMM of Plain (Prologue: pw_nn too; Wide, Fused*: the form's own kernel)
        int stats_nb = 0;                    // > 0: rows per group of statistics partials (BatchNorm behind the conv) the forward epilogue writes
        int bwd_nb = 0;                      // partial rows per group of the backward-data pass (bias sums, sums of the BatchNorm in front)
        // the BatchNorm in front is applied on load (the conv input is its raw input): its backward sums come out of the conv's
        // backward -- the backward-data epilogue, or the reduce kernel of the fused form, which leaves nothing for its own op
        bool bn_in = false;
    };
    // fused: BatchNorm work folded into the unit's convs (persistent / split-precision kernels); bb: and BatchNorm-backward apply as prologue
    ConvPlan plan_pw(const PwConv& c, bool fused, bool bb, bool bn_in);
    // How a BatchNorm's op runs (add_bn)
    struct BnOp {
        bool bessel = true;
        View out{nullptr, 0, 0}, dout{nullptr, 0, 0};
        int out_shuffle = 0, dout_shuffle = 0;
        float* dx = nullptr;                 // nullptr: tower mode, the gradient w.r.t. the input goes to the current scratch slot
        ConvPlan conv;                       // the conv in front.  stats_nb > 0: it wrote the statistics partials; bwd != Plain: it applies this
                                             // BatchNorm's backward on load, FusedFin finalizes it too
        bool sums_by_producer = false;       // the op that produces the incoming gradient accumulates the backward sums in its pass
        Passthrough pass;
    };
    // Fused depthwise block (add_dw_block); the input side comes first, so that a call site spells it as one aggregate
    struct DwBlock {
        float* x = nullptr;                  // block input [N*H*W][C]: raw input of `pre`, or the activated tensor without one
        int H = 0, W = 0, C = 0, stride = 1;
        View din{nullptr, 0, 0};             // gradient target when there is no pre-BN
        BnRec pre;                           // BatchNorm (+ReLU6) in front, or none
        ConvPlan pre_conv;                   // the conv in front of `pre` (as BnOp::conv)
        std::string dw, bn_post;             // parameter prefixes of the depthwise conv and the BatchNorm behind it
        float* y2 = nullptr;                 // raw depthwise output
        View out{nullptr, 0, 0}, dout{nullptr, 0, 0};
        // the conv behind.  bn_in: it applies the post-BN on load: its output is not materialised, and its backward sums come from that
        // conv -- bwd_nb rows per group from the backward-data epilogue, or everything from the fused form's reduce kernel
        ConvPlan post_conv;
    };
    // Second half of a unit branch (add_half): `d` carries the input side of its depthwise block (x .. pre_conv)
    struct Half {
        std::string unit;
        const char *dw, *bn_mid, *pw, *bn_out;      // layer names: dw / bn2 / pw2 / bn3 or sc_dw / sc_bn1 / sc_pw / sc_bn2
        DwBlock d;
        Tens out;                            // unit output
        int out_off = 0;                     // channel offset of this half before the shuffle
        int Cout = 0;
        bool fused = false, bb = false;      // BatchNorm work folded into the 1x1 conv; BatchNorm-backward apply as its operand prologue
        Passthrough pass;
    };

    // --- building
    void build(bool dry);
    float* alloc(size_t n);
    double* alloc_d(size_t n);
    Tens tens(int rows, int C, bool grad = true);
    // tower tensor in the activation type of the build (float32, or bf16 with Config::compute == 2); same Tens / View spelling,
    // p and g then point to bf16 elements (ld and channel offsets count elements)
    Tens tens_a(int rows, int C, bool grad = true);
    int at_ = 0;            // activation type of the tower: 0 float32, 1 bf16 (compute == 2)
    size_t esz() const { return at_ ? 2 : 4; }
    PRef param(int model, const std::string& name, std::initializer_list<int> shape, bool trainable);
    void build_trunk(std::vector<Op>& ops);
    void build_head(std::vector<Op>& ops, int model, const std::string& prefix, Tens& lin, int nheads,
                    const int* head_dims, const char* const* head_names);
    // make_bn registers a BatchNorm's parameters and allocates its blocks; add_bn emits its op.  pw_bn: the BatchNorm behind the 1x1
    // conv `conv`, whose own parameters are registered first (the parameter tables keep layer order wherever the blocks are created)
    BnRec make_bn(int model, const std::string& prefix, View x, int G, int Mg, int C, int act);
    BnRec pw_bn(const std::string& conv, int Cin, int Cout, const std::string& bn, float* y, int Mg, int act);
    // (returns whether the op took the single-launch form: bn_small_fwd / bn_small_bwd)
    bool add_bn(std::vector<Op>& ops, const BnRec& bn, const BnOp& o);
    // dense BatchNorm between two tensors (feature nets, trunk tail, control branches): no Bessel correction, no activation
    void add_dense_bn(std::vector<Op>& ops, int model, const std::string& prefix, const Tens& in, const Tens& out, int G);
    // emits what the plan says (bn_in: the record behind ConvPlan::bn_in, or none); the backward is one of three programs, chosen at build time
    void add_pw(std::vector<Op>& ops, const PwConv& c, const ConvPlan& plan, const BnRec& bn_in, const BnRec& bn_out);
    // which instantiations of the 1x1-conv family the built ops launch ("nn ok ksm nt pro epi mode acc", "x3 ok form kp nt pro epi",
    // "x3b ok sh epi acc"), noted while they are built
    std::set<std::string> pw_sigs_;
    void note_pw(const char* kind, std::initializer_list<int> fields);
    void note_pw(const PwNnPlan& p);
    void note_pw(const PwX3Plan& p);
    void note_pw(const PwX3BwdPlan& p);
    struct PwEmit {                          // what add_pw hands to the backward emitter of the plan's form
        PwConv c;
        ConvPlan plan;
        BnRec bn_in, bn_out;
        PRef w, b;
        const float* wpb = nullptr;          // packed W^T: float32 / bf16 MFMA fragment order (persistent kernel),
        const void *wpx = nullptr, *g3b = nullptr;      // three bf16 planes (fused and wide form), gemm_x3's
    };
    std::function<int(hipStream_t)> pw_bwd_fused_op(const PwEmit& e);
    std::function<int(hipStream_t)> pw_bwd_prologue_op(const PwEmit& e);
    std::function<int(hipStream_t)> pw_bwd_plain_op(const PwEmit& e);
    // pre_bn: the op also accumulates the backward sums of that BatchNorm (the layer that produced `in`)
    void add_dw(std::vector<Op>& ops, const std::string& prefix, View in, int N, int H, int W, int C, int stride,
                float* y, View din, int din_acc, const BnRec* pre_bn = nullptr);
    // Fused depthwise block (dwfused.hip): [BN `pre` (+ReLU6) of the raw 1x1-conv output x, or none] -> dw3x3 -> BN `bn_post` (no
    // activation) -> out.  Emits three ops (pre-BN, depthwise, post-BN); the normalised depthwise input and the post-BN input
    // gradient never touch HBM.  Returns the post-BN.
    BnRec add_dw_block(std::vector<Op>& ops, const DwBlock& d);
    // Depthwise block, then 1x1 conv, then BN + ReLU6 into a shuffled half of the unit output: the second half of a main branch and the
    // whole shortcut branch of a stride-2 unit (core/architectures.py:126-137)
    void add_half(std::vector<Op>& ops, const Half& h);
    bool fused_dw_ = true, fused_pw_ = true, fused_bb_ = true;
    bool fused_bwd_ = true;             // backward-data + filter gradient of the unit convs as one kernel (gemm_pw_bwd.hip)
    void add_dense(std::vector<Op>& ops, int model, const std::string& prefix, View in, int M, int K, int N, int act,
                   View out, View dout, View din, int din_acc, bool need_din, const char* bias_init);
    void add_gru(std::vector<Op>& ops, const std::string& name, Tens& x, int In, int u, View out, View dout,
                 bool need_dx);
    void note_scratch(size_t part_d, size_t part2_d, size_t dy_f, size_t tn_f, size_t fpart_d = 0);

    // Every public step runs on the scheduler's main stream (bridged to the caller's stream with
    // events) and, when `graphable`, is captured once into a hipGraph (main + side stream, ~1000
    // kernel nodes per pass) and replayed afterwards: the update-step is launch-bound on the host
    // otherwise (measured: 22 ms of CPU enqueue time per 30 ms update-step).  The cache key is the
    // step kind + every pointer / scalar argument baked into the captured kernel arguments.
    int launch(hipStream_t caller, std::vector<uint64_t> key, bool graphable, const std::function<int(hipStream_t)>& body);
    void drop_graphs();
    StreamSched sched_;                 // the streams and everything that orders them (sched.h)
    std::map<std::vector<uint64_t>, hipGraphExec_t> graphs_;
    // One training pass as its entry point describes it: the state pointers, the policy part (adv .. du_db) and / or the value part
    // (returns; both: the joint pass), the one speed / similarity pair, the device re-sampling and the gradient scale
    struct PassSpec {
        const float *image, *road, *vehicle, *navigation, *speed, *similarity;
        const PolicyBatch* policy;          // its adv, old_logp, u, du_da, du_db; or null
        const float* returns;               // or null
        float inv_world;
        bool resample = false;              // u, du_da, du_db: drawn on the device from the new policy with (seed, offset), not the batch's
        uint64_t seed = 0, offset = 0;
        // clone mode (policy is null): the clone loss on (clone_u, clone_w) stands where the policy loss stands
        const float *clone_u = nullptr, *clone_w = nullptr;
        // demonstration mode (policy is set): the mixed loss on (demo_u, demo_w) stands where the policy loss stands
        const float *demo_u = nullptr, *demo_w = nullptr;
        float policy_weight = 1.0f, value_weight = 1.0f, aux_weight = 1.0f;
        // representation mode (policy, returns, clone_u all null): the NT-Xent loss on the trunk's output, no head at all
        bool repr = false;
        float temperature = 0.0f;
        bool head() const { return policy || clone_u; }      // the policy head takes part
        bool joint() const { return head() && returns; }
    };
    static PassSpec policy_pass(const PolicyBatch& b, const float* returns, float inv_world, bool resample = false, uint64_t seed = 0,
                                uint64_t offset = 0) {
        return {b.image, b.road, b.vehicle, b.navigation, b.speed, b.similarity, &b, returns, inv_world, resample, seed, offset};
    }
    PolicyLossArgs policy_loss_args(const PassSpec& s) const;
    CloneLossArgs clone_loss_args(const PassSpec& s) const;
    MixedPolicyLossArgs mixed_loss_args(const PassSpec& s) const;
    DemoBlock* demo_block_ = nullptr;
    int demo_pass(PassSpec s, const float* demo_u, const float* demo_w, hipStream_t caller);
    ValueLossArgs value_loss_args(const PassSpec& s) const;
    NtxentArgs ntxent_args(const PassSpec& s) const;
    // forward half: trunk, the heads present (dist: policy_dist behind the policy head; re-sampling: and the Beta draw, both in
    // front of the value head); backward half: per head its loss and backward, joint: bn_small_bwd_pair, then the trunk
    int pass_forward(const PassSpec& s, bool dist, hipStream_t st);
    int pass_backward(const PassSpec& s, hipStream_t st);
    int trunk_backward_tail(hipStream_t st);
    // entry of every pass (fwd / bwd: the halves to run): gradient-scale hint, graph key, graph replay or eager launch
    int run_pass(const PassSpec& s, hipStream_t caller, bool fwd = true, bool bwd = true);
    int update_old_policy_impl(hipStream_t st, const GateBlock* gate = nullptr);
    ArenaSlice arena_slice(int model) const;      // the trainable slice of a model in params / grads / adam_m / adam_v
    // the ungated apply of one head (0 policy, 1 value); with_trunk = false: as gated_apply's
    int head_apply(int head, bool with_trunk, hipStream_t st);
    int policy_apply_impl(hipStream_t st);
    int value_apply_impl(hipStream_t st);
    int joint_apply_impl(hipStream_t st);
    int trunk_apply_impl(hipStream_t st);
    int repr_refused();
    int joint_refused();
    int predict_impl(const float* image, const float* road, const float* vehicle, const float* navigation, float* dist_out,
                     float* value_out, float* dyn_out, hipStream_t st);
    int run_fwd(std::vector<Op>& ops, hipStream_t st, int training);
    int run_bwd(std::vector<Op>& ops, hipStream_t st, size_t first = 0);      // ops [first, size) in reverse order
    int set_inputs(const float* image, const float* road, const float* vehicle, const float* navigation);

    Config cfg_;
    std::vector<ParamInfo> infos_[3];
    std::unordered_map<std::string, int> index_[3];
    int64_t tr_size_[3] = {0, 0, 0}, st_size_[3] = {0, 0, 0};
    bool table_frozen_ = false;

    Buffers buf_;
    bool dry_ = true;
    char* ws_base_ = nullptr;
    size_t ws_off_ = 0, ws_bytes_ = 0;
    static constexpr size_t GUARD_BYTES = 65536, GUARD_TABLE_MAX = 131072;
    bool guard_ = false;
    std::vector<int64_t> guard_off_;        // byte offsets of the bands (real build)
    int64_t* guard_tab_ = nullptr;          // device copy + [GUARD_TABLE_MAX]: bad count, [+1]: first bad band
    void add_guard();
    // scratch maxima (from the dry build) and pointers
    size_t max_part_ = 0, max_part2_ = 0, max_dy_ = 0, max_tn_ = 0, max_fpart_ = 0;
    // the same maxima over the ops built outside the trunk (heads): what the rotating slots must hold on a frozen learner
    bool building_trunk_ = false;
    size_t head_part2_ = 0, head_tn_ = 0;
    struct SlotSizes { size_t dy, part2, tn, fpart, qpart, dbpart, fintot; };
    SlotSizes slot_sizes() const;
    void alloc_scratch();               // main / aux / shortcut scratch, the NSLOT rotating slots, the NQ ring
    Scratch scr_main_, scr_aux_, scr_sc_;
    Scratch* build_scr_ = &scr_main_;
    std::vector<Op> aux_ops_;
    void add_aux_fork(std::vector<Op>& ops);
    void add_aux_join(std::vector<Op>& ops);
    // Rotating scratch sets of the backward's side jobs (dy, db partials, split-M partials, filter partials), indexed by sched_.slot()
    static constexpr int NSLOT = StreamSched::NSLOT;
    float* dys_[NSLOT] = {};
    double* part2s_[NSLOT] = {};
    float* tns_[NSLOT] = {};
    double* fparts_[NSLOT] = {};
    // fused conv backward: per-workgroup filter-product tiles / column sums.  Their own small ring (the tiles are large: 16-21 MB per
    // conv at B = 256), indexed by sched_.q()
    static constexpr int NQ = StreamSched::NQ;
    float* qparts_[NQ] = {};
    double* dbparts_[NQ] = {};
    double* fintots_[NQ] = {};           // [8][2][128] group totals of a finalize-on-load BatchNorm (gemm_pw_bwd.hip)
    bool fin_on_load_ = true;            // the fused conv backward finalizes the BatchNorm behind it on load (CDRL_FIN_ON_LOAD=0: stand-alone launches)
    size_t max_qpart_ = 0, max_dbpart_ = 0;
    bool packs_have_wt_ = false;                        // the last forward's pack launch also wrote the W^T copies of the backward

    std::vector<Op> trunk_ops_, policy_ops_, value_ops_, old_policy_ops_;
    // live input pointers (read by the first ops through these slots)
    const float* in_image_ = nullptr;
    const float* in_road_ = nullptr;
    const float* in_vehicle_ = nullptr;
    const float* in_navigation_ = nullptr;

    Tens dyn_, feat_, lin_p_, lin_v_, lin_old_;
    // The first BatchNorm of the policy ([0]) and value ([1]) head, both over dyn_: the joint pass runs the rest of a head's backward
    // (ops behind `op`) and then both of these in one launch
    struct HeadBn0 {
        BnRec bn;
        View dout{nullptr, 0, 0};
        size_t op = 0;              // index of its op in the head's list
        bool small = false;         // single-launch form
    } bn0_[2];
    float *metrics_p_ = nullptr, *metrics_v_ = nullptr, *aux_p_ = nullptr, *aux_v_ = nullptr;
    // representation pass: its 16 metrics sit behind the policy's in one allocation unit; the loss's scratch is backward slot 0's
    // tower-gradient block, idle between the end of the trunk forward and the first backward op (its own block only where that one
    // is too small).  Neither adds a byte to the workspace of a learner that never runs the pass.
    float *metrics_r_ = nullptr, *ntxent_ws_ = nullptr;
    float *sample_u_ = nullptr, *sample_da_ = nullptr, *sample_db_ = nullptr;
    DevHP hp_host_;
    DevHP* hp_dev_ = nullptr;
    DevHP* hp_stage_ = nullptr;     // pinned host staging (DevHP, and one float behind it for the gate block's threshold)
    GateBlock gate_host_;           // only clip_norm_dynamics is the host's
    GateBlock* gate_dev_ = nullptr; // in the workspace of a learner with gate_on() or trust_on() (this learner's, or the hyper-parameter owner's)
    TrustBlock trust_host_;         // its first TRUST_HOST_WORDS floats are the host's
    TrustBlock* trust_dev_ = nullptr;       // in the workspace of a learner with trust_on() (this learner's, or the owner's)
    int trust_refused(const PassSpec& s);   // an anchor without cfg.trust, a joint pass with it
    // with_trunk = false (the value head of a joint apply, whose trunk step the policy head's gated apply took): the head alone --
    // no trunk norm in the decision, no trunk update, no trunk tick
    int gated_apply(int head, hipStream_t st, bool with_trunk = true);
    // the trunk has a chunk table: its norms are wanted by the train stats or by the gate
    bool trunk_table() const { return !frozen() && (cfg_.train_stats > 0 || gate_on()); }
    // optimiser tables (device, inside workspace)
    struct SegTable {
        ChunkTable dev;
        std::vector<TensorSeg> h_segs;
        std::vector<int> h_chunk_tensor;
        std::vector<int64_t> h_chunk_off;
    } seg_[3];
    void build_seg_tables();
    float* stats_ring_ = nullptr;           // header + rows (this learner's, or the hyper-parameter owner's)
    int stats_row(int kind, hipStream_t st);    // the tail of an apply step: trunk chunk norms, per-tensor fold, row writer
    int upload_seg_tables();
    // transposed copies of weights for backward GEMMs (the GRUs' recurrent kernels; the unit convs read packed W^T fragments instead):
    // refreshed by the pack launch at the start of every training forward
    std::vector<PwTranspose> h_pwt_;
    std::map<std::string, float*> pwt_by_name_;
    PwTranspose* d_pwt_ = nullptr;
    int pwt_tiles_ = 0;
    // pointwise-conv weights in MFMA fragment order (forward operand W, backward-data operand W^T), re-packed by ONE launch
    // at the start of every trunk forward: the per-workgroup weight prologue of the persistent GEMM becomes KSM/4 16-byte loads
    std::string build_err_;                 // first configuration error met while the op lists were built (reported by create)
    void build_fail(const char* fmt, ...);
    // inference-mode BatchNorm statistics of the trunk (tower + trunk tail, main and aux streams): one batched launch at the
    // start of an inference forward instead of one per layer (bn_inference_stats_many)
    std::vector<BnInfEntry> h_bninf_;
    BnInfEntry* d_bninf_ = nullptr;
    int bninf_max_c_ = 0;
    void note_bn_inference(const float* gamma, const float* beta, const float* mm, const float* mv, float* stats, int G, int C);
    std::vector<PwPack> h_pack_;
    PwPack* d_pack_ = nullptr;
    float* pw_packed(const float* w, int K, int N, int sbk, int sbn, bool bf16 = false);
    std::vector<PwX3Pack> h_pack3_;         // three-plane bf16 fragments of the convs that run on the bf16 matrix pipe (gemm_pw_x3.hip)
    PwX3Pack* d_pack3_ = nullptr;
    const void* pw_x3_packed(const float* w, int K, int N, int sbk, int sbn);
    std::vector<GemmX3Pack> h_gpack_;       // general split-precision GEMM operands (head conv, wide shortcut convs: gemm_x3.hip)
    GemmX3Pack* d_gpack_ = nullptr;
    const void* gemm_x3_packed(const float* w, int K, int N, int sbk, int sbn);
    int run_trunk_fwd(hipStream_t st, int training);
    int64_t tail_off_ = 0;
    std::vector<std::pair<void*, size_t>> zero_once_;    // workspace regions that must read as zero and are never written
    float* pw_transposed(const std::string& name, const float* w, int cin, int cout);
    bool tables_uploaded_ = false;
    std::map<std::string, std::pair<void*, int64_t>> named_;
    void note_named(const std::string& name, const void* p, size_t bytes) {
        if (!dry_) named_[name] = std::make_pair(const_cast<void*>(p), (int64_t)bytes);
    }
};

}  // namespace cdrl

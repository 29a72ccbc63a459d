// Learner engine implementation (host side, gfx950 kernels from the sibling .hip files).
//
// Mirrors the structure built by the reference's Keras graph builders:
//   trunk  = dynamics_layers            (reference core/networks.py:37-56)
//            shufflenet_v2 over T slices (core/architectures.py:30-173)
//            feature_net x3             (core/architectures.py:9-27)
//   heads  = control_branch + policy / value heads (core/networks.py:59-66,115-137,255-275)
//   steps  = get_*_gradients / apply_*_gradients   (core/carla_agent.py:351-388,430-463;
//                                                    rl/agents/ppo.py:238-275)
// Frames are ordered f = t*B + b, so each per-time-slice BatchNorm group is a contiguous row
// range (F6); split / concat / channel_shuffle never materialise on their own: they are views
// (ld, channel offset) plus a destination-index permutation in the BN-apply store (F7).
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>

#include "engine.h"
#include "../../include/cdrl.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace cdrl {

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int same_out_h(int n, int s) { return (n + s - 1) / s; }
// path switch: on unless the variable is set to 0
static inline bool env_on(const char* name) { return !(cdrl_getenv(name) && atoi(cdrl_getenv(name)) == 0); }

Learner::Learner(const Config& cfg) : cfg_(cfg) {
    memset(&hp_host_, 0, sizeof(hp_host_));
    hp_host_.lr_policy = 3e-4f;
    hp_host_.lr_value = 3e-4f;
    hp_host_.lr_dynamics = 3e-4f;
    hp_host_.clip_ratio = 0.2f;
    hp_host_.entropy_coef = 1.0f;
    hp_host_.clip_norm_policy = 1.0f;
    hp_host_.clip_norm_value = 1.0f;
    hp_host_.beta1 = 0.9f;
    hp_host_.beta2 = 0.999f;
    hp_host_.eps = 1e-7f;
    hp_host_.m_cache_policy = hp_host_.m_cache_value = hp_host_.m_cache_dynamics = 1.0f;
    memset(&gate_host_, 0, sizeof(gate_host_));
    gate_host_.scale_head = gate_host_.scale_trunk = 1.0f;
    for (int h = 0; h < 2; ++h) gate_host_.last_scale[h][0] = gate_host_.last_scale[h][1] = 1.0f;
    memset(&trust_host_, 0, sizeof(trust_host_));
    trust_host_.kl_stop_factor = 1.5f;
    trust_host_.stop_pass = -1;
    at_ = cfg_.compute == 2 ? 1 : 0;
    guard_ = cdrl_getenv("CDRL_GUARD") && atoi(cdrl_getenv("CDRL_GUARD")) == 1;
    build(true);
    table_frozen_ = true;
    build_seg_tables();
}

Learner::~Learner() {
    if (hp_stage_) (void)hipHostFree(hp_stage_);
    drop_graphs();
}

void Learner::drop_graphs() {
    for (auto& kv : graphs_) (void)hipGraphExecDestroy(kv.second);
    graphs_.clear();
}

int Learner::launch(hipStream_t caller, std::vector<uint64_t> key, bool graphable,
                    const std::function<int(hipStream_t)>& body) {
    CDRL_TRY(sched_.hand_in(caller));       // (refuses a learner that is not bound)
    hipStream_t main = sched_.main();
    int rc = 0;
    if (!sched_.graphs() || !graphable) {
        sched_.begin_body(key);
        rc = body(main);
        sched_.end_body();
    } else {
        auto it = graphs_.find(key);
        if (it == graphs_.end()) {
            if (graphs_.size() >= 32) drop_graphs();
            hipGraph_t graph = nullptr;
            CDRL_HIP(hipStreamBeginCapture(main, hipStreamCaptureModeRelaxed));
            rc = body(main);
            hipError_t ce = hipStreamEndCapture(main, &graph);
            if (rc != 0 || ce != hipSuccess || !graph) {
                if (graph) (void)hipGraphDestroy(graph);
                if (rc == 0) {
                    set_error("hipStreamEndCapture failed: %s", hipGetErrorString(ce));
                    rc = -2;
                }
                return rc;
            }
            hipGraphExec_t exec = nullptr;
            hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ie != hipSuccess) {
                set_error("hipGraphInstantiate failed: %s", hipGetErrorString(ie));
                return -2;
            }
            it = graphs_.emplace(std::move(key), exec).first;
        }
        CDRL_HIP(hipGraphLaunch(it->second, main));
    }
    if (rc != 0) return rc;
    return sched_.hand_out(caller);
}

static const int g_diag_skip_fin = cdrl_getenv("CDRL_DIAG_SKIP_FIN") ? atoi(cdrl_getenv("CDRL_DIAG_SKIP_FIN")) : 0;   // timing diagnostics only (stale statistics)
static const int g_diag_skip_aux = cdrl_getenv("CDRL_DIAG_SKIP_AUX") ? atoi(cdrl_getenv("CDRL_DIAG_SKIP_AUX")) : 0;   // timing diagnostics only (wrong results)

int64_t Learner::tr_offset(int model) const {
    switch (model) {
        case M_POLICY: return 0;
        case M_TRUNK: return tr_size_[M_POLICY];
        case M_VALUE: return tr_size_[M_POLICY] + tr_size_[M_TRUNK];
        default: return grads_total() + st_size_[0] + st_size_[1] + st_size_[2];      // old policy trainable
    }
}

int64_t Learner::st_offset(int model) const {
    const int64_t base = grads_total();
    switch (model) {
        case M_POLICY: return base;
        case M_TRUNK: return base + st_size_[M_POLICY];
        case M_VALUE: return base + st_size_[M_POLICY] + st_size_[M_TRUNK];
        default: return tr_offset(M_OLD_POLICY) + tr_size_[M_POLICY];                  // old policy state
    }
}

int64_t Learner::params_total() const { return st_offset(M_OLD_POLICY) + st_size_[M_POLICY]; }

// ------------------------------------------------------------------------------------------
// allocation helpers
// ------------------------------------------------------------------------------------------
// CDRL_GUARD=1: a canary band behind every bump allocation (the only out-of-bounds detector this stack has for kernels that address
// the workspace through raw buffer descriptors: an overrun into the neighbour tensor is otherwise seen only if a parity test reads it)
void Learner::add_guard() {
    if (!guard_) return;
    if (!dry_) guard_off_.push_back((int64_t)ws_off_);
    ws_off_ += GUARD_BYTES;
}

float* Learner::alloc(size_t n) {
    const size_t bytes = align_up(n * sizeof(float), 256);
    float* p = dry_ ? nullptr : reinterpret_cast<float*>(ws_base_ + ws_off_);
    ws_off_ += bytes;
    add_guard();
    return p;
}

double* Learner::alloc_d(size_t n) {
    const size_t bytes = align_up(n * sizeof(double), 256);
    double* p = dry_ ? nullptr : reinterpret_cast<double*>(ws_base_ + ws_off_);
    ws_off_ += bytes;
    add_guard();
    return p;
}

static constexpr uint32_t GUARD_PATTERN = 0xA5C3961Eu;

__global__ void __launch_bounds__(256) guard_fill_kernel(char* base, const int64_t* __restrict__ offs, int words) {
    uint32_t* p = reinterpret_cast<uint32_t*>(base + offs[blockIdx.x]);
    for (int i = threadIdx.x; i < words; i += 256) p[i] = GUARD_PATTERN ^ (uint32_t)i;
}

__global__ void __launch_bounds__(256) guard_check_kernel(const char* base, const int64_t* __restrict__ offs, int words, int64_t* out) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(base + offs[blockIdx.x]);
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    int b = 0;
    for (int i = threadIdx.x; i < words; i += 256) b |= p[i] != (GUARD_PATTERN ^ (uint32_t)i);
    if (b) bad = 1;          // (benign race: every writer stores 1)
    __syncthreads();
    if (threadIdx.x == 0 && bad) {
        atomicAdd(reinterpret_cast<unsigned long long*>(out), 1ull);
        atomicMin(reinterpret_cast<long long*>(out + 1), (long long)blockIdx.x);
    }
}

int Learner::check_guards(hipStream_t st, int64_t* bad, int64_t* first_off) {
    if (!guard_ || !guard_tab_) {
        set_error("check_guards: the learner was not created with CDRL_GUARD=1 (or is not bound)");
        return -1;
    }
    const int n = (int)guard_off_.size();
    int64_t init[2] = {0, (int64_t)1 << 40};
    CDRL_HIP(hipMemcpyAsync(guard_tab_ + GUARD_TABLE_MAX, init, sizeof(init), hipMemcpyHostToDevice, st));
    tail_invalidate(st);
    hipLaunchKernelGGL(guard_check_kernel, dim3(n), dim3(256), 0, st, ws_base_, guard_tab_, (int)(GUARD_BYTES / 4), guard_tab_ + GUARD_TABLE_MAX);
    CDRL_LAUNCH_CHECK();
    int64_t out[2];
    CDRL_HIP(hipMemcpyAsync(out, guard_tab_ + GUARD_TABLE_MAX, sizeof(out), hipMemcpyDeviceToHost, st));
    tail_invalidate(st);
    CDRL_HIP(hipStreamSynchronize(st));
    if (bad) *bad = out[0];
    if (first_off) *first_off = out[0] ? guard_off_[(size_t)out[1]] : -1;
    return 0;
}

Learner::Tens Learner::tens(int rows, int C, bool grad) {
    Tens t;
    t.rows = rows;
    t.C = C;
    t.p = alloc((size_t)rows * C);
    if (grad) t.g = alloc((size_t)rows * C);
    return t;
}

Learner::Tens Learner::tens_a(int rows, int C, bool grad) {
    Tens t;
    t.rows = rows;
    t.C = C;
    const size_t n = ((size_t)rows * C * esz() + 3) / 4;        // float-sized slots
    t.p = alloc(n);
    if (grad) t.g = alloc(n);
    return t;
}

Learner::PRef Learner::param(int model, const std::string& name, std::initializer_list<int> shape, bool trainable) {
    const int tm = model == M_OLD_POLICY ? (int)M_POLICY : model;
    int idx;
    auto it = index_[tm].find(name);
    if (it == index_[tm].end()) {
        if (table_frozen_ || model == M_OLD_POLICY) {
            set_error("unknown parameter %s", name.c_str());
            return PRef();
        }
        ParamInfo pi;
        pi.name = name;
        pi.ndim = (int)shape.size();
        int64_t n = 1;
        int k = 0;
        for (int d : shape) {
            pi.shape[k++] = d;
            n *= d;
        }
        pi.numel = n;
        pi.trainable = trainable ? 1 : 0;
        pi.model = tm;
        int64_t& sz = trainable ? tr_size_[tm] : st_size_[tm];
        pi.off = sz;
        sz += (n + 3) / 4 * 4;           // 16-byte aligned tensor starts
        idx = (int)infos_[tm].size();
        infos_[tm].push_back(pi);
        index_[tm][name] = idx;
    } else {
        idx = it->second;
    }
    PRef r;
    if (dry_) return r;
    const ParamInfo& pi = infos_[tm][idx];
    if (pi.trainable) {
        r.p = buf_.params + tr_offset(model) + pi.off;
        if (model != M_OLD_POLICY) r.g = buf_.grads + tr_offset(model) + pi.off;
    } else {
        r.p = buf_.params + st_offset(model) + pi.off;
    }
    return r;
}

float* Learner::pw_transposed(const std::string& name, const float* w, int cin, int cout) {
    auto it = pwt_by_name_.find(name);
    if (it != pwt_by_name_.end()) return it->second;
    float* wt = alloc((size_t)cin * cout);
    pwt_by_name_[name] = wt;
    h_pwt_.push_back(PwTranspose{w, wt, cin, cout});
    pwt_tiles_ = std::max(pwt_tiles_, ((cin + 31) / 32) * ((cout + 31) / 32));
    return wt;
}

void Learner::build_fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (build_err_.empty()) build_err_ = buf;
}

float* Learner::pw_packed(const float* w, int K, int N, int sbk, int sbn, bool bf16) {
    float* wp = alloc((size_t)pw_packed_elems(N, K));
    h_pack_.push_back(pw_pack_entry(w, wp, K, N, sbk, sbn, bf16));
    return wp;
}

const void* Learner::pw_x3_packed(const float* w, int K, int N, int sbk, int sbn) {
    void* wp = alloc((size_t)pw_x3_packed_bytes_n(K, N) / sizeof(float));
    h_pack3_.push_back(pw_x3_pack_entry(w, wp, K, N, sbk, sbn));
    return wp;
}

const void* Learner::gemm_x3_packed(const float* w, int K, int N, int sbk, int sbn) {
    void* wp = alloc((size_t)gemm_x3_packed_bytes(N, K) / sizeof(float));
    h_gpack_.push_back(gemm_x3_pack_entry(w, wp, K, N, sbk, sbn));
    return wp;
}

void Learner::note_bn_inference(const float* gamma, const float* beta, const float* mm, const float* mv, float* stats, int G, int C) {
    h_bninf_.push_back(BnInfEntry{gamma, beta, mm, mv, stats, G, C});
    if (C > bninf_max_c_) bninf_max_c_ = C;
}

int Learner::run_trunk_fwd(hipStream_t st, int training) {
    if (!training) CDRL_TRY(bn_inference_stats_many(d_bninf_, (int)h_bninf_.size(), bninf_max_c_, st));
    // this pass's weights in fragment order (fwd + bwd-data).  On the side stream beside the stem block, joined behind it: measured twice,
    // 14.29 vs 14.30 ms with round 5's events and 12.46 vs 12.41 ms with round 6's -- three 10-us launches beside the bandwidth-bound stem
    // conv plus a join packet cost what they save; they stay in front of the stem.
    // ... and in ONE launch, with the W^T transposes of the backward (training passes) riding along: four dependent 4-13 us launches per
    // pass became one (pack_all; the weights do not change between here and the backward)
    // (frozen trunk: no backward follows, and the planner registered no backward operand at all)
    packs_have_wt_ = training != 0 && !frozen();
    CDRL_TRY(pack_all(d_gpack_, (int)h_gpack_.size(), d_pack_, (int)h_pack_.size(), d_pack3_, (int)h_pack3_.size(), d_pwt_,
                      packs_have_wt_ ? (int)h_pwt_.size() : 0, pwt_tiles_, st));
    return run_fwd(trunk_ops_, st, training);
}

void Learner::note_scratch(size_t part_d, size_t part2_d, size_t dy_f, size_t tn_f, size_t fpart_d) {
    if (part_d > max_part_) max_part_ = part_d;
    if (part2_d > max_part2_) max_part2_ = part2_d;
    if (dy_f > max_dy_) max_dy_ = dy_f;
    if (tn_f > max_tn_) max_tn_ = tn_f;
    if (fpart_d > max_fpart_) max_fpart_ = fpart_d;
    if (!building_trunk_) {
        if (part2_d > head_part2_) head_part2_ = part2_d;
        if (tn_f > head_tn_) head_tn_ = tn_f;
    }
}

// Sizes of the rotating backward scratch (NSLOT slots, NQ fused-conv ring).  A frozen learner runs the backward of the heads only:
// their dense layers use the slots' part2 / tn blocks (side-stream weight gradients); dy, the filter partials and the ring are
// tower-backward scratch and get no bytes (the allocations stay, empty, so that the guard-band count does not depend on the flag)
Learner::SlotSizes Learner::slot_sizes() const {
    if (frozen()) return SlotSizes{0, head_part2_, head_tn_, 0, 0, 0, 0};
    return SlotSizes{max_dy_, max_part2_, max_tn_, max_fpart_, max_qpart_, max_dbpart_, (size_t)8 * 2 * 128};
}

// ------------------------------------------------------------------------------------------
// op builders
// ------------------------------------------------------------------------------------------
Learner::BnRec Learner::make_bn(int model, const std::string& prefix, View x, int G, int Mg, int C, int act) {
    BnRec r;
    r.name = prefix;
    r.G = G;
    r.Mg = Mg;
    r.C = C;
    r.nb = r.bwd_nb = vcol_geom(Mg, C).nb;
    r.x = x;
    r.act = act;
    const bool tower = model == M_TRUNK && prefix.compare(0, 4, "img.") == 0;
    r.at = tower ? at_ : 0;
    r.gamma = param(model, prefix + ".gamma", {C}, true);
    r.beta = param(model, prefix + ".beta", {C}, true);
    r.mm = param(model, prefix + ".moving_mean", {C}, false);
    r.mv = param(model, prefix + ".moving_var", {C}, false);
    r.stats = alloc((size_t)4 * G * C);
    r.coef = alloc((size_t)3 * G * C);
    r.scr = build_scr_;
    note_named(prefix + ".stats", r.stats, (size_t)4 * G * C * sizeof(float));
    if (x.ld == C && x.coff == 0) note_named(prefix + ".x", x.p, (size_t)G * Mg * C * (tower ? esz() : 4));
    // trunk layers: the inference-mode statistics block comes from the batched launch at the start of the forward
    r.batched_inf = model == M_TRUNK;
    if (r.batched_inf) note_bn_inference(r.gamma.p, r.beta.p, r.mm.p, r.mv.p, r.stats, G, C);
    return r;
}

Learner::BnRec Learner::pw_bn(const std::string& conv, int Cin, int Cout, const std::string& bn, float* y, int Mg, int act) {
    (void)param(M_TRUNK, conv + ".w", {1, 1, Cin, Cout}, true);
    (void)param(M_TRUNK, conv + ".b", {Cout}, true);
    return make_bn(M_TRUNK, bn, make_view(y, Cout), cfg_.T, Mg, Cout, act);
}

void Learner::add_dense_bn(std::vector<Op>& ops, int model, const std::string& prefix, const Tens& in, const Tens& out, int G) {
    BnOp o;
    o.bessel = false;
    o.out = out.v();
    o.dout = out.gv();
    o.dx = in.g;
    add_bn(ops, make_bn(model, prefix, in.v(), G, in.rows / G, in.C, ACT_NONE), o);
}

bool Learner::add_bn(std::vector<Op>& ops, const BnRec& bn, const BnOp& o) {
    const int G = bn.G, Mg = bn.Mg, C = bn.C, nb = bn.nb, act = bn.act, at = bn.at, stats_nb = o.conv.stats_nb, bes = o.bessel ? 1 : 0;
    const View x = bn.x;
    const Passthrough pass = o.pass;
    const bool apply_by_conv = o.conv.bwd != PwBwd::Plain, fin_by_conv = o.conv.bwd == PwBwd::FusedFin;
    Scratch* sc = bn.scr;
    note_scratch((size_t)G * std::max(nb, stats_nb) * 2 * C, (size_t)G * nb * C, 0, 0);
    // single-group BatchNorm over a few hundred rows (dense BNs of the trunk tail and the control branches): one launch per
    // direction instead of three
    const bool small = G == 1 && Mg <= 2048 && !o.bessel && act == ACT_NONE && !o.out_shuffle && !o.dout_shuffle && o.dx &&
                       !stats_nb && !apply_by_conv && !pass.fsrc.p && !pass.gsrc.p && !pass.gap_out;
    const bool gap = pass.gap_out != nullptr;
    std::shared_ptr<int> diag_calls3 = std::make_shared<int>(0);
    if (at && small) build_fail("%s: single-launch BatchNorm has no bf16-storage form", bn.name.c_str());
    if (gap && (pass.gap_rows <= 0 || Mg % pass.gap_rows != 0 || x.ld != C || x.coff != 0 || o.out_shuffle || o.dout_shuffle || pass.fsrc.p ||
                pass.gsrc.p))
        build_fail("%s: fused global average pool needs a dense input and whole frames per group", bn.name.c_str());
    Op op;
    if (small) {
        op.fwd = [=](hipStream_t st, int training) -> int {
            if (training) return bn_small_fwd(x, Mg, C, bn.gamma.p, bn.beta.p, bn.mm.p, bn.mv.p, bn.stats, o.out, st);
            if (!bn.batched_inf) CDRL_TRY(bn_finalize(sc->part, nb, G, Mg, C, bn.gamma.p, bn.beta.p, bn.mm.p, bn.mv.p, bes, training, bn.stats, st));
            return bn_apply(x, G, Mg, C, bn.stats, act, o.out, o.out_shuffle, st);
        };
        op.bwd = [=](hipStream_t st) -> int { return bn_small_bwd(o.dout, x, Mg, C, bn.stats, bn.gamma.g, bn.beta.g, bn.coef, o.dx, st); };
        ops.push_back(op);
        return true;
    }
    op.fwd = [=](hipStream_t st, int training) -> int {
        if (training && !stats_nb) CDRL_TRY(colstats(x, G, Mg, C, sc->part, st, at));
        if ((training || !bn.batched_inf) && !((g_diag_skip_fin & 4) && stats_nb && ++*diag_calls3 > 3))
            CDRL_TRY(bn_finalize(sc->part, stats_nb ? stats_nb : nb, G, Mg, C, bn.gamma.p, bn.beta.p, bn.mm.p, bn.mv.p, bes, training, bn.stats, st));
        if (gap) return bn_act_gap_fwd(x.p, bn.stats, pass.gap_out, G, Mg / pass.gap_rows, pass.gap_rows, C, act, st, at);
        if (pass.fsrc.p) return bn_apply(x, G, Mg, C, bn.stats, act, o.out, o.out_shuffle, st, &pass.fsrc, &pass.fdst, at);
        return bn_apply(x, G, Mg, C, bn.stats, act, o.out, o.out_shuffle, st, nullptr, nullptr, at);
    };
    op.bwd = [=](hipStream_t st) -> int {
        // fused global average pool: the gradient source is the pooled gradient, one row per gap_rows rows of x
        const View dsrc = gap ? make_view(const_cast<float*>(pass.gap_dout), C) : o.dout;
        const int bc = gap ? pass.gap_rows : 0, dsh = o.dout_shuffle;
        if (pass.gsrc.p) CDRL_TRY(bn_bwd_reduce(o.dout, dsh, x, G, Mg, C, bn.stats, act, sc->part, st, nullptr, &pass.gsrc, &pass.gdst, 0, at));
        else if (!o.sums_by_producer) CDRL_TRY(bn_bwd_reduce(dsrc, dsh, x, G, Mg, C, bn.stats, act, sc->part, st, nullptr, nullptr, nullptr, bc, at));
        if (fin_by_conv) return 0;      // sums folded, applied and turned into dgamma / dbeta by the fused conv backward that follows
        CDRL_TRY(bn_bwd_finalize(sc->part, nb, G, Mg, C, bn.stats, bn.gamma.g, bn.beta.g, bn.coef, st));
        if (apply_by_conv) return 0;    // applied by the backward GEMMs of the conv in front on load
        if (o.dx) return bn_bwd_apply(dsrc, dsh, x, G, Mg, C, bn.stats, bn.coef, act, o.dx, sc->part2, st, nullptr, bc, at);
        CDRL_TRY(sched_.next_slot(st));       // tower: dy + db partials go to a rotating scratch slot
        return bn_bwd_apply(dsrc, dsh, x, G, Mg, C, bn.stats, bn.coef, act, dys_[sched_.slot()], part2s_[sched_.slot()], st, nullptr, bc, at);
    };
    ops.push_back(op);
    return false;
}

// One plan per 1x1 conv of the tower: forward kernel, backward form, backward-data GEMM and the partial-row counts its neighbours read.
// The value is a pure function of the conv's views and shapes, cfg_, at_ and the switches; a conv that has no kernel is refused here
// (build_fail), before anything of its unit is emitted.
Learner::ConvPlan Learner::plan_pw(const PwConv& c, bool fused, bool bb, bool bn_in) {
    static const bool x3_env = env_on("CDRL_PW_X3");
    const int G = cfg_.T, Mg = c.rows / G, Cin = c.Cin, Cout = c.Cout;
    // compute mode 1 (configuration 3): every 1x1 convolution of the tower multiplies bf16-rounded operands -- forward,
    // backward-data and filter gradient: the fused kernels in their BF variant, the plain wide ones through gemm_x3's
    // single-plane form, the filter gradients through tn_direct's BF variant
    const bool bfc = cfg_.compute >= 1;
    ConvPlan p;
    p.bn_in = bn_in;
    if (!fused) {
        // plain (unfused) wide convs -- the 464 -> 768 head conv, the 232-wide shortcut conv -- on the bf16 matrix pipe too (gemm_x3.hip)
        const bool g3 = bfc || (x3_env && (Cin >= 128 || Cout > 128));
        if (g3 && gemm_x3_supported(c.in, Cin)) p.fwd = PwGemm::GemmX3;
        if (g3 && Cout % 4 == 0) p.dgrad = PwGemm::GemmX3;
        if (bfc && (p.fwd != PwGemm::GemmX3 || p.dgrad != PwGemm::GemmX3))
            build_fail("bf16-operand mode: 1x1 convolution %s (%d -> %d, fwd 0 bwd 0 bb 0; input ld %d coff %d) has no bf16 kernel",
                       c.name.c_str(), Cin, Cout, c.in.ld, c.in.coff);
        return p;
    }
    // float32 engine, K or N above 128 (stage 2): the forward runs on the one-tile-per-workgroup split-precision kernel (gemm_pw_x3.hip
    // pw_x3_wide_kernel), which writes one statistics row per 32-row tile
    // (measured at M = 12288 and 49152 rows: 16-20 against 26-36 us, ~60 against 80 us; beyond that every 32-row tile would still stream
    //  its own copy of W -- 196 KB per tile and column block -- and the persistent kernel keeps the shape)
    // The engine's measured policy only (row limits, CDRL_PW_X3); whether a kernel can take a shape and a view is the plans' answer.
    auto wide_policy = [&](int64_t max_rows) { return cfg_.compute == 0 && x3_env && (int64_t)G * Mg <= max_rows; };
    const View dz = c.dz.ld ? c.dz : make_view(nullptr, Cout);
    const PwX3Plan xf = pw_x3_plan(c.in, make_view(c.y, Cout), G, Mg, Cout, Cin, bn_in, true, true);
    const bool wide = wide_policy(49152) && xf.form == 1 && xf.refusal != PWX3_REFUSE_SHAPE;
    // backward-data of the same convs (N = conv input channels, K = conv output channels): pw_x3_wide_bwd_kernel, one part2 / part row per tile
    // Small products only (M = 12288 rows at B = 256: the 3x4-pixel maps of stage 2): every workgroup streams its block of W^T once, so at
    // M = 49152 (the stride-2 unit's first conv, on the 6x8 maps) the fragment traffic (3072 x 196 KB) outweighs what the persistent kernel
    // loses to its serial tiles -- measured in the step: 140 us against 100 us there, 36 against 53 us (BatchNorm-sum epilogue) at M = 12288.
    const PwX3BwdPlan xb = pw_x3_wide_bwd_plan(dz, c.din, G, Mg, Cin, Cout, c.dz_shuffle, false, 0, true);
    const bool wide_bwd = wide_policy(16384) && xb.refusal != PWX3B_REFUSE_SHAPE;
    // forward on the bf16 matrix pipe (exact three-way operand split, gemm_pw_x3.hip) where the shape allows it
    // (dry build: `in.p` is null, which counts as aligned -- as every tens_a tensor is, dense and 256-byte aligned)
    const bool x3f = !bfc && x3_env && (xf.form == 0 || wide) && xf.ok;
    if (wide && !x3f)
        build_fail("%s: the wide split-precision forward needs 16-byte aligned input rows (ld %d, offset %d)", c.name.c_str(), c.in.ld, c.in.coff);
    p.fwd = x3f ? PwGemm::X3 : PwGemm::PwNN;
    p.dgrad = PwGemm::PwNN;
    p.stats_nb = wide ? xf.nbpg : pw_nn_shape_plan(G, Mg, Cout, Cin).nbpg;
    p.bwd_nb = wide_bwd ? xb.rows : pw_nn_shape_plan(G, Mg, Cin, Cout).nbpg;
    if (!bb) return p;
    // Backward form of a unit conv whose BatchNorm-backward apply rides on its operand loads (dz: the gradient w.r.t. the output of the
    // BatchNorm behind the conv, bn_in: the input is a BatchNorm output applied on load)
    // One kernel for backward-data + filter gradient + bias gradient (+ the backward sums of the BatchNorm in front of the conv):
    // float32 engine and bf16 activation storage (not the operand-only mode), both channel counts padded alike (gemm_pw_bwd.hip)
    // 24 input channels -- the first unit, the last conv of the backward -- pad to 64: 158 us against 104 us for the backward-data kernel of
    // the two-kernel form, which is why rounds 4 kept it there; but that form's filter gradient (163 us on the side stream) then bounds the
    // tail of the pass and slows the BatchNorm reduction beside it (117 us instead of 29): fused 14.00 vs 14.06 ms per update-step, and one
    // pass over (dz, y) = 0.3 GB per pass less.
    static constexpr int fbwd_min_cin = 24;
    if (fused_bwd_ && (!bfc || at_) && G <= 8 && Cin >= fbwd_min_cin && pw_bwd_fused_supported(dz, c.in, c.din, Cout, Cin, at_) &&
        (!bn_in || (c.in.ld == Cin && c.in.coff == 0)))
        // float32: the finalize of the BatchNorm behind the conv inside the fused kernel (no bn_bwd_finalize launch in front of it)
        p.bwd = (!at_ && fin_on_load_) ? PwBwd::FusedFin : PwBwd::Fused;
    // 232-channel convs (stage 2), float32: backward-data with the BatchNorm-backward prologue on the one-tile-per-workgroup
    // split-precision kernel (round 6; the filter gradient stays on the side stream)
    else if (!bfc && !at_ && wide_bwd) p.bwd = PwBwd::Wide;
    else p.bwd = PwBwd::Prologue;
    if (p.bwd == PwBwd::Wide && !xb.ok)
        build_fail("%s: the wide split-precision backward needs even / 16-byte aligned gradient rows (ld %d, offset %d, shuffle %d)", c.name.c_str(),
                   dz.ld, dz.coff, c.dz_shuffle);
    return p;
}

// The instantiations the learner's 1x1 convs reach, recorded while the ops are built (cdrl_learner_pw_signatures)
void Learner::note_pw(const char* kind, std::initializer_list<int> fields) {
    std::string r = kind;
    for (int f : fields) r += " " + std::to_string(f);
    pw_sigs_.insert(r);
}
void Learner::note_pw(const PwNnPlan& p) { note_pw("nn", {p.ok, p.ksm, p.nt, p.pro, p.epi, p.mode, p.acc}); }
void Learner::note_pw(const PwX3Plan& p) { note_pw("x3", {p.ok, p.form, p.kp, p.nt, p.pro, p.epi}); }
void Learner::note_pw(const PwX3BwdPlan& p) { note_pw("x3b", {p.ok, p.sh, p.epi, p.acc}); }

void Learner::add_pw(std::vector<Op>& ops, const PwConv& c, const ConvPlan& plan, const BnRec& bn_in, const BnRec& bn_out) {
    PwEmit e{c, plan, bn_in, bn_out};
    const PRef w = e.w = param(M_TRUNK, c.name + ".w", {1, 1, c.Cin, c.Cout}, true);
    const PRef b = e.b = param(M_TRUNK, c.name + ".b", {c.Cout}, true);
    const int G = cfg_.T, rows = c.rows, Mg = rows / G, Cin = c.Cin, Cout = c.Cout, at = at_, nb_fwd = plan.stats_nb;
    Scratch* sc = build_scr_;           // statistics / BatchNorm-sum partials: the scratch of the stream this op's forward runs on (the shortcut
                                        // branch of a stride-2 unit runs beside the main branch and has its own)
    const bool bfc = cfg_.compute >= 1;
    const bool fbwd = pw_fused(plan.bwd), two_kernel = plan.bwd == PwBwd::Plain || plan.bwd == PwBwd::Prologue;
    const float* pro_stats = bn_in.stats;      // (null without a BatchNorm in front)
    const View in = c.in, yv = make_view(c.y, Cout);
    // operands in fragment order, only those the plan's kernels read.  Forward: B(k = cin, n = cout).  Backward, B(k = cout, n = cin): W^T in
    // float32-MFMA fragment order for the persistent kernel, as three bf16 planes for the fused and the wide form (a frozen trunk has no
    // backward and packs nothing)
    const void* w3f = plan.fwd == PwGemm::X3 ? pw_x3_packed(w.p, Cin, Cout, Cout, 1) : nullptr;
    const void* g3f = plan.fwd == PwGemm::GemmX3 ? gemm_x3_packed(w.p, Cin, Cout, Cout, 1) : nullptr;
    if (plan.dgrad == PwGemm::GemmX3 && !frozen()) e.g3b = gemm_x3_packed(w.p, Cout, Cin, 1, Cout);
    const float* wpf = plan.fwd == PwGemm::PwNN ? pw_packed(w.p, Cin, Cout, Cout, 1, bfc) : nullptr;
    if (plan.dgrad == PwGemm::PwNN && two_kernel && !frozen()) e.wpb = pw_packed(w.p, Cout, Cin, 1, Cout, bfc);
    if (!two_kernel && !frozen()) e.wpx = pw_x3_packed(w.p, Cout, Cin, 1, Cout);
    note_scratch(0, 0, (size_t)rows * Cout, (size_t)gemm_tn_part_elems(rows, Cout, Cin, (plan.bn_in || plan.bwd != PwBwd::Plain) ? G : 1));
    if (nb_fwd) note_scratch((size_t)G * nb_fwd * 2 * Cout, 0, 0, 0);
    if (plan.bn_in && !fbwd) note_scratch((size_t)G * plan.bwd_nb * 2 * Cin, 0, 0, 0);     // backward-data epilogue: its sums
    if (plan.bwd != PwBwd::Plain) note_scratch(0, (size_t)G * plan.bwd_nb * Cout, 0, 0);
    if (fbwd) {
        max_qpart_ = std::max(max_qpart_, (size_t)pw_bwd_fused_qpart_elems(G, Mg, Cout, Cin, at));
        max_dbpart_ = std::max(max_dbpart_, (size_t)pw_bwd_fused_dbpart_elems(G, Mg, Cout, Cin, at));
    }
    if (plan.bwd == PwBwd::FusedFin && bn_out.bwd_nb <= 0) build_fail("%s: finalize on load without the BatchNorm's scratch block", c.name.c_str());
    if (plan.fwd == PwGemm::X3) note_pw(pw_x3_plan(in, yv, G, Mg, Cout, Cin, pro_stats != nullptr, true, true, nb_fwd));
    if (plan.fwd == PwGemm::PwNN) note_pw(pw_nn_plan(in, yv, G, Mg, Cout, Cin, pro_stats ? 1 : 0, 1, 0, true, bfc, at, true));
    Op op;
    op.fwd = [=](hipStream_t st, int) -> int {
        switch (plan.fwd) {
            case PwGemm::X3: return pw_x3(in, pro_stats, w3f, b.p, yv, G, Mg, Cout, Cin, sc->part, st, nb_fwd);
            case PwGemm::PwNN:
                return pw_nn(in, pro_stats, w.p, Cout, 1, b.p, yv, 0, G, Mg, Cout, Cin, 1, nullptr, nullptr, sc->part, st, nullptr, wpf, bfc, at);
            case PwGemm::GemmX3: return gemm_x3(in, g3f, b.p, yv, rows, Cout, Cin, 0, st, bfc, at);
            default: return gemm_nn(in, w.p, Cout, 1, b.p, yv, rows, Cout, Cin, 0, st);
        }
    };
    op.bwd = fbwd ? pw_bwd_fused_op(e) : plan.bwd == PwBwd::Plain ? pw_bwd_plain_op(e) : pw_bwd_prologue_op(e);
    ops.push_back(op);
}

// Fused / FusedFin: one kernel for backward-data, filter and bias gradient, then its reduce.  Everything but the scratch slot and the ring
// entry is known when the op is built.
std::function<int(hipStream_t)> Learner::pw_bwd_fused_op(const PwEmit& e) {
    const PwConv& c = e.c;
    const bool fin = e.plan.bwd == PwBwd::FusedFin, on_main = e.plan.bn_in;
    PwBwdFused f0;
    f0.dz = c.dz, f0.dz_shuffle = c.dz_shuffle, f0.act = c.dz_act;
    f0.y = c.y, f0.stats = e.bn_out.stats, f0.coef = e.bn_out.coef;
    f0.a = c.in, f0.a_stats = e.bn_in.stats, f0.a_coef = e.bn_in.coef;
    f0.a_gamma = e.bn_in.gamma.p, f0.a_beta = e.bn_in.beta.p, f0.a_dgamma = e.bn_in.gamma.g, f0.a_dbeta = e.bn_in.beta.g;
    f0.W = e.w.p, f0.Wp = e.wpx, f0.dW = e.w.g, f0.db = e.b.g;
    f0.da = c.din, f0.accumulate = c.din_acc;
    f0.G = cfg_.T, f0.Mg = c.rows / cfg_.T, f0.N = c.Cout, f0.K = c.Cin, f0.at = at_;
    if (fin) f0.fin_nb = e.bn_out.bwd_nb, f0.o_dgamma = e.bn_out.gamma.g, f0.o_dbeta = e.bn_out.beta.g;
    Scratch* o_scr = e.bn_out.scr;
    return [=](hipStream_t st) -> int {
        PwBwdFused f = f0;
        if (f.dz.ld) CDRL_TRY(sched_.next_slot(st));
        else f.dz = make_view(dys_[sched_.slot()], f.N);
        CDRL_TRY(sched_.next_q(st));
        const int qi = sched_.q();
        f.qpart = qparts_[qi];
        f.dbpart = dbparts_[qi];
        if (fin) {
            f.fin_part = o_scr->part;
            f.fin_tot = fintots_[qi];
        }
        CDRL_TRY(pw_bwd_fused(f, st));
        // the reduce also finalizes the BatchNorm in front of the conv (its coefficients are the next kernel's input): critical
        // stream; without one it only produces weight gradients -> side stream, flushed once per unit
        if (on_main) return pw_bwd_fused_reduce(f, st);
        CDRL_TRY(sched_.defer_side(st, [=](hipStream_t sd) -> int {
            CDRL_TRY(pw_bwd_fused_reduce(f, sd));
            return sched_.release_q(qi, sd);
        }));
        return sched_.flush_side(st);
    };
}

// Prologue / Wide: BN-backward apply fused into the operand loads of two kernels, dz (+ raw y, statistics, coefficients) instead of dy;
// filter gradient on the side stream, backward-data on the critical one
std::function<int(hipStream_t)> Learner::pw_bwd_prologue_op(const PwEmit& e) {
    const int G = cfg_.T, rows = e.c.rows, Mg = rows / G, Cin = e.c.Cin, Cout = e.c.Cout, at = at_, din_acc = e.c.din_acc, nb = e.plan.bwd_nb;
    const bool bfc = cfg_.compute >= 1, wide = e.plan.bwd == PwBwd::Wide, bn_in = e.plan.bn_in;
    Scratch* sc = build_scr_;
    const View in = e.c.in, din = e.c.din, dz0 = e.c.dz;
    const float *pro_stats = e.bn_in.stats, *bwd_ey = e.bn_in.x.p;      // (null without a BatchNorm in front)
    const TnBnBwd tb{e.c.y, e.bn_out.stats, e.bn_out.coef, e.c.dz_shuffle, e.c.dz_act};
    const PRef w = e.w, b = e.b;
    const float* wpb = e.wpb;
    const void* wpx = e.wpx;
    const View dzb = dz0.ld ? dz0 : make_view(nullptr, Cout);       // (the scratch slots are dense and 256-byte aligned)
    if (wide) note_pw(pw_x3_wide_bwd_plan(dzb, din, G, Mg, Cin, Cout, tb.shuffle_ctot, bn_in, din_acc, true));
    else note_pw(pw_nn_plan(dzb, din, G, Mg, Cin, Cout, 2, bn_in ? 2 : 0, din_acc, true, bfc, at, true, tb.y));
    return [=](hipStream_t st) -> int {
        if (dz0.ld) CDRL_TRY(sched_.next_slot(st));
        const View dz = dz0.ld ? dz0 : make_view(dys_[sched_.slot()], Cout);
        hipStream_t side = sched_.fork_side(st);
        CDRL_TRY(gemm_tn(in, dz, w.g, rows, Cout, Cin, tns_[sched_.slot()], 0, side, G, pro_stats, &tb, bfc, at));
        CDRL_TRY(sched_.done_side(side));
        PwBnBwd pb{tb.y, tb.stats, tb.coef, tb.shuffle_ctot, tb.act, part2s_[sched_.slot()]};
        if (wide)
            CDRL_TRY(pw_x3_wide_bwd(dz, pb, wpx, din, din_acc, G, Mg, Cin, Cout, bwd_ey, pro_stats, bn_in ? sc->part : nullptr, st));
        else
            CDRL_TRY(pw_nn(dz, nullptr, w.p, 1, Cout, nullptr, din, din_acc, G, Mg, Cin, Cout, bn_in ? 2 : 0, bwd_ey, pro_stats, sc->part, st, &pb,
                           wpb, bfc, at));
        // bias gradient = column sums of the (virtual) dy, reduced from the GEMM's partials: rides on the next fork
        double* p2 = part2s_[sched_.slot()];
        return sched_.defer_side(st, [=](hipStream_t sd) -> int { return reduce_partials(p2, G * nb, Cout, Cout, b.g, 0, sd); });
    };
}

// Plain: dy is in the current scratch slot (left there by the BatchNorm behind the conv, with its column sums per block)
std::function<int(hipStream_t)> Learner::pw_bwd_plain_op(const PwEmit& e) {
    const int G = cfg_.T, rows = e.c.rows, Mg = rows / G, Cin = e.c.Cin, Cout = e.c.Cout, at = at_, din_acc = e.c.din_acc;
    const int o_rows = e.bn_out.G * e.bn_out.nb, tn_groups = e.plan.bn_in ? G : 1, epi = e.plan.bn_in ? 2 : 0;
    const bool bfc = cfg_.compute >= 1;
    const PwGemm dgrad = e.plan.dgrad;
    Scratch* sc = build_scr_;
    const View in = e.c.in, din = e.c.din;
    const float *pro_stats = e.bn_in.stats, *bwd_ey = e.bn_in.x.p;      // (null without a BatchNorm in front)
    const PRef w = e.w, b = e.b;
    const float* wpb = e.wpb;
    const void* g3b = e.g3b;
    if (din.ld && dgrad == PwGemm::PwNN) note_pw(pw_nn_plan(make_view(nullptr, Cout), din, G, Mg, Cin, Cout, 0, epi, din_acc, true, bfc, at, true));
    return [=](hipStream_t st) -> int {
        const View dy = make_view(dys_[sched_.slot()], Cout);
        // side stream: bias gradient (column sums of dy, reduced per block by bn_bwd_apply) + filter gradient
        hipStream_t side = sched_.fork_side(st);
        CDRL_TRY(reduce_partials(part2s_[sched_.slot()], o_rows, Cout, Cout, b.g, 0, side));
        CDRL_TRY(gemm_tn(in, dy, w.g, rows, Cout, Cin, tns_[sched_.slot()], 0, side, tn_groups, pro_stats, nullptr, bfc, at));
        CDRL_TRY(sched_.done_side(side));
        // main stream: the critical path to the previous layer
        if (!din.p) return 0;
        if (dgrad == PwGemm::PwNN)
            return pw_nn(dy, nullptr, w.p, 1, Cout, nullptr, din, din_acc, G, Mg, Cin, Cout, epi, bwd_ey, pro_stats, sc->part, st, nullptr, wpb, bfc, at);
        if (dgrad == PwGemm::GemmX3) return gemm_x3(dy, g3b, nullptr, din, rows, Cin, Cout, din_acc, st, bfc, at);
        return gemm_nn(dy, w.p, 1, Cout, nullptr, din, rows, Cin, Cout, din_acc, st);
    };
}

void Learner::add_dw(std::vector<Op>& ops, const std::string& prefix, View in, int N, int H, int W, int C, int stride,
                     float* y, View din, int din_acc, const BnRec* pre_bn) {
    PRef w = param(M_TRUNK, prefix + ".w", {3, 3, C, 1}, true);
    PRef b = param(M_TRUNK, prefix + ".b", {C}, true);
    const int Ho = same_out_h(H, stride), Wo = same_out_h(W, stride);
    note_scratch(0, 0, (size_t)N * Ho * Wo * C, 0, (size_t)dw_bwd_part_elems(N, H, W, C, stride));
    const bool fuse = pre_bn != nullptr;
    if (fuse && (din_acc != 0 || pre_bn->C != C || pre_bn->Mg * pre_bn->G != N * H * W || pre_bn->x.ld != C || pre_bn->x.coff != 0))
        build_fail("%s: the BatchNorm in front does not cover the depthwise input", prefix.c_str());
    const int pre_G = fuse ? pre_bn->G : 0, pre_act = fuse ? pre_bn->act : 0;
    const float *pre_y = fuse ? pre_bn->x.p : nullptr, *pre_stats = fuse ? pre_bn->stats : nullptr;
    if (at_) build_fail("%s: the unfused depthwise path has no bf16-storage form (CDRL_FUSED_DW=0 is set)", prefix.c_str());
    Op op;
    op.fwd = [=](hipStream_t st, int) -> int { return dw_fwd(in, w.p, b.p, y, N, H, W, C, stride, st); };
    op.bwd = [=](hipStream_t st) -> int {
        float* dy = dys_[sched_.slot()];
        hipStream_t side = sched_.fork_side(st);
        CDRL_TRY(dw_bwd_filter(in, dy, w.g, b.g, N, H, W, C, stride, fparts_[sched_.slot()], side));
        CDRL_TRY(sched_.done_side(side));
        if (fuse)      // bwd-data + BN-backward sums of the layer that produced `in` in one pass over da
            return dw_bwd_data_bnreduce(dy, w.p, din, N, H, W, C, stride, pre_G, pre_y, pre_stats, pre_act, scr_main_.part, st);
        return dw_bwd_data(dy, w.p, din, N, H, W, C, stride, din_acc, st);
    };
    ops.push_back(op);
}

Learner::BnRec Learner::add_dw_block(std::vector<Op>& ops, const DwBlock& d) {
    const int B = cfg_.B, G = cfg_.T, N = B * G;
    const int H = d.H, W = d.W, C = d.C, stride = d.stride;
    const int Ho = same_out_h(H, stride), Wo = same_out_h(W, stride);
    const int Mi = B * H * W, Mo = B * Ho * Wo;
    const bool pre = (bool)d.pre;
    Scratch* sc = build_scr_;           // the shortcut branch of a stride-2 unit has its own partial buffers (it runs on the side stream)
    float *x = d.x, *y2 = d.y2;
    PRef w = param(M_TRUNK, d.dw + ".w", {3, 3, C, 1}, true);
    PRef b = param(M_TRUNK, d.dw + ".b", {C}, true);
    const BnRec post = make_bn(M_TRUNK, d.bn_post, make_view(y2, C), G, Mo, C, ACT_NONE);
    const View out = d.out, dout = d.dout, din = d.din;
    const int pre_stats_nb = d.pre_conv.stats_nb, post_bwd_nb = d.post_conv.bwd_nb;
    const bool pre_apply_by_conv = d.pre_conv.bwd != PwBwd::Plain, pre_fin_by_conv = d.pre_conv.bwd == PwBwd::FusedFin;
    const bool post_on_load = d.post_conv.bn_in, post_bwd_by_conv = pw_fused(d.post_conv.bwd);
    const int nb_in = vcol_geom(Mi, C).nb, nb_out = post.nb;
    const DwfPlan dp = dwf_plan(B, G, H, W, C, stride, pre ? C : din.ld);      // (dx: a scratch slot behind BN1, the caller's view otherwise)
    const int nbf = dp.nb;              // partial rows of the forward kernel (BN2 statistics) ...
    const int nbb = dp.nb_bwd;          // ... and of the backward (BN1 sums, filter partials)
    const size_t nbmax = (size_t)std::max(std::max(std::max(nb_in, nb_out), std::max(nbf, nbb)), std::max(pre_stats_nb, post_bwd_nb));
    note_scratch((size_t)G * nbmax * 2 * C, (size_t)G * nbmax * C, (size_t)N * H * W * C, 0, (size_t)dp.filter_part_elems);
    const View xv = make_view(x, C), y2v = make_view(y2, C);
    const int at = at_;
    std::shared_ptr<int> diag_calls = std::make_shared<int>(0);

    if (pre) {      // BN1: statistics only in the forward; backward = finalize of the sums the depthwise op produced
        Op op;
        op.fwd = [=](hipStream_t st, int training) -> int {
            if (!training) return 0;                            // inference: statistics block from the batched launch
            if (!pre_stats_nb) CDRL_TRY(colstats(xv, G, Mi, C, sc->part, st, at));
            if ((g_diag_skip_fin & 1) && ++*diag_calls > 6) return 0;      // timing diagnostic: stale statistics of an earlier step
            return bn_finalize(sc->part, pre_stats_nb ? pre_stats_nb : nb_in, G, Mi, C, d.pre.gamma.p, d.pre.beta.p, d.pre.mm.p, d.pre.mv.p, 1, training, d.pre.stats, st);
        };
        op.bwd = [=](hipStream_t st) -> int {
            if (pre_fin_by_conv) return 0;                 // folded by the fused backward of the 1x1 conv in front (finalize on load)
            CDRL_TRY(bn_bwd_finalize(sc->part, nbb, G, Mi, C, d.pre.stats, d.pre.gamma.g, d.pre.beta.g, d.pre.coef, st));
            if (pre_apply_by_conv) return 0;               // the 1x1 conv in front applies it on load
            const float* dz = dys_[sched_.slot()];                 // masked gradient left there by the depthwise op
            CDRL_TRY(sched_.next_slot(st));
            return bn_bwd_apply(make_view(const_cast<float*>(dz), C), 0, xv, G, Mi, C, d.pre.stats, d.pre.coef, ACT_NONE, dys_[sched_.slot()],
                                part2s_[sched_.slot()], st, nullptr, 0, at);
        };
        ops.push_back(op);
    }
    {
        Op op;
        op.fwd = [=](hipStream_t st, int) -> int {
            return dwf_fwd(dp, DwfFwdArgs{x, d.pre.stats, w.p, b.p, y2, sc->part, st, at});
        };
        op.bwd = [=](hipStream_t st) -> int {
            CDRL_TRY(sched_.next_slot(st));
            double* pw = fparts_[sched_.slot()];
            const View dx = pre ? make_view(dys_[sched_.slot()], C) : din;
            CDRL_TRY(dwf_bwd(dp, DwfBwdArgs{x, d.pre.stats, dout.p, y2, post.stats, post.coef, w.p, dx, sc->part, pw, st, at}));
            return sched_.defer_side(st, [=](hipStream_t sd) -> int {
                return reduce_partials2(pw, G * nbb, 9 * C, C, (int64_t)10 * C, w.g, b.g, 0, sd);
            });
        };
        ops.push_back(op);
    }
    {               // BN2: finalize + apply in the forward; backward = sums + coefficients only (applied by the dw op)
        Op op;
        op.fwd = [=](hipStream_t st, int training) -> int {
            if (training && !((g_diag_skip_fin & 2) && ++*diag_calls > 6))
                CDRL_TRY(bn_finalize(sc->part, nbf, G, Mo, C, post.gamma.p, post.beta.p, post.mm.p, post.mv.p, 1, training, post.stats, st));
            if (post_on_load) return 0;
            return bn_apply(y2v, G, Mo, C, post.stats, ACT_NONE, out, 0, st, nullptr, nullptr, at);
        };
        op.bwd = [=](hipStream_t st) -> int {
            if (post_bwd_by_conv) return 0;     // dgamma, dbeta, coefficients come out of the consumer conv's reduce kernel
            if (!post_bwd_nb) CDRL_TRY(bn_bwd_reduce(dout, 0, y2v, G, Mo, C, post.stats, ACT_NONE, sc->part, st, nullptr, nullptr, nullptr, 0, at));
            return bn_bwd_finalize(sc->part, post_bwd_nb ? post_bwd_nb : nb_out, G, Mo, C, post.stats, post.gamma.g, post.beta.g, post.coef, st);
        };
        ops.push_back(op);
    }
    return post;
}

void Learner::add_half(std::vector<Op>& ops, const Half& h) {
    const int B = cfg_.B, T = cfg_.T, N = B * T;
    DwBlock d = h.d;
    const int Ho = same_out_h(d.H, d.stride), Wo = same_out_h(d.W, d.stride);
    const int rows_in = N * d.H * d.W, rows_out = N * Ho * Wo, Mg_out = B * Ho * Wo;
    const int Cm = d.C, Co = h.Cout, Ct = h.out.C;
    const std::string dw = h.unit + "." + h.dw, bn_mid = h.unit + "." + h.bn_mid, pw = h.unit + "." + h.pw, bn_out = h.unit + "." + h.bn_out;
    Tens y2 = tens_a(rows_out, Cm, false), a2 = tens_a(rows_out, Cm), y3 = tens_a(rows_out, Co, false);
    BnOp o3;
    o3.out = h.out.v(h.out_off);
    o3.dout = h.out.gv(h.out_off);
    o3.out_shuffle = o3.dout_shuffle = Ct;
    o3.pass = h.pass;
    d.dw = dw;
    d.bn_post = bn_mid;
    d.y2 = y2.p;
    d.out = a2.v();
    d.dout = a2.gv();
    if (h.fused) {
        // BN-apply of the middle BatchNorm on the conv's operand load (its output is never written), statistics of the last one in
        // the conv's epilogue; backward: the BatchNorm-backward of the last one as the conv's operand prologue (gathered through the
        // shuffle map), the middle one's backward sums out of the conv backward -- the fused form's reduce kernel, else the
        // backward-data epilogue
        const PwConv conv{pw, y2.v(), rows_out, Cm, Co, y3.p, a2.gv(), 0, o3.dout, Ct, ACT_RELU6};
        const ConvPlan plan = plan_pw(conv, true, h.bb, true);
        d.post_conv = plan;
        const BnRec mid = add_dw_block(ops, d);
        const BnRec last = pw_bn(pw, Cm, Co, bn_out, y3.p, Mg_out, ACT_RELU6);
        add_pw(ops, conv, plan, mid, last);
        o3.conv = plan;
        add_bn(ops, last, o3);
        return;
    }
    if (fused_dw_) {
        add_dw_block(ops, d);
    } else {
        if (d.pre) {
            Tens a1 = tens_a(rows_in, Cm);
            BnOp o1;
            o1.out = a1.v();
            o1.dout = a1.gv();
            o1.sums_by_producer = true;     // the depthwise backward-data kernel leaves them
            add_bn(ops, d.pre, o1);
            add_dw(ops, dw, a1.v(), N, d.H, d.W, Cm, d.stride, y2.p, a1.gv(), 0, &d.pre);
        } else {
            add_dw(ops, dw, make_view(d.x, Cm), N, d.H, d.W, Cm, d.stride, y2.p, d.din, 0);
        }
        BnOp o2;
        o2.out = a2.v();
        o2.dout = a2.gv();
        add_bn(ops, make_bn(M_TRUNK, bn_mid, y2.v(), T, Mg_out, Cm, ACT_NONE), o2);
    }
    const BnRec last = pw_bn(pw, Cm, Co, bn_out, y3.p, Mg_out, ACT_RELU6);
    const PwConv conv{pw, a2.v(), rows_out, Cm, Co, y3.p, a2.gv()};
    add_pw(ops, conv, plan_pw(conv, false, false, false), BnRec(), last);
    add_bn(ops, last, o3);
}

void Learner::add_dense(std::vector<Op>& ops, int model, const std::string& prefix, View in, int M, int K, int N,
                        int act, View out, View dout, View din, int din_acc, bool need_din, const char*) {
    PRef w = param(model, prefix + ".w", {K, N}, true);
    PRef b = param(model, prefix + ".b", {N}, true);
    float *z = nullptr, *dz = nullptr;
    if (act != ACT_NONE) {
        z = alloc((size_t)M * N);
        dz = alloc((size_t)M * N);
        note_named(prefix + ".z", z, (size_t)M * N * sizeof(float));
    }
    note_scratch((size_t)vcol_geom(M, N).nb * N, (size_t)vcol_geom(M, N).nb * N, 0, (size_t)gemm_tn_part_elems(M, N, K));
    const int nb = vcol_geom(M, N).nb;
    Scratch* sc = build_scr_;
    const size_t dskn = (size_t)std::max(gemm_nn_splitk_elems(M, N, K), gemm_nn_splitk_elems(M, K, N));
    float* dsk = dskn ? alloc(dskn) : nullptr;          // split-K scratch (batch-sized M, K >= 256)
    Op op;
    op.fwd = [=](hipStream_t st, int) -> int {
        if (act == ACT_NONE) return gemm_nn(in, w.p, N, 1, b.p, out, M, N, K, 0, st, dsk);
        bool act_done = false;      // (split-K layers: the activation rides in the slab reduce)
        const bool dense_out = out.ld == N && out.coff == 0;
        CDRL_TRY(gemm_nn(in, w.p, N, 1, b.p, make_view(z, N), M, N, K, 0, st, dsk, dense_out ? out.p : nullptr, act, &act_done));
        if (act_done) return 0;
        return act_fwd(z, out.p, (int64_t)M * N, act, st);
    };
    op.bwd = [=](hipStream_t st) -> int {
        View dzv = dout;
        if (act != ACT_NONE) {
            CDRL_TRY(act_bwd(z, dout.p, dz, (int64_t)M * N, act, st));
            dzv = make_view(dz, N);
        }
        // critical path first, then the weight / bias gradients on the side stream (main-stream layers only)
        if (need_din) CDRL_TRY(gemm_nn(dzv, w.p, 1, N, nullptr, din, M, K, N, din_acc, st, dsk));
        if (sc == &scr_main_) {
            CDRL_TRY(sched_.next_slot(st));
            hipStream_t side = sched_.fork_side(st);
            CDRL_TRY(colsum(dzv, M, N, part2s_[sched_.slot()], side));
            CDRL_TRY(reduce_partials(part2s_[sched_.slot()], nb, N, N, b.g, 0, side));
            CDRL_TRY(gemm_tn(in, dzv, w.g, M, N, K, tns_[sched_.slot()], 0, side));
            return sched_.done_side(side);
        }
        CDRL_TRY(colsum(dzv, M, N, sc->part, st));
        CDRL_TRY(reduce_partials(sc->part, nb, N, N, b.g, 0, st));
        return gemm_tn(in, dzv, w.g, M, N, K, sc->tn, 0, st);
    };
    ops.push_back(op);
}

void Learner::add_gru(std::vector<Op>& ops, const std::string& name, Tens& x, int In, int u, View out, View dout,
                      bool need_dx) {
    const int B = cfg_.B, T = cfg_.T, U3 = 3 * u;
    PRef Kp = param(M_TRUNK, name + ".kernel", {In, U3}, true);
    PRef Rp = param(M_TRUNK, name + ".recurrent", {u, U3}, true);
    PRef bp = param(M_TRUNK, name + ".bias", {2, U3}, true);
    float* XP = alloc((size_t)T * B * U3);
    float* HP = alloc((size_t)T * B * U3);
    float* Z = alloc((size_t)T * B * u);
    float* R = alloc((size_t)T * B * u);
    float* HH = alloc((size_t)T * B * u);
    float* Hs = alloc((size_t)(T + 1) * B * u);         // Hs[0] = h_{-1} = 0: zeroed once at bind, never written
    float* dXP = alloc((size_t)T * B * U3);
    float* dHP = alloc((size_t)T * B * U3);
    float* dHa = alloc((size_t)B * u);
    float* dHb = alloc((size_t)B * u);
    if (!dry_) zero_once_.push_back(std::make_pair(Hs, (size_t)B * u * sizeof(float)));
    if (!gru_step_supported(u)) build_fail("GRU units %d unsupported by the fused step kernels", u);
    const float* RT = frozen() ? nullptr : pw_transposed(name + ".recurrent", Rp.p, u, U3);        // [3u][u], refreshed by the pack launch
    note_scratch((size_t)vcol_geom(T * B, U3).nb * U3, (size_t)vcol_geom(T * B, U3).nb * U3, 0,
                 (size_t)std::max(gemm_tn_part_elems(T * B, U3, In), gemm_tn_part_elems(T * B, U3, u)));
    const int nbc = vcol_geom(T * B, U3).nb;
    View xv = x.v();
    View xg = x.gv();
    Scratch* sc = build_scr_;
    // split-K scratch for the input projections (M = T*B, K = In / 3u): own buffer per GRU, the GRUs of different
    // modalities run on different streams
    size_t skn = 0;
    for (int64_t e : {gemm_nn_splitk_elems(T * B, U3, In), gemm_nn_splitk_elems(T * B, In, U3)}) skn = std::max(skn, (size_t)e);
    float* sk = skn ? alloc(skn) : nullptr;
    Op op;
    op.fwd = [=](hipStream_t st, int) -> int {
        CDRL_TRY(gemm_nn(xv, Kp.p, U3, 1, bp.p, make_view(XP, U3), T * B, U3, In, 0, st, sk));
        for (int t = 0; t < T; ++t)         // one fused kernel per step: h R + b1, gates, saved tensors, (last step) the concat slot
            CDRL_TRY(gru_step_fwd(XP + (size_t)t * B * U3, Hs + (size_t)t * B * u, Rp.p, bp.p + U3, Z + (size_t)t * B * u,
                                  R + (size_t)t * B * u, HH + (size_t)t * B * u, HP + (size_t)t * B * U3,
                                  Hs + (size_t)(t + 1) * B * u, t == T - 1 ? out : View{nullptr, 0, 0}, B, u, st));
        return 0;
    };
    op.bwd = [=](hipStream_t st) -> int {
        View cur = dout;                    // the gradient enters through the last hidden state only
        float* nxt = dHa;
        for (int t = T - 1; t >= 0; --t) {
            CDRL_TRY(gru_step_bwd(cur, Z + (size_t)t * B * u, R + (size_t)t * B * u, HH + (size_t)t * B * u,
                                  HP + (size_t)t * B * U3, Hs + (size_t)t * B * u, RT, dXP + (size_t)t * B * U3,
                                  dHP + (size_t)t * B * U3, t > 0 ? nxt : nullptr, B, u, st));
            cur = make_view(nxt, u);
            nxt = nxt == dHa ? dHb : dHa;
        }
        // critical path first: the gradient w.r.t. the GRU input
        if (need_dx) CDRL_TRY(gemm_nn(make_view(dXP, U3), Kp.p, 1, U3, nullptr, xg, T * B, In, U3, 0, st, sk));
        // weight / bias gradients: off the critical path -> side stream with a rotating scratch slot (main-stream GRU only;
        // the small-modality GRUs already run on the aux stream with their own scratch)
        hipStream_t ws = st;
        float* tn = sc->tn;
        double* part = sc->part;
        const bool on_side = sc == &scr_main_;
        if (on_side) {
            CDRL_TRY(sched_.next_slot(st));
            ws = sched_.fork_side(st);
            tn = tns_[sched_.slot()];
            part = part2s_[sched_.slot()];
        }
        CDRL_TRY(gemm_tn(xv, make_view(dXP, U3), Kp.g, T * B, U3, In, tn, 0, ws));
        CDRL_TRY(colsum(make_view(dXP, U3), T * B, U3, part, ws));
        CDRL_TRY(reduce_partials(part, nbc, U3, U3, bp.g, 0, ws));
        CDRL_TRY(gemm_tn(make_view(Hs, u), make_view(dHP, U3), Rp.g, T * B, U3, u, tn, 0, ws));
        CDRL_TRY(colsum(make_view(dHP, U3), T * B, U3, part, ws));
        CDRL_TRY(reduce_partials(part, nbc, U3, U3, bp.g + U3, 0, ws));
        if (on_side) CDRL_TRY(sched_.done_side(ws));
        return 0;
    };
    ops.push_back(op);
}

// The road / vehicle / navigation feature nets and their GRUs are ~150 latency-bound launches that
// do not depend on the image tower: they are enqueued on the side stream at the start of the forward
// (fork) and joined right before the concat BatchNorm; in the backward they are forked as soon as the
// gradient of the concat exists and run under the tower's backward.
void Learner::add_aux_fork(std::vector<Op>& ops) {
    Op op;
    op.fwd = [=](hipStream_t st, int training) -> int {
        if (g_diag_skip_aux & 1) return 0;
        if (!sched_.side_on()) return run_fwd(aux_ops_, st, training);
        CDRL_TRY(sched_.fork_aux(st));        // parameters / inputs produced on the main stream
        CDRL_TRY(run_fwd(aux_ops_, sched_.aux(), training));
        return sched_.done_aux();
    };
    op.bwd = [](hipStream_t) -> int { return 0; };
    ops.push_back(op);
}

void Learner::add_aux_join(std::vector<Op>& ops) {
    Op op;
    op.fwd = [=](hipStream_t st, int) -> int {
        return sched_.join_aux(st);
    };
    op.bwd = [=](hipStream_t st) -> int {
        if (g_diag_skip_aux & 2) return 0;
        if (!sched_.side_on()) return run_bwd(aux_ops_, st);
        // the aux stream, not the side stream; joined by join_side() at the end of the backward
        CDRL_TRY(sched_.fork_aux(st));        // gradient of the concat is ready
        CDRL_TRY(run_bwd(aux_ops_, sched_.aux()));
        return sched_.done_aux();
    };
    ops.push_back(op);
}

// ------------------------------------------------------------------------------------------
// graph construction
// ------------------------------------------------------------------------------------------
void Learner::build_trunk(std::vector<Op>& ops) {
    const Config& c = cfg_;
    const int B = c.B, T = c.T, N = B * T;
    const int Hs = (c.H - 3) / 2 + 1, Ws = (c.W - 3) / 2 + 1;
    aux_ops_.clear();
    add_aux_fork(ops);
    {
        fused_dw_ = env_on("CDRL_FUSED_DW");        // 0 -> unfused bn-apply / depthwise / stats kernels
        fused_pw_ = env_on("CDRL_FUSED_PW");        // 0 -> generic tiled GEMM + separate BN passes around the 1x1 convs
        // BN-backward apply as GEMM operand prologue, for both 1x1 convs of a unit (bn1; bn3, gathered through the shuffle map) and the
        // shortcut conv of the stride-2 units; 0 -> separate apply passes with a materialised dy
        // measured at v19 (bit mask: 1 = bn1, 2 = bn3): 1 -> 25.5, 0 -> 25.8, 3 -> 26.0, 2 -> 26.2 ms/update-step; re-measured at v29
        // (buffer-load filter gradient: the shuffle gather costs nothing there any more): 3 -> 20.66, 1 -> 20.80, 0 -> 21.0, 2 -> 21.3, and
        // with the wide fused pointwise path 3 -> 20.21.  The first unit's conv with 24 input channels takes it too -- slower before the
        // accumulate variant prefetched its old output tile (248 us against 165 us for apply + plain GEMM), now 15.91 vs 15.96
        // ms/update-step and one 164 MB tensor less
        fused_bb_ = env_on("CDRL_FUSED_BB");
        // (round 4's LDS-resident 64-row panel form of the 232-channel forward convs, gemm_pw_wide.hip, is gone: 18 vs 26 us per launch
        //  isolated but 14.43 vs 14.48 ms per update-step, and -- like any change of a float32 forward -- it re-drew the ReLU6 decisions
        //  and moved smoke()'s worst tensor from 6.9e-5 to 9.5e-5 of the 1e-4 gate, both times it was measured: DESIGN.md section 3)
        // The fused conv backward folds the backward sums of the BatchNorm behind it in its own prologue (no bn_bwd_finalize launch in
        // front: 46 fewer critical-stream launches per update-step, 614 -> 568; losses bit-identical over 155 update-steps).  Round 4
        // measured it neutral (-0.07 ms) with 128-256 partial rows per time slice -- every one of the 64 workgroups of a slice reads all
        // of them from L2 -- and kept it opt-in; with 64 rows from the strip-form depthwise backward and 128 from the BatchNorm reductions
        // (NB_STATS) it is worth 0.16 ms per update-step (14.15 vs 14.31 ms, same box) and is the default.  CDRL_FIN_ON_LOAD=0 -> stand-alone
        // finalize launches.
        fin_on_load_ = env_on("CDRL_FIN_ON_LOAD");
        const char* e4 = cdrl_getenv("CDRL_FUSED_BWD");     // 0 -> backward-data (critical stream) + filter gradient (side stream) as two kernels
        fused_bwd_ = env_on("CDRL_FUSED_BWD");
        // bf16 storage: its two-kernel form is cheap already (one plane, half the bytes); fused-on vs fused-off measured
        // 12.41 vs 12.20 ms per update-step at B = 256, 18.67 vs 18.74 at B = 512, 31.38 vs 32.62 at B = 1024 -> from B = 512
        if (at_ && !(e4 && atoi(e4) == 1) && B < 512) fused_bwd_ = false;
    }

    // ---- stem (core/architectures.py:159-161)
    {
        const int at = at_;
        Tens y = tens_a(N * Hs * Ws, c.stem, false);
        PRef w = param(M_TRUNK, "img.stem.conv.w", {3, 3, 3, c.stem}, true);
        PRef b = param(M_TRUNK, "img.stem.conv.b", {c.stem}, true);
        note_scratch(0, 0, (size_t)N * Hs * Ws * c.stem, 0, (size_t)stem_bwd_part_elems(B, T, c.H, c.W, c.stem));
        Op op;
        const int H = c.H, W = c.W, Cs = c.stem;
        // forward: BN statistics in the conv's epilogue (training only; inference uses the moving statistics)
        const bool stem_fstats = stem_fwd_stats_supported(Cs) && env_on("CDRL_FUSED_STEM");
        const int nb_stem = stem_fstats ? stem_fwd_stats_nb(B, T, H, W, Cs) : 0;
        if (at && !stem_fstats) build_fail("bf16 activation storage needs the fused stem forward (stem channels %d, CDRL_FUSED_STEM)", Cs);
        op.fwd = [=](hipStream_t st, int training) -> int {
            // (bf16 storage: the statistics form is the one with a bf16 store; its partials are simply unused in inference)
            if (stem_fstats && (training || at)) return stem_fwd_stats(in_image_, w.p, b.p, y.p, scr_main_.part, B, T, H, W, Cs, st, at);
            return stem_fwd(in_image_, w.p, b.p, y.p, B, T, H, W, Cs, st);
        };
        const bool stem_fused = stem_bwd_fused_supported(Cs) && env_on("CDRL_FUSED_STEM");
        // the stem BatchNorm (made here: the stem conv's backward consumes its blocks in the fused form)
        const BnRec sbn = make_bn(M_TRUNK, "img.stem.bn", y.v(), T, B * Hs * Ws, Cs, ACT_RELU6);
        float *stem_stats = sbn.stats, *stem_coef = sbn.coef;
        const int Hp0 = same_out_h(Hs, 2), Wp0 = same_out_h(Ws, 2);
        Tens pool = tens_a(N * Hp0 * Wp0, c.stem);
        if (at && !stem_fused) build_fail("bf16 activation storage needs the fused stem backward (stem channels %d, CDRL_FUSED_STEM)", Cs);
        uint8_t* argmax = reinterpret_cast<uint8_t*>(alloc(((size_t)N * Hp0 * Wp0 * c.stem + 3) / 4));
        note_named("img.stem.pool.argmax", argmax, (size_t)N * Hp0 * Wp0 * Cs);
        note_named("img.stem.pool.out", pool.p, (size_t)N * Hp0 * Wp0 * Cs * esz());
        note_named("img.stem.pool.out.g", pool.g, (size_t)N * Hp0 * Wp0 * Cs * esz());
        op.bwd = [=](hipStream_t st) -> int {
            if (stem_fused) {
                CDRL_TRY(sched_.next_slot(st));
                // the last kernel of the backward, on the critical stream: nothing is left there to run beside it, so a hand-over to the
                // side stream and back would only cost its two event bubbles (rounds 1-4 ran it on the side stream)
                PoolSrc ps = make_pool_src(argmax, pool.g, Hs, Ws);
                static const bool diag_skip = cdrl_getenv("CDRL_DIAG_SKIP_STEMF") && atoi(cdrl_getenv("CDRL_DIAG_SKIP_STEMF")) == 1;    // timing diagnostics only (no stem filter gradient)
                if (!diag_skip)
                    CDRL_TRY(stem_bwd_filter_fused(in_image_, ps, y.p, stem_stats, stem_coef, w.g, b.g, B, T, H, W, Cs, fparts_[sched_.slot()], st, at));
                return 0;
            }
            hipStream_t side = sched_.fork_side(st);
            CDRL_TRY(stem_bwd_filter(in_image_, dys_[sched_.slot()], w.g, b.g, B, T, H, W, Cs, fparts_[sched_.slot()], side));
            return sched_.done_side(side);
        };
        ops.push_back(op);
        // stem BN + ReLU6 + max-pool as one fused block: the BN op only produces statistics in the forward
        // (no apply), the pool kernel applies scale/shift/ReLU6 on the raw conv output while pooling, and the
        // BN backward gathers its incoming gradient straight from the pooled gradient through the argmax.
        const int Hp = Hp0, Wp = Wp0;
        {
            const int G = sbn.G, Mg = sbn.Mg, C = sbn.C, nb = sbn.nb;
            const PRef gamma = sbn.gamma, beta = sbn.beta, mm = sbn.mm, mv = sbn.mv;
            float *stats = sbn.stats, *coef = sbn.coef;
            const int nb_pool = vcol_geom(B * Hp * Wp, C).nb;
            note_scratch((size_t)G * std::max(std::max(nb, nb_pool), nb_stem) * 2 * C, (size_t)G * nb * C, 0, 0);
            View yv = y.v();
            Op bn;
            bn.fwd = [=](hipStream_t st, int training) -> int {
                if (training && !stem_fstats) CDRL_TRY(colstats(yv, G, Mg, C, scr_main_.part, st));
                if (training)       // (inference: statistics block from the batched launch)
                    CDRL_TRY(bn_finalize(scr_main_.part, stem_fstats ? nb_stem : nb, G, Mg, C, gamma.p, beta.p, mm.p, mv.p, 1, training, stats,
                                         st));
                return maxpool_bn_fwd(y.p, stats, G, B, pool.p, argmax, N, Hs, Ws, C, st, at);
            };
            bn.bwd = [=](hipStream_t st) -> int {
                PoolSrc ps = make_pool_src(argmax, pool.g, Hs, Ws);
                View none{nullptr, 0, 0};
                if (stem_fused) {       // sums in scatter form over the pooled gradient; the apply happens inside the stem filter-gradient GEMM
                    ps.pa = pool.p;                 // mask and xhat from the pooled activated output, no gather (bf16 storage: xhat from the ROUNDED pooled value)
                    CDRL_TRY(pool_bn_bwd_reduce(ps, y.p, G, B, C, stats, scr_main_.part, st, at));
                    return bn_bwd_finalize(scr_main_.part, nb_pool, G, Mg, C, stats, gamma.g, beta.g, coef, st);
                }
                CDRL_TRY(bn_bwd_reduce(none, 0, yv, G, Mg, C, stats, ACT_RELU6, scr_main_.part, st, &ps));
                CDRL_TRY(bn_bwd_finalize(scr_main_.part, nb, G, Mg, C, stats, gamma.g, beta.g, coef, st));
                CDRL_TRY(sched_.next_slot(st));
                return bn_bwd_apply(none, 0, yv, G, Mg, C, stats, coef, ACT_RELU6, dys_[sched_.slot()], part2s_[sched_.slot()], st, &ps);
            };
            ops.push_back(bn);
        }

        // ---- stages (core/architectures.py:120-151,164-167)
        Tens X = pool;
        int curH = Hp, curW = Wp, curC = c.stem;
        for (int s = 0; s < 3; ++s) {
            for (int u = 0; u < c.stage_n[s]; ++u) {
                const int stride = u == 0 ? 2 : 1;
                const int C = c.stage_c[s];
                const int sc_c = stride == 2 ? curC : curC / 2;
                const int main_in = stride == 2 ? curC : curC - sc_c;
                const int main_off = stride == 2 ? 0 : sc_c;
                const int mid = C / 2, main_out = C - sc_c;
                const int Ho = stride == 2 ? same_out_h(curH, 2) : curH, Wo = stride == 2 ? same_out_h(curW, 2) : curW;
                const int rows_in = N * curH * curW, rows_out = N * Ho * Wo;
                const int Mg_in = B * curH * curW;
                const std::string pre = "img.s" + std::to_string(s) + ".u" + std::to_string(u);
                Tens out = tens_a(rows_out, C);
                note_named(pre + ".out", out.p, (size_t)rows_out * C * esz());        // unit output / its gradient (per-unit parity tests)
                note_named(pre + ".out.g", out.g, (size_t)rows_out * C * esz());
                // stride-2 units: the shortcut branch (dw3x3/s2 -> BN -> 1x1 -> BN+ReLU6) only depends on the unit input; in the
                // FORWARD pass (where the side stream is idle) it runs on the side stream next to the main branch
                const bool sc_overlap = stride == 2;
                const int sc_ev = s;
                if (sc_overlap) {
                    Op fk;
                    fk.fwd = [=](hipStream_t st, int) -> int { return sched_.fork_shortcut(st, sc_ev); };
                    fk.bwd = [](hipStream_t) -> int { return 0; };
                    ops.push_back(fk);
                }
                Passthrough pass;
                static const bool fuse_pass = env_on("CDRL_FUSED_PASS");
                if (stride == 1 && fuse_pass && sc_c == C - sc_c) {
                    // identity half: carried by the unit's last BatchNorm op (same channel count as the main half)
                    pass.fsrc = X.v(0);
                    pass.fdst = out.v(0);
                    pass.gsrc = out.gv(0);
                    pass.gdst = X.gv(0);
                } else if (stride == 1) {
                    if (at) build_fail("%s: the stand-alone identity-half copy has no bf16-storage form (CDRL_FUSED_PASS=0 is set)", pre.c_str());
                    Op cp;                      // shortcut half: identity through concat + shuffle
                    View src = X.v(0), dst = out.v(0), gsrc = out.gv(0), gdst = X.gv(0);
                    cp.fwd = [=](hipStream_t st, int) -> int {
                        return bn_apply(src, 1, rows_in, sc_c, nullptr, ACT_NONE, dst, C, st);
                    };
                    cp.bwd = [=](hipStream_t st) -> int { return gather_view(gsrc, C, rows_in, sc_c, gdst, 0, st); };
                    ops.push_back(cp);
                }
                Tens y1 = tens_a(rows_in, mid, false);
                const View xin = X.v(main_off), xg = X.gv(main_off);
                // BatchNorm work folded into the 1x1-conv GEMMs, every stage
                // (the K, N = 232 variants of stage 2 run at one workgroup per CU -- 116 W-fragment VGPRs per wave; slower than the
                //  tiled GEMM + separate BN passes at v19 (+0.15 ms), faster at v29 (-0.24 ms/update-step))
                // (the views of y2 / y3 are probed as null pointers: every tens_a tensor is dense and 256-byte aligned, like them)
                const bool fpw = fused_dw_ && fused_pw_ && pw_nn_supported(xin, mid, main_in) && pw_nn_supported(make_view(nullptr, mid), main_out, mid) &&
                                 pw_nn_supported(make_view(nullptr, main_out), mid, main_out) && pw_nn_supported(y1.v(), main_in, mid);
                // BN-backward apply as GEMM operand prologue (needs the filter-gradient GEMM's fixed column mapping)
                // (also for N <= 32 outputs of the backward-data GEMM, i.e. the first unit's 24 input channels; see CDRL_FUSED_BB above)
                // (also for the wide stage-2 units: without the prologues there 19.55 vs 18.82 ms/update-step;
                //  CU-masking the side stream re-measured at v33: 224 / 192 / 128 CUs -> 21.2 / 21.2 / 23.5 vs 18.7 ms)
                const bool bb1 = fpw && fused_bb_ && gemm_tn_dpro_supported(mid);
                const bool bb3 = fpw && fused_bb_ && gemm_tn_dpro_supported(main_out);
                // order: blocks of bn1, plan of pw1, then the ops (pw1; bn1, dw, bn2, pw2, bn3 from add_half)
                BnRec bn1 = pw_bn(pre + ".pw1", main_in, mid, pre + ".bn1", y1.p, Mg_in, ACT_RELU6);
                // dz (default view) = the masked gradient the depthwise op leaves in the current scratch slot; BN1's backward sums come out
                // of the depthwise backward too
                const PwConv pw1{pre + ".pw1", xin, rows_in, main_in, mid, y1.p, xg, stride == 2 ? 1 : 0};
                const ConvPlan p1 = plan_pw(pw1, fpw, bb1, false);
                if (fpw) bn1.bwd_nb = dwf_plan(B, T, curH, curW, mid, stride).nb_bwd;
                add_pw(ops, pw1, p1, BnRec(), bn1);
                Half mh{pre, "dw", "bn2", "pw2", "bn3", DwBlock{y1.p, curH, curW, mid, stride}, out, sc_c};
                mh.d.pre = bn1;
                mh.d.pre_conv = p1;
                mh.Cout = main_out;
                mh.fused = fpw;
                mh.bb = bb3;
                mh.pass = pass;
                add_half(ops, mh);
                if (stride == 2) {
                    // Round 6: the shortcut branch dw3x3/s2 -> BN -> 1x1 -> BN+ReLU6 (core/architectures.py:133-137) is the second half of a
                    // main branch and runs on the same fused ops (fused conv backward: stages 0 / 1; the BatchNorm-sum epilogue of the
                    // wide kernel: stage 2).  Before: 3 more launches per stride-2 unit on the critical stream of every backward (apply
                    // of sc_bn2, reduce + finalize of sc_bn1) and two on the forward's side stream.
                    const size_t sc_begin = ops.size();
                    if (sc_overlap) build_scr_ = &scr_sc_;
                    Half sh{pre, "sc_dw", "sc_bn1", "sc_pw", "sc_bn2", DwBlock{X.p, curH, curW, sc_c, 2, X.gv(0)}, out, 0, sc_c};
                    // (null probe view: every tens_a tensor is dense and 256-byte aligned, like the null pointer)
                    sh.fused = sh.bb = fused_dw_ && fused_pw_ && fused_bb_ && gemm_tn_dpro_supported(sc_c) && pw_nn_supported(make_view(nullptr, sc_c), sc_c, sc_c);
                    add_half(ops, sh);
                    if (sc_overlap) {
                        build_scr_ = &scr_main_;
                        for (size_t i = sc_begin; i < ops.size(); ++i) {        // forward of the shortcut ops -> side stream
                            auto f = ops[i].fwd;
                            ops[i].fwd = [=](hipStream_t st, int training) -> int { return f(sched_.side_on() ? sched_.side() : st, training); };
                        }
                        Op jn;
                        jn.fwd = [=](hipStream_t st, int) -> int { return sched_.join_shortcut(st, sc_ev); };
                        jn.bwd = [](hipStream_t) -> int { return 0; };
                        ops.push_back(jn);
                    }
                }
                X = out;
                curH = Ho;
                curW = Wo;
                curC = C;
            }
        }
        // ---- head conv + GAP (core/architectures.py:170-172)
        const int P = curH * curW, rows = N * P;
        Tens yh = tens_a(rows, c.last, false);
        const BnRec head_bn = pw_bn("img.head.conv", curC, c.last, "img.head.bn", yh.p, B * P, ACT_RELU6);
        const PwConv head{"img.head.conv", X.v(), rows, curC, c.last, yh.p, X.gv()};
        add_pw(ops, head, plan_pw(head, false, false, false), BnRec(), head_bn);
        feat_ = tens(N, c.last);
        // BatchNorm + ReLU6 + GlobalAveragePooling2D as one op: the 12288 x 768 activated tensor and its gradient are never
        // written -- the forward pools on the fly, the backward reads the pooled gradient broadcast over the frame's pixels
        BnOp hp;
        hp.pass.gap_out = feat_.p;
        hp.pass.gap_dout = feat_.g;
        hp.pass.gap_rows = P;
        add_bn(ops, head_bn, hp);
    }

    // every trunk parameter registered from here on is a TAIL tensor (feature nets, GRUs, concat BN + Dense): their gradients
    // are final at the `mark` op below, those of the tower above only at the end of the backward
    if (!table_frozen_) tail_off_ = tr_size_[M_TRUNK];
    // ---- feature nets (core/architectures.py:9-27)
    const char* fnames[3] = {"road", "vehicle", "navigation"};
    const int fdims[3] = {c.road, c.vehicle, c.navigation};
    Tens fout[3];
    for (int i = 0; i < 3; ++i) {
        const std::string nm = fnames[i];
        const int D = fdims[i];
        Tens xin = tens(N, D, false);
        Op pin;
        const int which = i;
        pin.fwd = [=](hipStream_t st, int) -> int {
            const float* src = which == 0 ? in_road_ : (which == 1 ? in_vehicle_ : in_navigation_);
            return permute_bt(src, xin.p, B, T, D, st);
        };
        pin.bwd = [](hipStream_t) -> int { return 0; };
        build_scr_ = &scr_aux_;
        aux_ops_.push_back(pin);
        Tens a0 = tens(N, c.feat), n0 = tens(N, c.feat), a1 = tens(N, c.feat), n1 = tens(N, c.feat);
        add_dense(aux_ops_, M_TRUNK, nm + ".fc0", xin.v(), N, D, c.feat, ACT_RELU6, a0.v(), a0.gv(), View{nullptr, 0, 0}, 0,
                  false, "glorot");
        add_dense_bn(aux_ops_, M_TRUNK, nm + ".bn0", a0, n0, T);
        add_dense(aux_ops_, M_TRUNK, nm + ".fc1", n0.v(), N, c.feat, c.feat, ACT_RELU6, a1.v(), a1.gv(), n0.gv(), 0, true,
                  "glorot");
        add_dense_bn(aux_ops_, M_TRUNK, nm + ".bn1", a1, n1, T);
        build_scr_ = &scr_main_;
        fout[i] = n1;
    }

    // ---- GRUs + concat + BN + Dense (core/networks.py:44-56)
    const int catC = c.rnn_image + 3 * c.rnn_small;
    Tens cat = tens(B, catC);
    {   // backward: everything behind this point of the (reversed) op list -- heads, concat BN + Dense, the small-modality
        // nets on the aux stream, the image GRU -- has its gradient work enqueued: hand the "tail gradients final" point to
        // the caller's communication stream (DataParallelLearner: early all-reduce bucket under the tower's backward)
        Op mark;
        mark.fwd = [](hipStream_t, int) -> int { return 0; };
        mark.bwd = [=](hipStream_t st) -> int { return sched_.publish_tail(st); };
        ops.push_back(mark);
    }
    add_gru(ops, "gru_image", feat_, c.last, c.rnn_image, cat.v(0), cat.gv(0), true);
    build_scr_ = &scr_aux_;
    for (int i = 0; i < 3; ++i)
        add_gru(aux_ops_, std::string("gru_") + fnames[i], fout[i], c.feat, c.rnn_small, cat.v(c.rnn_image + i * c.rnn_small),
                cat.gv(c.rnn_image + i * c.rnn_small), true);
    build_scr_ = &scr_main_;
    add_aux_join(ops);
    Tens ncat = tens(B, catC);
    add_dense_bn(ops, M_TRUNK, "dyn.bn", cat, ncat, 1);
    dyn_ = tens(B, c.dyn);
    add_dense(ops, M_TRUNK, "dyn.fc", ncat.v(), B, catC, c.dyn, ACT_NONE, dyn_.v(), dyn_.gv(), ncat.gv(), 0, true, "glorot");
}

void Learner::build_head(std::vector<Op>& ops, int model, const std::string& prefix, Tens& lin, int nheads,
                         const int* head_dims, const char* const* head_names) {
    const Config& c = cfg_;
    const int B = c.B;
    Tens n0 = tens(B, c.dyn), a0 = tens(B, c.head), n1 = tens(B, c.head), a1 = tens(B, c.head);
    {   // bn0 as add_dense_bn emits it; the policy and value heads keep its record for the joint pass
        BnOp o;
        o.bessel = false;
        o.out = n0.v();
        o.dout = n0.gv();
        o.dx = dyn_.g;
        const BnRec bn = make_bn(model, prefix + ".bn0", dyn_.v(), 1, dyn_.rows, dyn_.C, ACT_NONE);
        const size_t at_op = ops.size();
        const bool small = add_bn(ops, bn, o);
        if (model == M_POLICY || model == M_VALUE) {
            HeadBn0& h = bn0_[model == M_POLICY ? 0 : 1];
            h.bn = bn;
            h.dout = o.dout;
            h.op = at_op;
            h.small = small;
        }
    }
    add_dense(ops, model, prefix + ".fc0", n0.v(), B, c.dyn, c.head, ACT_SWISH6, a0.v(), a0.gv(), n0.gv(), 0, true, "glorot");
    add_dense_bn(ops, model, prefix + ".bn1", a0, n1, 1);
    add_dense(ops, model, prefix + ".fc1", n1.v(), B, c.head, c.head, ACT_SWISH6, a1.v(), a1.gv(), n1.gv(), 0, true, "glorot");
    int L = 0;
    for (int i = 0; i < nheads; ++i) L += head_dims[i];
    lin = tens(B, L);
    if (nheads <= HEADS_MAX && L <= HEADS_MAX_OUT) {
        // all linear heads of the branch in one launch per direction (heads.hip); same parameter names / order as add_dense
        HeadSet hs{};
        hs.nheads = nheads;
        int off = 0;
        for (int i = 0; i < nheads; ++i) {
            PRef w = param(model, prefix + "." + head_names[i] + ".w", {c.head, head_dims[i]}, true);
            PRef b = param(model, prefix + "." + head_names[i] + ".b", {head_dims[i]}, true);
            hs.n[i] = head_dims[i];
            hs.off[i] = off;
            hs.w[i] = w.p;
            hs.b[i] = b.p;
            hs.gw[i] = w.g;
            hs.gb[i] = b.g;
            off += head_dims[i];
        }
        const int K = c.head;
        Tens a1c = a1, linc = lin;
        Op op;
        op.fwd = [=](hipStream_t st, int) -> int { return heads_fwd(a1c.p, K, hs, linc.p, L, B, K, st); };
        op.bwd = [=](hipStream_t st) -> int { return heads_bwd(a1c.p, K, hs, linc.g, L, a1c.g, K, B, K, st); };
        ops.push_back(op);
        return;
    }
    int off = 0;
    for (int i = 0; i < nheads; ++i) {
        add_dense(ops, model, prefix + "." + head_names[i], a1.v(), B, c.head, head_dims[i], ACT_NONE, lin.v(off),
                  lin.gv(off), a1.gv(), i < nheads - 1 ? 1 : 0, true, "glorot");
        off += head_dims[i];
    }
}

void Learner::alloc_scratch() {
    const SlotSizes ss = slot_sizes();
    for (Scratch* s : {&scr_main_, &scr_aux_, &scr_sc_}) {
        s->part = alloc_d(max_part_);
        s->part2 = alloc_d(max_part2_);
    }
    scr_main_.tn = alloc(max_tn_);
    scr_aux_.tn = alloc(max_tn_);
    scr_sc_.tn = scr_aux_.tn;           // (unused by the shortcut ops)
    for (int i = 0; i < NSLOT; ++i) {
        dys_[i] = alloc((ss.dy * esz() + 3) / 4);      // tower gradients: activation-typed
        part2s_[i] = alloc_d(ss.part2);
        tns_[i] = alloc(ss.tn);
        fparts_[i] = alloc_d(ss.fpart);
    }
    for (int i = 0; i < NQ; ++i) {
        qparts_[i] = alloc(ss.qpart);
        dbparts_[i] = alloc_d(ss.dbpart);
        fintots_[i] = alloc_d(ss.fintot);
    }
}

void Learner::build(bool dry) {
    dry_ = dry;
    ws_off_ = 0;
    guard_off_.clear();
    trunk_ops_.clear();
    policy_ops_.clear();
    value_ops_.clear();
    old_policy_ops_.clear();
    // the scratch blocks are sized by the maxima the dry build collects: the real layout starts with them, the dry build (where alloc
    // only counts bytes and bands) adds them once its op lists are built
    if (!dry) alloc_scratch();
    h_pwt_.clear();
    pwt_by_name_.clear();
    pwt_tiles_ = 0;
    zero_once_.clear();
    h_pack_.clear();
    h_pack3_.clear();
    h_gpack_.clear();
    h_bninf_.clear();
    bninf_max_c_ = 0;
    building_trunk_ = true;
    build_trunk(trunk_ops_);
    building_trunk_ = false;
    const int A = cfg_.A;
    const int pdims[4] = {A, A, 1, 1};
    const char* const pnames[4] = {"alpha", "beta", "similarity", "speed"};
    build_head(policy_ops_, M_POLICY, "pi", lin_p_, 4, pdims, pnames);
    const int vdims[4] = {1, 1, 1, 1};
    const char* const vnames[4] = {"base", "exp", "speed", "similarity"};
    build_head(value_ops_, M_VALUE, "v", lin_v_, 4, vdims, vnames);
    build_head(old_policy_ops_, M_OLD_POLICY, "pi", lin_old_, 4, pdims, pnames);
    // device copies of the per-pass tables (packed weights, inference statistics, transposes): sized AFTER the heads are built, so that an
    // op of a control branch may register entries too (round 6: a small-M GEMM that did so overflowed the table sized behind the trunk)
    d_bninf_ = reinterpret_cast<BnInfEntry*>(alloc((h_bninf_.size() + 1) * sizeof(BnInfEntry) / sizeof(float) + 4));
    d_pack_ = reinterpret_cast<PwPack*>(alloc((h_pack_.size() + 1) * sizeof(PwPack) / sizeof(float) + 4));
    d_pack3_ = reinterpret_cast<PwX3Pack*>(alloc((h_pack3_.size() + 1) * sizeof(PwX3Pack) / sizeof(float) + 4));
    d_gpack_ = reinterpret_cast<GemmX3Pack*>(alloc((h_gpack_.size() + 1) * sizeof(GemmX3Pack) / sizeof(float) + 4));
    d_pwt_ = reinterpret_cast<PwTranspose*>(alloc((h_pwt_.size() + 1) * sizeof(PwTranspose) / sizeof(float) + 4));
    metrics_p_ = alloc(32);                                 // policy metrics, then the representation pass's (one 256-byte unit)
    metrics_r_ = dry_ ? nullptr : metrics_p_ + 16;
    metrics_v_ = alloc(16);
    ntxent_ws_ = nullptr;
    if (!frozen() && cfg_.B % 2 == 0 && cfg_.B <= 2048) {   // (the learners the representation pass accepts)
        const size_t need = (size_t)ntxent_workspace_floats(cfg_.B, cfg_.dyn);
        const size_t have = (slot_sizes().dy * esz() + 3) / 4;      // floats of a backward slot's tower-gradient block
        // dry build: the slots are sized behind the op lists, from the same maxima; the real build has them already
        if (need > have) ntxent_ws_ = alloc(need);
        else if (!dry_) ntxent_ws_ = dys_[0];
    }
    aux_p_ = alloc((size_t)cfg_.B * 4 * A);
    aux_v_ = alloc((size_t)cfg_.B * 2);
    sample_u_ = alloc((size_t)cfg_.B * A);
    sample_da_ = alloc((size_t)cfg_.B * A);
    sample_db_ = alloc((size_t)cfg_.B * A);
    note_named("sample.u", sample_u_, (size_t)cfg_.B * A * sizeof(float));
    note_named("sample.du_dalpha", sample_da_, (size_t)cfg_.B * A * sizeof(float));
    note_named("sample.du_dbeta", sample_db_, (size_t)cfg_.B * A * sizeof(float));
    hp_dev_ = reinterpret_cast<DevHP*>(alloc(sizeof(DevHP) / sizeof(float) + 4));
    note_named("hparams", hp_dev_, sizeof(DevHP));      // 10 floats (lr x3, clip, entropy, clip norms x2, beta1, beta2, eps), 3 int step counters,
                                                        // 3 Nadam m_caches
    // optimiser tables
    // (train stats, unfrozen: the trunk gets a table too -- its norms are diagnostics there; the gradient gate folds them into the
    // trunk list's norm)
    for (int m = trunk_table() ? 0 : 1; m <= 2; ++m) {
        SegTable& s = seg_[m];
        int nt = 0;
        int64_t nch = 0;
        for (const ParamInfo& pi : infos_[m])
            if (pi.trainable) {
                ++nt;
                nch += (pi.numel + 1023) / 1024;
            }
        s.dev.segs = reinterpret_cast<TensorSeg*>(alloc((size_t)nt * sizeof(TensorSeg) / sizeof(float)));
        s.dev.chunk_tensor = reinterpret_cast<int*>(alloc((size_t)nch));
        s.dev.chunk_off = reinterpret_cast<int64_t*>(alloc((size_t)nch * 2));
        s.dev.chunk_part = alloc_d((size_t)nch);
        alloc((size_t)nt);      // unnamed padding: every offset behind the tables, and so the workspace size, is pinned by the planner's tests
    }
    if (gate_on() || trust_on()) {
        gate_dev_ = reinterpret_cast<GateBlock*>(alloc(sizeof(GateBlock) / sizeof(float) + 4));
        note_named("gate", gate_dev_, sizeof(GateBlock));
    }
    if (trust_on()) {
        trust_dev_ = reinterpret_cast<TrustBlock*>(alloc_d(sizeof(TrustBlock) / sizeof(double) + 2));
        note_named("trust", trust_dev_, sizeof(TrustBlock));
        note_named("policy.lin.g", lin_p_.g, (size_t)cfg_.B * (2 * A + 2) * sizeof(float));
    }
    if (cfg_.train_stats > 0) {
        stats_ring_ = alloc(stats_bytes() / sizeof(float));
        if (!dry_) zero_once_.push_back(std::make_pair(stats_ring_, (size_t)STATS_HEADER * sizeof(float)));
    }
    if (dry) alloc_scratch();
    if (guard_) {       // band table (device) behind everything else; no band behind it
        const bool g = guard_;
        guard_ = false;
        guard_tab_ = reinterpret_cast<int64_t*>(alloc_d(GUARD_TABLE_MAX + 2));
        guard_ = g;
        if (!dry && guard_off_.size() > GUARD_TABLE_MAX) build_fail("CDRL_GUARD: %zu bands exceed the table", guard_off_.size());
    }
    if (dry) ws_bytes_ = ws_off_ + 4096;
}

void Learner::build_seg_tables() {
    for (int m = trunk_table() ? 0 : 1; m <= 2; ++m) {
        SegTable& s = seg_[m];
        s.h_segs.clear();
        s.h_chunk_tensor.clear();
        s.h_chunk_off.clear();
        for (const ParamInfo& pi : infos_[m]) {
            if (!pi.trainable) continue;
            TensorSeg seg;
            seg.off = pi.off;
            seg.n = pi.numel;
            seg.first_chunk = (int)s.h_chunk_tensor.size();
            seg.nchunks = (int)((pi.numel + 1023) / 1024);
            for (int k = 0; k < seg.nchunks; ++k) {
                s.h_chunk_tensor.push_back((int)s.h_segs.size());
                s.h_chunk_off.push_back(pi.off + (int64_t)k * 1024);
            }
            s.h_segs.push_back(seg);
        }
        s.dev.ntensors = (int)s.h_segs.size();
        s.dev.nchunks = (int)s.h_chunk_tensor.size();
    }
}

int Learner::upload_seg_tables() {
    if (!h_pwt_.empty())
        CDRL_HIP(hipMemcpy(d_pwt_, h_pwt_.data(), h_pwt_.size() * sizeof(PwTranspose), hipMemcpyHostToDevice));
    if (!h_pack_.empty())
        CDRL_HIP(hipMemcpy(d_pack_, h_pack_.data(), h_pack_.size() * sizeof(PwPack), hipMemcpyHostToDevice));
    if (!h_bninf_.empty())
        CDRL_HIP(hipMemcpy(d_bninf_, h_bninf_.data(), h_bninf_.size() * sizeof(BnInfEntry), hipMemcpyHostToDevice));
    if (!h_pack3_.empty())
        CDRL_HIP(hipMemcpy(d_pack3_, h_pack3_.data(), h_pack3_.size() * sizeof(PwX3Pack), hipMemcpyHostToDevice));
    if (!h_gpack_.empty())
        CDRL_HIP(hipMemcpy(d_gpack_, h_gpack_.data(), h_gpack_.size() * sizeof(GemmX3Pack), hipMemcpyHostToDevice));
    for (int m = trunk_table() ? 0 : 1; m <= 2; ++m) {
        SegTable& s = seg_[m];
        CDRL_HIP(hipMemcpy(s.dev.segs, s.h_segs.data(), s.h_segs.size() * sizeof(TensorSeg), hipMemcpyHostToDevice));
        CDRL_HIP(hipMemcpy(s.dev.chunk_tensor, s.h_chunk_tensor.data(), s.h_chunk_tensor.size() * sizeof(int),
                           hipMemcpyHostToDevice));
        CDRL_HIP(hipMemcpy(s.dev.chunk_off, s.h_chunk_off.data(), s.h_chunk_off.size() * sizeof(int64_t),
                           hipMemcpyHostToDevice));
    }
    return 0;
}

int Learner::bind(const Buffers& b) {
    if (!b.params || !b.grads || !b.adam_m || !b.adam_v || !b.workspace) {
        set_error("bind: null buffer");
        return -1;
    }
    if (b.workspace_bytes < ws_bytes_) {
        set_error("bind: workspace too small (%zu < %zu)", b.workspace_bytes, ws_bytes_);
        return -1;
    }
    drop_graphs();
    named_.clear();
    buf_ = b;
    ws_base_ = reinterpret_cast<char*>(b.workspace);
    build(false);
    if (ws_off_ > b.workspace_bytes) {
        set_error("bind: internal workspace overflow");
        return -1;
    }
    CDRL_TRY(upload_seg_tables());
    for (auto& z : zero_once_) CDRL_HIP(hipMemset(z.first, 0, z.second));
    if (guard_) {
        if (!build_err_.empty()) {
            set_error("bind: %s", build_err_.c_str());
            return -1;
        }
        CDRL_HIP(hipMemcpy(guard_tab_, guard_off_.data(), guard_off_.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(guard_fill_kernel, dim3((unsigned)guard_off_.size()), dim3(256), 0, nullptr, ws_base_, guard_tab_, (int)(GUARD_BYTES / 4));
        CDRL_LAUNCH_CHECK();
        CDRL_HIP(hipDeviceSynchronize());
    }
    if (!sched_.created()) CDRL_TRY(sched_.create());
    if (!hp_stage_) CDRL_HIP(hipHostMalloc(reinterpret_cast<void**>(&hp_stage_), sizeof(DevHP) + sizeof(float), 0));
    CDRL_HIP(hipMemcpy(hp_dev_, &hp_host_, sizeof(DevHP), hipMemcpyHostToDevice));
    if (gate_dev_) CDRL_HIP(hipMemcpy(gate_dev_, &gate_host_, sizeof(GateBlock), hipMemcpyHostToDevice));
    if (trust_dev_) CDRL_HIP(hipMemcpy(trust_dev_, &trust_host_, sizeof(TrustBlock), hipMemcpyHostToDevice));
    return 0;
}

int Learner::upload_hp(hipStream_t st) {
    // only the float block (lr / clip / entropy / betas); the Adam counters stay device-resident
    memcpy(hp_stage_, &hp_host_, sizeof(DevHP));
    CDRL_HIP(hipMemcpyAsync(hp_dev_, hp_stage_, offsetof(DevHP, t_policy), hipMemcpyHostToDevice, st));
    if (gate_dev_) {        // the gate block's one host-written field; DevHP keeps its layout
        static_assert(offsetof(GateBlock, clip_norm_dynamics) == 0, "the host writes the first float of the gate block");
        float* stage = reinterpret_cast<float*>(hp_stage_ + 1);
        *stage = gate_host_.clip_norm_dynamics;
        CDRL_HIP(hipMemcpyAsync(gate_dev_, stage, sizeof(float), hipMemcpyHostToDevice, st));
    }
    tail_invalidate(st);
    return 0;
}

int Learner::upload_trust(hipStream_t st) {
    if (!trust_dev_) {
        set_error("set_trust_params: the learner was created without cdrl_config.trust = 1, or is not bound");
        return -1;
    }
    // by value through a one-thread launch (as set_steps): no staging buffer that a later call could rewrite before this one has run
    CDRL_TRY(trust_set_params(trust_dev_, trust_host_.target_kl, trust_host_.kl_stop_factor, trust_host_.kl_coef, st));
    tail_invalidate(st);
    return 0;
}

int Learner::trust_stats(TrustBlock* out, hipStream_t st) {
    if (!trust_dev_) {
        set_error("trust_stats: the learner was created without cdrl_config.trust = 1, or is not bound");
        return -1;
    }
    CDRL_HIP(hipMemcpyAsync(out, trust_dev_, sizeof(TrustBlock), hipMemcpyDeviceToHost, st));
    tail_invalidate(st);
    CDRL_HIP(hipStreamSynchronize(st));
    return 0;
}

int Learner::trust_reset_block(hipStream_t st) {
    if (!trust_dev_) {
        set_error("trust_reset: the learner was created without cdrl_config.trust = 1, or is not bound");
        return -1;
    }
    CDRL_TRY(trust_reset(trust_dev_, st));
    tail_invalidate(st);
    return 0;
}

int Learner::gate_stats(GateBlock* out, hipStream_t st) {
    if (!gate_dev_) {
        set_error("gate_stats: the learner has neither clip_mode = global nor skip_nonfinite, or is not bound");
        return -1;
    }
    CDRL_HIP(hipMemcpyAsync(out, gate_dev_, sizeof(GateBlock), hipMemcpyDeviceToHost, st));
    tail_invalidate(st);
    CDRL_HIP(hipStreamSynchronize(st));
    return 0;
}

int Learner::gate_reset(hipStream_t st) {
    if (!gate_dev_) {
        set_error("gate_reset: the learner has neither clip_mode = global nor skip_nonfinite, or is not bound");
        return -1;
    }
    static_assert(offsetof(GateBlock, applied) == offsetof(GateBlock, skipped) + 2 * sizeof(int), "the four counters are contiguous");
    CDRL_HIP(hipMemsetAsync(reinterpret_cast<unsigned char*>(gate_dev_) + offsetof(GateBlock, skipped), 0, 4 * sizeof(int), st));
    tail_invalidate(st);
    return 0;
}

int Learner::reset_counters(hipStream_t st) {
    CDRL_TRY(reset_steps(hp_dev_, st));      // counters 0, Nadam m_caches 1
    tail_invalidate(st);
    return 0;
}

int Learner::get_counters(int t[3], float m_cache[3], hipStream_t st) {
    if (!hp_dev_) {
        set_error("get_optimizer_state: learner not bound");
        return -1;
    }
    static_assert(offsetof(DevHP, m_cache_dynamics) + sizeof(float) == sizeof(DevHP) &&
                      offsetof(DevHP, m_cache_policy) == offsetof(DevHP, t_policy) + 3 * sizeof(int),
                  "DevHP ends in 3 int counters and 3 float m_caches");
    unsigned char tail[sizeof(DevHP) - offsetof(DevHP, t_policy)];
    CDRL_HIP(hipMemcpyAsync(tail, reinterpret_cast<const unsigned char*>(hp_dev_) + offsetof(DevHP, t_policy), sizeof(tail),
                            hipMemcpyDeviceToHost, st));
    tail_invalidate(st);
    CDRL_HIP(hipStreamSynchronize(st));
    memcpy(t, tail, 3 * sizeof(int));
    memcpy(m_cache, tail + 3 * sizeof(int), 3 * sizeof(float));
    return 0;
}

int Learner::set_counters(const int t[3], const float m_cache[3], hipStream_t st) {
    if (!hp_dev_) {
        set_error("set_optimizer_state: learner not bound");
        return -1;
    }
    static const char* const names[3] = {"policy", "value", "dynamics"};
    for (int i = 0; i < 3; ++i) {       // validate everything first: a refused state writes nothing
        if (t[i] < 0) {
            set_error("set_optimizer_state: t_%s = %d is negative", names[i], t[i]);
            return -1;
        }
        if (!std::isfinite(m_cache[i]) || !(m_cache[i] > 0.0f)) {
            set_error("set_optimizer_state: m_cache_%s = %g is not a finite positive number", names[i], (double)m_cache[i]);
            return -1;
        }
    }
    CDRL_TRY(set_steps(hp_dev_, t, m_cache, st));
    tail_invalidate(st);
    return 0;
}

// ------------------------------------------------------------------------------------------
// execution
// ------------------------------------------------------------------------------------------
int Learner::run_fwd(std::vector<Op>& ops, hipStream_t st, int training) {
    for (Op& op : ops) CDRL_TRY(op.fwd(st, training));
    return 0;
}

int Learner::run_bwd(std::vector<Op>& ops, hipStream_t st, size_t first) {
    for (size_t i = ops.size(); i-- > first;) CDRL_TRY(ops[i].bwd(st));
    return 0;
}

int Learner::set_inputs(const float* image, const float* road, const float* vehicle, const float* navigation) {
    if (!ws_base_) {
        set_error("learner not bound");
        return -1;
    }
    if (!image || !road || !vehicle || !navigation) {
        set_error("null state input");
        return -1;
    }
    in_image_ = image;
    in_road_ = road;
    in_vehicle_ = vehicle;
    in_navigation_ = navigation;
    return 0;
}

int Learner::trunk_forward_train(const float* image, const float* road, const float* vehicle, const float* navigation,
                                 hipStream_t caller) {
    return launch(caller, {}, false, [&](hipStream_t st) -> int {
        CDRL_TRY(set_inputs(image, road, vehicle, navigation));
        return run_trunk_fwd(st, 1);
    });
}

// ------------------------------------------------------------------------------------------
// Training passes.  Every entry describes its pass as a PassSpec and goes through run_pass; both heads present: the joint
// policy + value update, one trunk forward and one trunk backward per minibatch
// ------------------------------------------------------------------------------------------
static inline uint64_t K(const void* p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); }
static inline uint64_t Kf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
// step kind: the first word of a graph key
enum KeyKind : uint64_t {
    KEY_POLICY_PASS = 1, KEY_VALUE_PASS = 2, KEY_POLICY_APPLY = 3, KEY_VALUE_APPLY = 4, KEY_PREDICT = 5, KEY_JOINT_PASS = 6, KEY_JOINT_APPLY = 7,
    KEY_CLONE_PASS = 8, KEY_REPR_PASS = 9, KEY_TRUNK_APPLY = 10, KEY_DEMO_PASS = 11
};

PolicyLossArgs Learner::policy_loss_args(const PassSpec& s) const {
    PolicyLossArgs a;
    a.lin = lin_p_.p;
    a.adv = s.policy->adv;
    a.old_logp = s.policy->old_logp;
    a.speed = s.speed;
    a.similarity = s.similarity;
    a.u = s.resample ? sample_u_ : s.policy->u;
    a.du_da = s.resample ? sample_da_ : s.policy->du_da;
    a.du_db = s.resample ? sample_db_ : s.policy->du_db;
    a.hp = reinterpret_cast<const float*>(hp_dev_);
    a.dlin = lin_p_.g;
    a.metrics = metrics_p_;
    a.aux = aux_p_;
    a.B = cfg_.B;
    a.A = cfg_.A;
    a.inv_world = s.inv_world;
    return a;
}

CloneLossArgs Learner::clone_loss_args(const PassSpec& s) const {
    CloneLossArgs a;
    a.lin = lin_p_.p;
    a.u = s.clone_u;
    a.weight = s.clone_w;
    a.speed = s.speed;
    a.similarity = s.similarity;
    a.hp = reinterpret_cast<const float*>(hp_dev_);
    a.entropy_coef = 0.0f;
    a.aux_weight = s.aux_weight;
    a.dlin = lin_p_.g;
    a.metrics = metrics_p_;
    a.aux = aux_p_;
    a.B = cfg_.B;
    a.A = cfg_.A;
    a.grad_scale = s.inv_world * s.policy_weight;
    return a;
}

MixedPolicyLossArgs Learner::mixed_loss_args(const PassSpec& s) const {
    MixedPolicyLossArgs a;
    a.ppo = policy_loss_args(s);
    a.demo_u = s.demo_u;
    a.demo_w = s.demo_w;
    a.block = demo_block_;
    return a;
}

ValueLossArgs Learner::value_loss_args(const PassSpec& s) const {
    ValueLossArgs a;
    a.lin = lin_v_.p;
    a.returns = s.returns;
    a.speed = s.speed;
    a.similarity = s.similarity;
    a.dlin = lin_v_.g;
    a.metrics = metrics_v_;
    a.values = aux_v_;
    a.B = cfg_.B;
    a.exp_scale = cfg_.exp_scale;
    a.inv_world = s.inv_world * s.value_weight;         // (1 outside a clone pass: the product is exact)
    return a;
}

int Learner::pass_forward(const PassSpec& s, bool dist, hipStream_t st) {
    CDRL_TRY(set_inputs(s.image, s.road, s.vehicle, s.navigation));
    CDRL_TRY(run_trunk_fwd(st, 1));
    if (s.head()) CDRL_TRY(run_fwd(policy_ops_, st, 1));
    const int A = cfg_.A;
    // alpha, beta (+ mean, std) of the CURRENT policy for the Beta re-sampling
    if (dist || s.resample) CDRL_TRY(policy_dist(lin_p_.p, aux_p_, cfg_.B, A, st));
    if (s.resample)     // u ~ Beta(alpha, beta) of the new policy, with its pathwise Jacobians
        CDRL_TRY(beta_sample(aux_p_, aux_p_ + A, cfg_.B, A, 4 * A, s.seed, s.offset, sample_u_, sample_da_, sample_db_, st));
    return s.returns ? run_fwd(value_ops_, st, 1) : 0;
}

NtxentArgs Learner::ntxent_args(const PassSpec& s) const {
    NtxentArgs a;
    a.z = dyn_.p;
    a.dz = dyn_.g;
    a.metrics = metrics_r_;
    a.workspace = ntxent_ws_;
    a.B = cfg_.B;
    a.D = cfg_.dyn;
    a.temperature = s.temperature;
    a.grad_scale = s.inv_world;
    return a;
}

int Learner::pass_backward(const PassSpec& s, hipStream_t st) {
    // joint: each head's backward stops in front of its bn0; one launch then finishes both bn0 over the trunk output -- their own
    // gradients, and dyn_.g = d(policy loss)/d(dynamics) + d(value loss)/d(dynamics)
    const HeadBn0 &p0 = bn0_[0], &v0 = bn0_[1];
    if (s.repr) CDRL_TRY(ntxent_loss(ntxent_args(s), st));   // writes dyn_.g, where a head's bn0 backward would
    // trust learner: a policy pass with an anchor measures its KL (and arms the latch for its apply) behind the policy loss; every
    // other pass that an apply of the policy head or the trunk may follow disarms it, so that no old latch gates it
    const bool measure = trust_on() && s.policy && s.policy->anchor;
    if (trust_on() && !measure && (s.head() || s.repr)) CDRL_TRY(trust_disarm(trust_dev_, st));
    if (s.head()) {
        CDRL_TRY(s.demo_u  ? mixed_policy_loss(mixed_loss_args(s), st)
                 : s.policy ? policy_loss(policy_loss_args(s), st)
                            : clone_loss(clone_loss_args(s), st));
        if (measure) {
            BetaKlArgs k;
            k.lin = lin_p_.p;
            k.anchor = s.policy->anchor;
            k.dlin = lin_p_.g;
            k.trust = trust_dev_;
            k.kl_coef = 0.0f;
            k.metrics = nullptr;
            k.B = cfg_.B;
            k.A = cfg_.A;
            k.inv_world = s.inv_world;
            CDRL_TRY(beta_kl(k, st));
        }
        CDRL_TRY(run_bwd(policy_ops_, st, s.joint() ? p0.op + 1 : 0));
    }
    if (s.returns) {
        CDRL_TRY(value_loss(value_loss_args(s), st));
        CDRL_TRY(run_bwd(value_ops_, st, s.joint() ? v0.op + 1 : 0));
    }
    if (s.joint())
        CDRL_TRY(bn_small_bwd_pair(p0.dout, v0.dout, p0.bn.x, p0.bn.Mg, p0.bn.C, p0.bn.stats, v0.bn.stats, p0.bn.gamma.g, p0.bn.beta.g,
                                   p0.bn.coef, v0.bn.gamma.g, v0.bn.beta.g, v0.bn.coef, dyn_.g, st));
    return trunk_backward_tail(st);
}

int Learner::trunk_backward_tail(hipStream_t st) {
    // Frozen trunk: the heads' backward ends in the BatchNorm of bn0 (joint: the pair launch), which also writes d(loss)/d(dynamics)
    // into the trunk's output gradient.  That write has no consumer here, but up to 2048 rows it comes out of the same launch that
    // produces the BatchNorm's dgamma / dbeta (bn_small_bwd, one launch per direction): it stays, and the head gradients are those of
    // a full pass.
    if (frozen()) return sched_.join_side(st);
    if (!packs_have_wt_) CDRL_TRY(transpose_many(d_pwt_, (int)h_pwt_.size(), pwt_tiles_, st));      // W^T of the pointwise convs (normally packed with the forward's operands)
    CDRL_TRY(run_bwd(trunk_ops_, st));
    return sched_.join_side(st);
}

int Learner::joint_refused() {
    if (bn0_[0].small && bn0_[1].small && bn0_[0].op == 0 && bn0_[1].op == 0) return 0;
    set_error("joint update: the heads' first BatchNorm is not in the single-launch form (B = %d > 2048 rows); use the separate passes",
              cfg_.B);
    return -1;
}

int Learner::repr_refused() {
    if (frozen()) {
        set_error("representation pass: freeze_trunk = 1: the pass trains the trunk and nothing else");
        return -1;
    }
    if (cfg_.B % 2 != 0 || cfg_.B > 2048) {
        set_error("representation pass: B = %d must be even (rows i and i + B/2 are two views) and at most 2048", cfg_.B);
        return -1;
    }
    return 0;
}

int Learner::trust_refused(const PassSpec& s) {
    if (!trust_on() && s.policy && s.policy->anchor) {
        set_error("policy batch: anchor given to a learner created without cdrl_config.trust = 1");
        return -1;
    }
    if (trust_on() && s.joint()) {
        set_error("joint pass: cdrl_config.trust = 1: the trust-region latch gates policy_apply only, half of a joint apply has no gated form");
        return -1;
    }
    return 0;
}

int Learner::run_pass(const PassSpec& s, hipStream_t caller, bool fwd, bool bwd) {
    CDRL_TRY(trust_refused(s));
    if (s.joint()) CDRL_TRY(joint_refused());
    if (s.repr) CDRL_TRY(repr_refused());
    if (s.inv_world != 1.0f) sched_.note_scaled_pass();
    // one half alone (the split form) is eager; so is re-sampling: (seed, offset) are kernel arguments that change every call
    const bool graphable = fwd && bwd && !s.resample;
    std::vector<uint64_t> key;
    if (graphable) {
        key = {s.repr      ? KEY_REPR_PASS
               : s.clone_u ? KEY_CLONE_PASS
               : s.demo_u  ? KEY_DEMO_PASS
               : s.joint() ? KEY_JOINT_PASS
               : s.policy  ? KEY_POLICY_PASS
                           : KEY_VALUE_PASS,
               K(s.image), K(s.road), K(s.vehicle), K(s.navigation), K(s.speed), K(s.similarity), K(s.returns), Kf(s.inv_world)};
        if (const PolicyBatch* b = s.policy) key.insert(key.end(), {K(b->adv), K(b->old_logp), K(b->u), K(b->du_da), K(b->du_db)});
        if (s.policy && s.policy->anchor) key.push_back(K(s.policy->anchor));
        if (s.clone_u) key.insert(key.end(), {K(s.clone_u), K(s.clone_w), Kf(s.policy_weight), Kf(s.value_weight), Kf(s.aux_weight)});
        if (s.demo_u) key.insert(key.end(), {K(s.demo_u), K(s.demo_w), K(demo_block_)});
        if (s.repr) key.push_back(Kf(s.temperature));
    }
    return launch(caller, key, graphable, [&](hipStream_t st) -> int {
        if (fwd) CDRL_TRY(pass_forward(s, !bwd, st));       // (the forward alone: its caller samples from alpha, beta)
        return bwd ? pass_backward(s, st) : 0;
    });
}

int Learner::policy_forward_backward(const PolicyBatch& b, float inv_world, hipStream_t caller) {
    return run_pass(policy_pass(b, nullptr, inv_world), caller);
}

int Learner::policy_forward(const float* image, const float* road, const float* vehicle, const float* navigation,
                            hipStream_t caller) {
    const PolicyBatch b{image, road, vehicle, navigation};
    return run_pass(policy_pass(b, nullptr, 1.0f), caller, true, false);
}

int Learner::policy_backward(const PolicyBatch& b, float inv_world, hipStream_t caller) {
    return run_pass(policy_pass(b, nullptr, inv_world), caller, false, true);
}

int Learner::policy_forward_backward_resample(const PolicyBatch& b, uint64_t seed, uint64_t offset, float inv_world,
                                              hipStream_t caller) {
    return run_pass(policy_pass(b, nullptr, inv_world, true, seed, offset), caller);
}

int Learner::demo_pass(PassSpec s, const float* demo_u, const float* demo_w, hipStream_t caller) {
    if (!demo_u || !demo_w) {
        set_error("demonstration pass: null demo_u / demo_w");
        return -1;
    }
    if (s.policy->anchor) {
        set_error("demonstration pass: the batch carries an anchor: the trust-region sweep has no demonstration rows");
        return -1;
    }
    s.demo_u = demo_u;
    s.demo_w = demo_w;
    return run_pass(s, caller);
}

int Learner::demo_forward_backward(const PolicyBatch& b, const float* demo_u, const float* demo_w, float inv_world, hipStream_t caller) {
    return demo_pass(policy_pass(b, nullptr, inv_world), demo_u, demo_w, caller);
}

int Learner::demo_forward_backward_resample(const PolicyBatch& b, const float* demo_u, const float* demo_w, uint64_t seed, uint64_t offset,
                                            float inv_world, hipStream_t caller) {
    return demo_pass(policy_pass(b, nullptr, inv_world, true, seed, offset), demo_u, demo_w, caller);
}

int Learner::value_forward_backward(const ValueBatch& b, float inv_world, hipStream_t caller) {
    return run_pass({b.image, b.road, b.vehicle, b.navigation, b.speed, b.similarity, nullptr, b.returns, inv_world}, caller);
}

int Learner::joint_forward_backward(const PolicyBatch& b, const float* returns, float inv_world, hipStream_t caller) {
    return run_pass(policy_pass(b, returns, inv_world), caller);
}

int Learner::joint_forward_backward_resample(const PolicyBatch& b, const float* returns, uint64_t seed, uint64_t offset, float inv_world,
                                             hipStream_t caller) {
    return run_pass(policy_pass(b, returns, inv_world, true, seed, offset), caller);
}

int Learner::clone_forward_backward(const CloneBatch& b, float policy_weight, float value_weight, float aux_weight, float inv_world,
                                    hipStream_t caller) {
    PassSpec s{b.image, b.road, b.vehicle, b.navigation, b.speed, b.similarity, nullptr, b.returns, inv_world};
    s.clone_u = b.u;
    s.clone_w = b.weight;
    s.policy_weight = policy_weight;
    s.value_weight = value_weight;
    s.aux_weight = aux_weight;
    return run_pass(s, caller);
}

int Learner::repr_forward_backward(const float* image, const float* road, const float* vehicle, const float* navigation,
                                   float temperature, float inv_world, hipStream_t caller) {
    PassSpec s{image, road, vehicle, navigation, nullptr, nullptr, nullptr, nullptr, inv_world};
    s.repr = true;
    s.temperature = temperature;
    return run_pass(s, caller);
}

int Learner::trunk_apply(hipStream_t caller) {
    if (frozen()) {
        set_error("trunk_apply: freeze_trunk = 1: the trunk has no optimizer step");
        return -1;
    }
    if (gate_on()) {
        set_error("trunk_apply: clip_mode = global / skip_nonfinite = 1: the gradient gate's decisions and counters are per head, a "
                  "trunk-only step has no place in them");
        return -1;
    }
    return launch(caller, {KEY_TRUNK_APPLY}, true, [&](hipStream_t st) -> int { return trunk_apply_impl(st); });
}

// order as in head_apply: the trunk's update (unclipped, not yet ticked), the tick behind it -- the chunk-norm kernel's
// tick on its own: a learner without train stats has no trunk chunk table, and this step needs no norm
int Learner::trunk_apply_impl(hipStream_t st) {
    const int opt = cfg_.optimizer;
    CDRL_TRY(clip_update(opt, 1.0f, arena_slice(M_TRUNK), ChunkTable{}, hp_dev_, WHICH_TRUNK, st));
    return tick_steps(hp_dev_, TICK_TRUNK | (opt == CDRL_OPT_NADAM ? TICK_NADAM : 0), st);
}

// the trainable slice of `model` in the four arenas
ArenaSlice Learner::arena_slice(int model) const {
    const int64_t o = tr_offset(model);
    return ArenaSlice{buf_.params + o, buf_.grads + o, buf_.adam_m + o, buf_.adam_v + o, tr_size_[model]};
}

int Learner::joint_apply(hipStream_t caller) {
    if (trust_on()) {
        set_error("joint_apply: cdrl_config.trust = 1: the trust-region latch gates policy_apply only, half of a joint apply has no gated form");
        return -1;
    }
    return launch(caller, {KEY_JOINT_APPLY}, true, [&](hipStream_t st) -> int { return joint_apply_impl(st); });
}

int Learner::joint_apply_impl(hipStream_t st) {
    // gated: trunk + policy head decided together (trunk list, policy list), then the value head from its own list, without the trunk
    if (gate_on()) {
        CDRL_TRY(gated_apply(0, st));
        return gated_apply(1, st, false);
    }
    // the value head without the trunk step and trunk tick: the trunk's optimizer steps once per joint step
    CDRL_TRY(head_apply(0, true, st));
    return head_apply(1, false, st);
}

int Learner::update_old_policy(hipStream_t caller) {
    return launch(caller, {}, false, [&](hipStream_t st) -> int { return update_old_policy_impl(st); });
}

int Learner::update_old_policy_impl(hipStream_t st, const GateBlock* gate) {
    // old_policy.set_weights(policy.get_weights()): all weights incl. BN moving statistics
    // (reference core/networks.py:281-285); gate: the copy of a gated apply, which a skipped step does not make
    return copy_two(buf_.params + tr_offset(M_OLD_POLICY), buf_.params + tr_offset(M_POLICY), tr_size_[M_POLICY],
                    buf_.params + st_offset(M_OLD_POLICY), buf_.params + st_offset(M_POLICY), st_size_[M_POLICY], st, gate);
}

int Learner::policy_apply(hipStream_t caller) {
    return launch(caller, {KEY_POLICY_APPLY}, true, [&](hipStream_t st) -> int { return policy_apply_impl(st); });
}

// The apply step of a learner with the gradient gate: chunk norms of the lists the step consumes -> gate (scales,
// skip flag, counter ticks) -> trunk update -> old_policy copy (policy) -> head update, the last three in their gated forms, which
// return at once when the gate said skip.  Both updates run behind the tick.  No host read: the sequence is capturable.
int Learner::gated_apply(int head, hipStream_t st, bool with_trunk) {
    const int hm = head == 0 ? M_POLICY : M_VALUE;
    const int opt = cfg_.optimizer;
    // (a trust learner in tensor mode without the guard: the head's per-tensor clip still wants its chunk partials)
    const int flags = (cfg_.clip_mode == CDRL_CLIP_GLOBAL ? GATE_GLOBAL : 0) | (cfg_.skip_nonfinite ? GATE_GUARD : 0) |
                      (frozen() || !with_trunk ? 0 : GATE_TRUNK) | (opt == CDRL_OPT_NADAM ? GATE_NADAM : 0) |
                      (cfg_.train_stats > 0 || (trust_on() && cfg_.clip_mode != CDRL_CLIP_GLOBAL) ? GATE_HEAD_PARTS : 0);
    const int mode = cfg_.clip_mode == CDRL_CLIP_GLOBAL ? GATE_MODE_GLOBAL : GATE_MODE_TENSOR;
    const ChunkTable &s = seg_[hm].dev, &t = seg_[M_TRUNK].dev;
    const ArenaSlice ha = arena_slice(hm), ta = arena_slice(M_TRUNK);
    CDRL_TRY(gate_chunk_sqnorms(ha.g, s, ta.g, t, hp_dev_, gate_dev_, head, flags, st));
    CDRL_TRY(gate_decide(s, t, hp_dev_, gate_dev_, head, flags, st, head == 0 ? trust_dev_ : nullptr));      // (the latch: policy only)
    if (!frozen() && with_trunk) CDRL_TRY(clip_update(opt, 1.0f, ta, ChunkTable{}, hp_dev_, WHICH_TRUNK, st, TICKED, gate_dev_, mode));
    if (head == 0) CDRL_TRY(update_old_policy_impl(st, gate_dev_));
    CDRL_TRY(clip_update(opt, cfg_.polyak, ha, s, hp_dev_, head, st, TICKED, gate_dev_, mode));
    return cfg_.train_stats > 0 ? stats_row(head, st) : 0;
}

// The ungated apply of one head (0 policy, 1 value).  with_trunk = false (the value head of a joint apply): no trunk step, no trunk tick.
// order: trunk Adam (unclipped, F9) -> clip -> old_policy <- policy -> policy Adam
// frozen trunk: no trunk Adam step, and the trunk's step counter stays where it is (reference ppo.py:238-252 on the heads only)
// (another cdrl_config.optimizer: its step in place of Adam's, same launches; polyak < 1: the head is averaged in its update)
int Learner::head_apply(int head, bool with_trunk, hipStream_t st) {
    const int hm = head == 0 ? M_POLICY : M_VALUE;
    const int opt = cfg_.optimizer;
    const bool trunk = with_trunk && !frozen();
    if (trunk) CDRL_TRY(clip_update(opt, 1.0f, arena_slice(M_TRUNK), ChunkTable{}, hp_dev_, WHICH_TRUNK, st));
    const ChunkTable& s = seg_[hm].dev;
    const ArenaSlice ha = arena_slice(hm);
    // four launches: the chunk kernel of the norms also advances the trunk's step counter (its update ran in front) and the head's (its
    // update runs behind and is told so); the per-tensor fold of the chunk partials happens inside the head's update kernel
    const int tick = (head == 0 ? TICK_POLICY : TICK_VALUE) | (trunk ? TICK_TRUNK : 0) | (opt == CDRL_OPT_NADAM ? TICK_NADAM : 0);
    CDRL_TRY(chunk_sqnorms_tick(ha.g, s, hp_dev_, tick, st));
    if (head == 0) CDRL_TRY(update_old_policy_impl(st));
    CDRL_TRY(clip_update(opt, cfg_.polyak, ha, s, hp_dev_, head, st, TICKED));
    return cfg_.train_stats > 0 ? stats_row(head, st) : 0;
}

int Learner::policy_apply_impl(hipStream_t st) { return gate_on() || trust_on() ? gated_apply(0, st) : head_apply(0, true, st); }
int Learner::value_apply_impl(hipStream_t st) { return gate_on() ? gated_apply(1, st) : head_apply(1, true, st); }

// Tail of an apply step with cfg.train_stats > 0: one ring row.  The gradients are read-only during the apply and the head's chunk
// partials (written by the clip path above, from the unclipped gradient) stay until the head's next apply, so this runs in order
// behind the updates: one extra read of the trunk gradient, a fold per tensor, the row writer.
int Learner::stats_row(int kind, hipStream_t st) {
    const int head = kind == 0 ? M_POLICY : M_VALUE;
    const ChunkTable &h = seg_[head].dev, &t = seg_[M_TRUNK].dev;      // (frozen trunk: it has no table, t is empty)
    CDRL_TRY(stats_chunk_sqnorms(arena_slice(M_TRUNK).g, t, st));
    CDRL_TRY(stats_fold_norms(stats_ring_, STATS_HEADER, stats_rows(), stats_width(), h, stats_off_norms(), t, stats_off_trunk(), st));
    StatsRowArgs a;
    a.ring = stats_ring_;
    a.header = STATS_HEADER;
    a.rows = stats_rows();
    a.width = stats_width();
    a.kind = kind;
    a.hp = hp_dev_;
    a.metrics = kind == 0 ? metrics_p_ : metrics_v_;
    a.lin = kind == 0 ? lin_p_.p : lin_v_.p;
    a.B = cfg_.B;
    a.ld = kind == 0 ? 2 * cfg_.A + 2 : 4;                  // policy: alpha, beta, similarity, speed; value: base, exp, speed, similarity
    a.col_speed = kind == 0 ? 2 * cfg_.A + 1 : 2;
    a.col_similarity = kind == 0 ? 2 * cfg_.A : 3;
    a.off_scalars = 0;
    a.off_metrics = STATS_SCALARS;
    a.off_norms = stats_off_norms();
    a.off_trunk = stats_off_trunk();
    a.n_head = h.ntensors;
    a.n_trunk = t.ntensors;
    return stats_write_row(a, st);
}

int Learner::stats_reset(hipStream_t caller) {
    if (!stats_ring_) {
        set_error("train stats are off (cdrl_config.train_stats = 0) or the learner is not bound");
        return -1;
    }
    return launch(caller, {}, false, [&](hipStream_t st) -> int { return stats_reset_ring(stats_ring_, st); });
}

int Learner::value_apply(hipStream_t caller) {
    return launch(caller, {KEY_VALUE_APPLY}, true, [&](hipStream_t st) -> int { return value_apply_impl(st); });
}

int Learner::predict(const float* image, const float* road, const float* vehicle, const float* navigation,
                     float* dist_out, float* value_out, float* dyn_out, hipStream_t caller) {
    std::vector<uint64_t> key = {KEY_PREDICT, K(image), K(road), K(vehicle), K(navigation), K(dist_out), K(value_out), K(dyn_out)};
    return launch(caller, key, true, [&](hipStream_t st) -> int {
        return predict_impl(image, road, vehicle, navigation, dist_out, value_out, dyn_out, st);
    });
}

int Learner::predict_impl(const float* image, const float* road, const float* vehicle, const float* navigation,
                          float* dist_out, float* value_out, float* dyn_out, hipStream_t st) {
    CDRL_TRY(set_inputs(image, road, vehicle, navigation));
    CDRL_TRY(run_trunk_fwd(st, 0));
    CDRL_TRY(run_fwd(old_policy_ops_, st, 0));
    CDRL_TRY(policy_dist(lin_old_.p, dist_out, cfg_.B, cfg_.A, st));
    CDRL_TRY(run_fwd(value_ops_, st, 0));
    CDRL_TRY(value_act(lin_v_.p, value_out, cfg_.B, cfg_.exp_scale, st));
    if (dyn_out)
        CDRL_HIP(hipMemcpyAsync(dyn_out, dyn_.p, (size_t)cfg_.B * cfg_.dyn * sizeof(float), hipMemcpyDeviceToDevice, st));
    tail_invalidate(st);
    return 0;
}

}  // namespace cdrl

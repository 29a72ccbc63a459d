// extern "C" surface of libcdrl_hip.so (declared in include/cdrl.h).
#include <stdlib.h>
#include <string.h>

#include <new>

#include "../../include/cdrl.h"
#include "engine.h"
#include "score_block.h"

using namespace cdrl;

struct cdrl_learner {
    Learner* impl;
};

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define CHECK_L(l)                         \
    if (!(l) || !(l)->impl) {              \
        cdrl::set_error("null learner");   \
        return -1;                         \
    }

// act_type of the op-level entry points below: element type of their ACTIVATION tensors -- 0 float32, 1 bf16 (configuration 3's storage)
static inline bool bad_act_type(int at) {
    if (at == 0 || at == 1) return false;
    cdrl::set_error("act_type: 0 (float32) or 1 (bf16)");
    return true;
}

// cdrl_policy_batch -> PolicyBatch.  need_u: the stored-action forms; the re-sampling forms ignore u / du_* (passed on as null)
static int policy_batch(const cdrl_policy_batch* b, bool need_u, const char* what, PolicyBatch* out) {
    if (!b) {
        cdrl::set_error("%s: null batch", what);
        return -1;
    }
    *out = PolicyBatch{b->image, b->road, b->vehicle, b->navigation, b->advantages, b->old_log_prob, b->speed, b->similarity,
                       need_u ? b->u : nullptr, need_u ? b->du_dalpha : nullptr, need_u ? b->du_dbeta : nullptr, b->anchor};
    if (!out->adv || !out->old_logp || !out->speed || !out->similarity || (need_u && !out->u)) {
        cdrl::set_error("%s: null tensor", what);
        return -1;
    }
    return 0;
}

// ... plus the returns of a joint pass
static int joint_batch(const cdrl_policy_batch* b, bool need_u, const float* returns, PolicyBatch* out) {
    CDRL_TRY(policy_batch(b, need_u, "joint batch", out));
    if (returns) return 0;
    cdrl::set_error("joint batch: null tensor");
    return -1;
}

extern "C" {

const char* cdrl_last_error(void) { return cdrl::last_error(); }
int cdrl_version(void) { return CDRL_VERSION; }
int cdrl_env_overrides(char* buf, int cap) { return cdrl::env_overrides(buf, cap); }
int cdrl_diag_active(void) { return cdrl::diag_active(); }

// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), slicing-by-8 on the host: checksums of the TF-checkpoint-V2
// writer (tf_checkpoint.py): every SSTable block and every tensor entry carries one
namespace {
struct Crc32cTable {
    uint32_t t[8][256];
    Crc32cTable() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int k = 1; k < 8; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xff];
    }
};
}  // namespace

uint32_t cdrl_crc32c(uint32_t crc, const void* data, size_t n) {
    // function-local static: initialised exactly once, thread-safe (ctypes releases the GIL around the call)
    static const Crc32cTable table;
    const uint32_t (*T)[256] = table.t;
    const unsigned char* p = static_cast<const unsigned char*>(data);
    uint32_t c = ~crc;
    while (n >= 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = T[7][lo & 0xff] ^ T[6][(lo >> 8) & 0xff] ^ T[5][(lo >> 16) & 0xff] ^ T[4][lo >> 24] ^ T[3][hi & 0xff] ^
            T[2][(hi >> 8) & 0xff] ^ T[1][(hi >> 16) & 0xff] ^ T[0][hi >> 24];
        p += 8;
        n -= 8;
    }
    while (n--) c = (c >> 8) ^ T[0][(c ^ *p++) & 0xff];
    return ~c;
}

void cdrl_config_default(cdrl_config* c) {
    if (!c) return;
    Config d;
    c->B = d.B; c->T = d.T; c->H = d.H; c->W = d.W;
    c->road = d.road; c->vehicle = d.vehicle; c->navigation = d.navigation; c->A = d.A;
    c->stem = d.stem;
    for (int i = 0; i < 3; ++i) { c->stage_c[i] = d.stage_c[i]; c->stage_n[i] = d.stage_n[i]; }
    c->last = d.last; c->feat = d.feat; c->rnn_image = d.rnn_image; c->rnn_small = d.rnn_small;
    c->dyn = d.dyn; c->head = d.head; c->exp_scale = d.exp_scale;
    c->compute = d.compute;
    c->freeze_trunk = d.freeze_trunk;
    c->optimizer = d.optimizer;
    c->polyak = d.polyak;
    c->train_stats = d.train_stats;
    c->clip_mode = d.clip_mode;
    c->skip_nonfinite = d.skip_nonfinite;
    c->trust = d.trust;
}

int cdrl_optimizer_slots(int optimizer, int32_t* used, float* init) {
    // {uses adam_m, uses adam_v, initial adam_m, initial adam_v} of every CDRL_OPT_* (include/cdrl.h table)
    static const float tab[8][4] = {{1, 1, 0.0f, 0.0f},     // adam: m, v
                                    {0, 0, 0.0f, 0.0f},     // sgd
                                    {0, 1, 0.0f, 0.0f},     // rmsprop: -, rms
                                    {0, 1, 0.0f, 0.1f},     // adagrad: -, accumulator (Keras initial_accumulator_value)
                                    {1, 1, 0.0f, 0.0f},     // adadelta: accum_var, accum_grad
                                    {1, 1, 0.0f, 0.0f},     // adamax: m, v
                                    {1, 1, 0.0f, 0.0f},     // nadam: m, v
                                    {1, 1, 0.0f, 0.1f}};    // ftrl: linear, accumulator (Keras initial_accumulator_value)
    if (optimizer < CDRL_OPT_ADAM || optimizer > CDRL_OPT_FTRL) {
        cdrl::set_error("cdrl_optimizer_slots: unknown optimizer %d", optimizer);
        return -1;
    }
    for (int i = 0; i < 2; ++i) {
        if (used) used[i] = (int32_t)tab[optimizer][i];
        if (init) init[i] = tab[optimizer][2 + i];
    }
    return 0;
}

int cdrl_learner_create(const cdrl_config* c, cdrl_learner** out) {
    if (!c || !out) {
        cdrl::set_error("cdrl_learner_create: null argument");
        return -1;
    }
    if (c->B < 1 || c->T < 1 || c->H < 35 || c->W < 35 || c->A < 1 || c->A > 8) {
        cdrl::set_error("cdrl_learner_create: bad geometry B=%d T=%d H=%d W=%d A=%d", c->B, c->T, c->H, c->W, c->A);
        return -1;
    }
    for (int i = 0; i < 3; ++i)
        if (c->stage_c[i] % 4 != 0 || c->stage_n[i] < 1) {
            cdrl::set_error("cdrl_learner_create: stage channels must be multiples of 4");
            return -1;
        }
    Config d;
    d.B = c->B; d.T = c->T; d.H = c->H; d.W = c->W;
    d.road = c->road; d.vehicle = c->vehicle; d.navigation = c->navigation; d.A = c->A;
    d.stem = c->stem;
    for (int i = 0; i < 3; ++i) { d.stage_c[i] = c->stage_c[i]; d.stage_n[i] = c->stage_n[i]; }
    d.last = c->last; d.feat = c->feat; d.rnn_image = c->rnn_image; d.rnn_small = c->rnn_small;
    d.dyn = c->dyn; d.head = c->head; d.exp_scale = c->exp_scale;
    if (c->compute != CDRL_COMPUTE_F32 && c->compute != CDRL_COMPUTE_BF16_OPERANDS && c->compute != CDRL_COMPUTE_BF16_STORAGE) {
        cdrl::set_error("cdrl_learner_create: unknown compute mode %d", c->compute);
        return -1;
    }
    d.compute = c->compute;
    if (c->freeze_trunk != 0 && c->freeze_trunk != 1) {
        cdrl::set_error("cdrl_learner_create: freeze_trunk must be 0 or 1 (got %d)", c->freeze_trunk);
        return -1;
    }
    d.freeze_trunk = c->freeze_trunk;
    if (c->optimizer < CDRL_OPT_ADAM || c->optimizer > CDRL_OPT_FTRL) {
        cdrl::set_error("cdrl_learner_create: unknown optimizer %d (CDRL_OPT_ADAM .. CDRL_OPT_FTRL)", c->optimizer);
        return -1;
    }
    d.optimizer = c->optimizer;
    if (!(c->polyak > 0.0f && c->polyak <= 1.0f)) {      // (NaN fails too)
        cdrl::set_error("cdrl_learner_create: polyak must be in (0, 1] (got %g)", (double)c->polyak);
        return -1;
    }
    d.polyak = c->polyak;
    if (c->train_stats < 0 || c->train_stats > (1 << 20)) {
        cdrl::set_error("cdrl_learner_create: train_stats must be 0 (off) or a row count up to 2^20 (got %d)", c->train_stats);
        return -1;
    }
    d.train_stats = c->train_stats;
    if (c->clip_mode != CDRL_CLIP_TENSOR && c->clip_mode != CDRL_CLIP_GLOBAL) {
        cdrl::set_error("cdrl_learner_create: clip_mode must be CDRL_CLIP_TENSOR (0) or CDRL_CLIP_GLOBAL (1) (got %d)", c->clip_mode);
        return -1;
    }
    d.clip_mode = c->clip_mode;
    if (c->skip_nonfinite != 0 && c->skip_nonfinite != 1) {
        cdrl::set_error("cdrl_learner_create: skip_nonfinite must be 0 or 1 (got %d)", c->skip_nonfinite);
        return -1;
    }
    d.skip_nonfinite = c->skip_nonfinite;
    if (c->trust != 0 && c->trust != 1) {
        cdrl::set_error("cdrl_learner_create: trust must be 0 or 1 (got %d)", c->trust);
        return -1;
    }
    d.trust = c->trust;
    if (cdrl::diag_active()) {      // loud, every time: results of this learner are WRONG by request (timing diagnostics)
        char ov[2048];
        cdrl::env_overrides(ov, (int)sizeof(ov));
        fprintf(stderr, "[cdrl] WARNING: CDRL_DIAG=1 with %d wrong-result diagnostic switch(es) active -- environment: %s\n",
                cdrl::diag_active(), ov);
    }
    cdrl_learner* l = new (std::nothrow) cdrl_learner;
    if (!l) return -3;
    l->impl = new (std::nothrow) Learner(d);
    if (!l->impl) {
        delete l;
        return -3;
    }
    if (!l->impl->build_error().empty()) {
        cdrl::set_error("cdrl_learner_create: %s", l->impl->build_error().c_str());
        delete l->impl;
        delete l;
        return -1;
    }
    *out = l;
    return 0;
}

void cdrl_learner_destroy(cdrl_learner* l) {
    if (!l) return;
    delete l->impl;
    delete l;
}

int cdrl_learner_param_count(const cdrl_learner* l, int model) {
    CHECK_L(l);
    if (model == CDRL_OLD_POLICY) model = CDRL_POLICY;
    if (model < 0 || model > 2) return -1;
    return (int)l->impl->params(model).size();
}

int cdrl_learner_param_info(const cdrl_learner* l, int model, int index, cdrl_param_info* out) {
    CHECK_L(l);
    if (model == CDRL_OLD_POLICY) model = CDRL_POLICY;
    if (model < 0 || model > 2 || !out) return -1;
    const auto& v = l->impl->params(model);
    if (index < 0 || index >= (int)v.size()) {
        cdrl::set_error("param index %d out of range", index);
        return -1;
    }
    const ParamInfo& p = v[index];
    memset(out, 0, sizeof(*out));
    strncpy(out->name, p.name.c_str(), sizeof(out->name) - 1);
    for (int i = 0; i < 4; ++i) out->shape[i] = p.shape[i];
    out->ndim = p.ndim;
    out->trainable = p.trainable;
    out->numel = p.numel;
    out->offset = p.off;
    return 0;
}

int64_t cdrl_learner_region_offset(const cdrl_learner* l, int model, int trainable) {
    CHECK_L(l);
    return trainable ? l->impl->tr_offset(model) : l->impl->st_offset(model);
}

int64_t cdrl_learner_region_elems(const cdrl_learner* l, int model, int trainable) {
    CHECK_L(l);
    if (model == CDRL_OLD_POLICY) model = CDRL_POLICY;
    return trainable ? l->impl->trainable_elems(model) : l->impl->state_elems(model);
}

int64_t cdrl_learner_params_total(const cdrl_learner* l) {
    CHECK_L(l);
    return l->impl->params_total();
}

int64_t cdrl_learner_grads_total(const cdrl_learner* l) {
    CHECK_L(l);
    return l->impl->grads_total();
}

size_t cdrl_learner_workspace_bytes(const cdrl_learner* l) {
    if (!l || !l->impl) return 0;
    return l->impl->workspace_bytes();
}

int cdrl_learner_bind(cdrl_learner* l, float* params, float* grads, float* adam_m, float* adam_v, void* workspace,
                      size_t workspace_bytes) {
    CHECK_L(l);
    Buffers b;
    b.params = params;
    b.grads = grads;
    b.adam_m = adam_m;
    b.adam_v = adam_v;
    b.workspace = workspace;
    b.workspace_bytes = workspace_bytes;
    return l->impl->bind(b);
}

int cdrl_learner_set_hparams(cdrl_learner* l, const cdrl_hparams* hp, void* stream) {
    CHECK_L(l);
    if (!hp) return -1;
    DevHP* h = l->impl->host_hp();
    h->lr_policy = hp->policy_lr;
    h->lr_value = hp->value_lr;
    h->lr_dynamics = hp->dynamics_lr;
    h->clip_ratio = hp->clip_ratio;
    h->entropy_coef = hp->entropy_coef;
    h->clip_norm_policy = hp->clip_norm_policy;
    h->clip_norm_value = hp->clip_norm_value;
    h->beta1 = hp->beta1;
    h->beta2 = hp->beta2;
    h->eps = hp->eps;
    l->impl->host_gate()->clip_norm_dynamics = hp->clip_norm_dynamics;
    return l->impl->upload_hp(S(stream));
}

int cdrl_learner_share_hparams(cdrl_learner* l, const cdrl_learner* owner) {
    CHECK_L(l);
    if (!owner || !owner->impl || !owner->impl->dev_hp() || !l->impl->dev_hp()) {
        cdrl::set_error("cdrl_learner_share_hparams: both learners must be bound");
        return -1;
    }
    const Config &a = l->impl->config(), &b = owner->impl->config();
    if (a.optimizer != b.optimizer || a.polyak != b.polyak) {      // one optimizer: its state and step counters must agree
        cdrl::set_error("cdrl_learner_share_hparams: optimizer / polyak differ (%d, %g vs the owner's %d, %g)", a.optimizer,
                        (double)a.polyak, b.optimizer, (double)b.polyak);
        return -1;
    }
    if (a.clip_mode != b.clip_mode || a.skip_nonfinite != b.skip_nonfinite) {      // one gate block: one decision per step
        cdrl::set_error("cdrl_learner_share_hparams: clip_mode / skip_nonfinite differ (%d, %d vs the owner's %d, %d)", a.clip_mode,
                        a.skip_nonfinite, b.clip_mode, b.skip_nonfinite);
        return -1;
    }
    if (a.trust != b.trust) {      // one trust block: one latch
        cdrl::set_error("cdrl_learner_share_hparams: trust differs (%d vs the owner's %d)", a.trust, b.trust);
        return -1;
    }
    if (a.train_stats > 0 && b.train_stats > 0 && (a.train_stats != b.train_stats || a.freeze_trunk != b.freeze_trunk)) {      // one ring: one layout
        cdrl::set_error("cdrl_learner_share_hparams: train_stats / freeze_trunk differ (%d, %d vs the owner's %d, %d)", a.train_stats,
                        a.freeze_trunk, b.train_stats, b.freeze_trunk);
        return -1;
    }
    l->impl->share_hp(*owner->impl);
    return 0;
}

int cdrl_learner_train_stats_layout(const cdrl_learner* l, cdrl_train_stats_layout* out) {
    CHECK_L(l);
    if (!out) return -1;
    const Learner& e = *l->impl;
    memset(out, 0, sizeof(*out));
    out->rows = e.stats_rows();
    if (out->rows <= 0) return 0;
    out->width = e.stats_width();
    out->header = Learner::STATS_HEADER;
    out->kind = STATS_KIND;
    out->t_head = STATS_T_HEAD;
    out->t_dynamics = STATS_T_DYNAMICS;
    out->lr = STATS_LR;
    out->lr_dynamics = STATS_LR_DYNAMICS;
    out->clip_ratio = STATS_CLIP_RATIO;
    out->entropy_coef = STATS_ENTROPY_COEF;
    out->speed = STATS_SPEED;
    out->similarity = STATS_SIMILARITY;
    out->metrics = Learner::STATS_SCALARS;
    out->norms = e.stats_off_norms();
    out->trunk_norms = e.stats_off_trunk();
    out->n_policy = e.stats_tensors(cdrl::M_POLICY);
    out->n_value = e.stats_tensors(cdrl::M_VALUE);
    out->n_trunk = e.stats_tensors(cdrl::M_TRUNK);
    return 0;
}

int cdrl_learner_train_stats_buffer(const cdrl_learner* l, void** ptr, int64_t* bytes) {
    CHECK_L(l);
    if (!ptr || !bytes) return -1;
    if (!l->impl->stats_ring()) {
        cdrl::set_error("cdrl_learner_train_stats_buffer: train stats are off (cdrl_config.train_stats = 0) or the learner is not bound");
        return -1;
    }
    *ptr = l->impl->stats_ring();
    *bytes = (int64_t)l->impl->stats_bytes();
    return 0;
}

int cdrl_learner_train_stats_reset(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    return l->impl->stats_reset(S(stream));
}

int cdrl_learner_gate_stats(const cdrl_learner* l, cdrl_gate_stats* out, void* stream) {
    CHECK_L(l);
    if (!out) {
        cdrl::set_error("cdrl_learner_gate_stats: null output");
        return -1;
    }
    if (!l->impl->gate_on()) {
        cdrl::set_error("cdrl_learner_gate_stats: the learner has neither clip_mode = CDRL_CLIP_GLOBAL nor skip_nonfinite = 1");
        return -1;
    }
    cdrl::GateBlock g;
    const int rc = l->impl->gate_stats(&g, S(stream));
    if (rc) return rc;
    for (int h = 0; h < 2; ++h) {
        out->skipped[h] = g.skipped[h], out->applied[h] = g.applied[h];
        out->norm[h] = g.last_norm[h][0], out->scale[h] = g.last_scale[h][0];
        out->norm_dynamics[h] = g.last_norm[h][1], out->scale_dynamics[h] = g.last_scale[h][1];
    }
    return 0;
}

int cdrl_learner_gate_reset(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    if (!l->impl->gate_on()) {
        cdrl::set_error("cdrl_learner_gate_reset: the learner has neither clip_mode = CDRL_CLIP_GLOBAL nor skip_nonfinite = 1");
        return -1;
    }
    return l->impl->gate_reset(S(stream));
}

int cdrl_learner_set_trust_params(cdrl_learner* l, const cdrl_trust_params* tp, void* stream) {
    CHECK_L(l);
    if (!tp) {
        cdrl::set_error("cdrl_learner_set_trust_params: null parameters");
        return -1;
    }
    if (!l->impl->trust_on()) {
        cdrl::set_error("cdrl_learner_set_trust_params: the learner was created without trust = 1");
        return -1;
    }
    // (NaN fails every comparison below)
    if (!(tp->target_kl >= 0.0f) || !(tp->kl_stop_factor > 0.0f) || !(tp->kl_coef >= 0.0f)) {
        cdrl::set_error("cdrl_learner_set_trust_params: target_kl = %g and kl_coef = %g must not be negative, kl_stop_factor = %g must be positive",
                        (double)tp->target_kl, (double)tp->kl_coef, (double)tp->kl_stop_factor);
        return -1;
    }
    cdrl::TrustBlock* t = l->impl->host_trust();
    t->target_kl = tp->target_kl;
    t->kl_stop_factor = tp->kl_stop_factor;
    t->kl_coef = tp->kl_coef;
    return l->impl->upload_trust(S(stream));
}

int cdrl_learner_trust_stats(const cdrl_learner* l, cdrl_trust_stats* out, void* stream) {
    CHECK_L(l);
    if (!out) {
        cdrl::set_error("cdrl_learner_trust_stats: null output");
        return -1;
    }
    if (!l->impl->trust_on()) {
        cdrl::set_error("cdrl_learner_trust_stats: the learner was created without trust = 1");
        return -1;
    }
    cdrl::TrustBlock t;
    const int rc = l->impl->trust_stats(&t, S(stream));
    if (rc) return rc;
    out->target_kl = t.target_kl, out->kl_stop_factor = t.kl_stop_factor, out->kl_coef = t.kl_coef;
    out->kl_last = t.kl_last, out->kl_max = t.kl_max;
    out->passes = t.passes, out->stop = t.stop, out->stop_pass = t.stop_pass, out->armed = t.armed, out->skipped = t.skipped;
    out->kl_sum = t.kl_sum;
    return 0;
}

int cdrl_learner_trust_reset(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    if (!l->impl->trust_on()) {
        cdrl::set_error("cdrl_learner_trust_reset: the learner was created without trust = 1");
        return -1;
    }
    return l->impl->trust_reset_block(S(stream));
}

int cdrl_learner_set_comm_stream(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    l->impl->set_comm_stream(S(stream));
    return 0;
}

int cdrl_learner_pw_signatures(const cdrl_learner* l, char* buf, int n) {
    if (!l || (!buf && n > 0)) return -1;
    std::string all;
    for (const std::string& r : l->impl->pw_signatures()) all += r + "\n";
    if (n > 0) snprintf(buf, (size_t)n, "%s", all.c_str());
    return (int)all.size() + 1;
}

int64_t cdrl_learner_tail_offset(const cdrl_learner* l) {
    if (!l) return -1;
    // with hipGraph replay the communication stream is never released mid-pass: no early bucket (everything is "tower")
    if (l->impl->graphs_enabled()) return l->impl->trainable_elems(cdrl::M_TRUNK);
    return l->impl->tail_offset();
}

int cdrl_learner_reset_optimizer_steps(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    return l->impl->reset_counters(S(stream));
}

int cdrl_learner_get_optimizer_state(const cdrl_learner* l, cdrl_optimizer_state* out, void* stream) {
    CHECK_L(l);
    if (!out) {
        cdrl::set_error("cdrl_learner_get_optimizer_state: null output");
        return -1;
    }
    int t[3];
    float mc[3];
    const int rc = l->impl->get_counters(t, mc, S(stream));
    if (rc) return rc;
    out->t_policy = t[0], out->t_value = t[1], out->t_dynamics = t[2];
    out->m_cache_policy = mc[0], out->m_cache_value = mc[1], out->m_cache_dynamics = mc[2];
    return 0;
}

int cdrl_learner_set_optimizer_state(cdrl_learner* l, const cdrl_optimizer_state* in, void* stream) {
    CHECK_L(l);
    if (!in) {
        cdrl::set_error("cdrl_learner_set_optimizer_state: null state");
        return -1;
    }
    const int t[3] = {in->t_policy, in->t_value, in->t_dynamics};
    const float mc[3] = {in->m_cache_policy, in->m_cache_value, in->m_cache_dynamics};
    return l->impl->set_counters(t, mc, S(stream));
}

int cdrl_learner_policy_forward_backward(cdrl_learner* l, const cdrl_policy_batch* b, float grad_scale, void* stream) {
    CHECK_L(l);
    PolicyBatch pb;
    CDRL_TRY(policy_batch(b, true, "policy batch", &pb));
    return l->impl->policy_forward_backward(pb, grad_scale, S(stream));
}

int cdrl_learner_policy_forward(cdrl_learner* l, const float* image, const float* road, const float* vehicle,
                                const float* navigation, void* stream) {
    CHECK_L(l);
    return l->impl->policy_forward(image, road, vehicle, navigation, S(stream));
}

int cdrl_learner_policy_backward(cdrl_learner* l, const cdrl_policy_batch* b, float grad_scale, void* stream) {
    CHECK_L(l);
    PolicyBatch pb;
    CDRL_TRY(policy_batch(b, true, "policy batch", &pb));
    return l->impl->policy_backward(pb, grad_scale, S(stream));
}

int cdrl_learner_policy_forward_backward_resample(cdrl_learner* l, const cdrl_policy_batch* b, uint64_t seed,
                                                 uint64_t offset, float grad_scale, void* stream) {
    CHECK_L(l);
    PolicyBatch pb;
    CDRL_TRY(policy_batch(b, false, "policy batch", &pb));
    return l->impl->policy_forward_backward_resample(pb, seed, offset, grad_scale, S(stream));
}

int cdrl_beta_sample_logp(const float* alpha, const float* beta, int rows, int A, int ld, uint64_t seed, uint64_t offset,
                          float* u, float* log_prob, void* stream) {
    if (!alpha || !beta || !u || !log_prob) {
        cdrl::set_error("cdrl_beta_sample_logp: null argument");
        return -1;
    }
    return beta_sample(alpha, beta, rows, A, ld, seed, offset, u, nullptr, nullptr, S(stream), log_prob);
}

int cdrl_beta_sample(const float* alpha, const float* beta, int rows, int A, int ld, uint64_t seed, uint64_t offset,
                     float* u, float* du_dalpha, float* du_dbeta, void* stream) {
    if (!alpha || !beta || !u) {
        cdrl::set_error("cdrl_beta_sample: null argument");
        return -1;
    }
    return beta_sample(alpha, beta, rows, A, ld, seed, offset, u, du_dalpha, du_dbeta, S(stream));
}

int cdrl_beta_act(const float* dist, const float* value, int rows, int A, int mode, uint64_t seed, uint64_t offset,
                  const int32_t* active, float* action, float* log_prob, double* stats, void* stream) {
    return beta_act(dist, value, rows, A, mode, seed, offset, active, action, log_prob, stats, S(stream));
}

int cdrl_gamma_implicit_grad(const double* a, const double* g, int n, double* out, void* stream) {
    return gamma_implicit_grad(a, g, n, out, S(stream));
}

int cdrl_beta_sample_gammas(const float* alpha, const float* beta, int rows, int A, int ld, uint64_t seed, uint64_t offset,
                            double* gammas, void* stream) {
    if (!alpha || !beta || !gammas) {
        cdrl::set_error("cdrl_beta_sample_gammas: null argument");
        return -1;
    }
    return beta_sample(alpha, beta, rows, A, ld, seed, offset, nullptr, nullptr, nullptr, S(stream), nullptr, gammas);
}

int cdrl_philox_words(uint64_t seed, uint64_t offset, uint64_t idx0, int n, int nblocks, uint32_t* out, void* stream) {
    if (!out) {
        cdrl::set_error("cdrl_philox_words: null output");
        return -1;
    }
    return philox_words(seed, offset, idx0, n, nblocks, out, S(stream));
}

int cdrl_learner_sequence_begin(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    return l->impl->sequence_begin(S(stream));
}

int cdrl_learner_sequence_end(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    return l->impl->sequence_end(S(stream));
}

int cdrl_learner_policy_apply(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    return l->impl->policy_apply(S(stream));
}

int cdrl_learner_value_forward_backward(cdrl_learner* l, const cdrl_value_batch* b, float grad_scale, void* stream) {
    CHECK_L(l);
    if (!b) return -1;
    ValueBatch vb{b->image, b->road, b->vehicle, b->navigation, b->returns, b->speed, b->similarity};
    if (!vb.returns || !vb.speed || !vb.similarity) {
        cdrl::set_error("value batch: null tensor");
        return -1;
    }
    return l->impl->value_forward_backward(vb, grad_scale, S(stream));
}

int cdrl_learner_value_apply(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    return l->impl->value_apply(S(stream));
}

int cdrl_learner_joint_forward_backward(cdrl_learner* l, const cdrl_policy_batch* b, const float* returns, float grad_scale,
                                       void* stream) {
    CHECK_L(l);
    PolicyBatch pb;
    CDRL_TRY(joint_batch(b, true, returns, &pb));
    return l->impl->joint_forward_backward(pb, returns, grad_scale, S(stream));
}

int cdrl_learner_joint_forward_backward_resample(cdrl_learner* l, const cdrl_policy_batch* b, const float* returns, uint64_t seed,
                                                uint64_t offset, float grad_scale, void* stream) {
    CHECK_L(l);
    PolicyBatch pb;
    CDRL_TRY(joint_batch(b, false, returns, &pb));
    return l->impl->joint_forward_backward_resample(pb, returns, seed, offset, grad_scale, S(stream));
}

int cdrl_learner_joint_apply(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    return l->impl->joint_apply(S(stream));
}

int cdrl_learner_clone_forward_backward(cdrl_learner* l, const cdrl_clone_batch* b, float policy_weight, float value_weight,
                                        float aux_weight, float grad_scale, void* stream) {
    CHECK_L(l);
    if (!b) {
        cdrl::set_error("clone batch: null batch");
        return -1;
    }
    if (!b->u) {
        cdrl::set_error("clone batch: null tensor (u)");
        return -1;
    }
    if (!b->speed != !b->similarity) {
        cdrl::set_error("clone batch: speed and similarity come together (both, or both null)");
        return -1;
    }
    if (b->returns && !b->speed) {
        cdrl::set_error("clone batch: returns need the speed and similarity targets (the value loss reads them)");
        return -1;
    }
    const CloneBatch cb{b->image, b->road, b->vehicle, b->navigation, b->u, b->weight, b->speed, b->similarity, b->returns};
    return l->impl->clone_forward_backward(cb, policy_weight, value_weight, aux_weight, grad_scale, S(stream));
}

static_assert(sizeof(cdrl_demo_stats) == sizeof(cdrl::DemoBlock), "cdrl_demo_stats mirrors DemoBlock");

int cdrl_learner_set_demo_block(cdrl_learner* l, cdrl_demo_stats* device_block) {
    CHECK_L(l);
    if (reinterpret_cast<uintptr_t>(device_block) % alignof(cdrl::DemoBlock) != 0) {
        cdrl::set_error("cdrl_learner_set_demo_block: the block must be 8-byte aligned");
        return -1;
    }
    l->impl->set_demo_block(reinterpret_cast<cdrl::DemoBlock*>(device_block));
    return 0;
}

int cdrl_learner_demo_forward_backward(cdrl_learner* l, const cdrl_policy_batch* b, const float* demo_u, const float* demo_w,
                                       float grad_scale, void* stream) {
    CHECK_L(l);
    PolicyBatch pb;
    CDRL_TRY(policy_batch(b, true, "demonstration batch", &pb));
    return l->impl->demo_forward_backward(pb, demo_u, demo_w, grad_scale, S(stream));
}

int cdrl_learner_demo_forward_backward_resample(cdrl_learner* l, const cdrl_policy_batch* b, const float* demo_u, const float* demo_w,
                                                uint64_t seed, uint64_t offset, float grad_scale, void* stream) {
    CHECK_L(l);
    PolicyBatch pb;
    CDRL_TRY(policy_batch(b, false, "demonstration batch", &pb));
    return l->impl->demo_forward_backward_resample(pb, demo_u, demo_w, seed, offset, grad_scale, S(stream));
}

int cdrl_learner_repr_forward_backward(cdrl_learner* l, const float* image, const float* road, const float* vehicle,
                                       const float* navigation, float temperature, float grad_scale, void* stream) {
    CHECK_L(l);
    if (!(temperature > 0.0f)) {
        cdrl::set_error("representation pass: temperature = %g must be positive", (double)temperature);
        return -1;
    }
    return l->impl->repr_forward_backward(image, road, vehicle, navigation, temperature, grad_scale, S(stream));
}

int cdrl_learner_trunk_apply(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    return l->impl->trunk_apply(S(stream));
}

int cdrl_learner_update_old_policy(cdrl_learner* l, void* stream) {
    CHECK_L(l);
    return l->impl->update_old_policy(S(stream));
}

int cdrl_learner_predict(cdrl_learner* l, const float* image, const float* road, const float* vehicle,
                         const float* navigation, float* dist_out, float* value_out, float* dynamics_out, void* stream) {
    CHECK_L(l);
    if (!dist_out || !value_out) return -1;
    return l->impl->predict(image, road, vehicle, navigation, dist_out, value_out, dynamics_out, S(stream));
}

int cdrl_learner_trunk_forward_train(cdrl_learner* l, const float* image, const float* road, const float* vehicle,
                                     const float* navigation, void* stream) {
    CHECK_L(l);
    return l->impl->trunk_forward_train(image, road, vehicle, navigation, S(stream));
}

int cdrl_learner_get_buffer(const cdrl_learner* l, int which, float** ptr, int64_t* elems) {
    CHECK_L(l);
    if (!ptr || !elems) return -1;
    const Config& c = l->impl->config();
    switch (which) {
        case CDRL_BUF_DYNAMICS: *ptr = l->impl->dyn_out(); *elems = (int64_t)c.B * c.dyn; break;
        case CDRL_BUF_IMG_FEAT: *ptr = l->impl->img_feat(); *elems = (int64_t)c.B * c.T * c.last; break;
        case CDRL_BUF_METRICS_P: *ptr = l->impl->metrics_policy(); *elems = 16; break;
        case CDRL_BUF_METRICS_V: *ptr = l->impl->metrics_value(); *elems = 16; break;
        case CDRL_BUF_AUX_P: *ptr = l->impl->policy_aux(); *elems = (int64_t)c.B * 4 * c.A; break;
        case CDRL_BUF_AUX_V: *ptr = l->impl->value_aux(); *elems = (int64_t)c.B * 2; break;
        case CDRL_BUF_LIN_P: *ptr = l->impl->policy_lin(); *elems = (int64_t)c.B * (2 * c.A + 2); break;
        case CDRL_BUF_LIN_V: *ptr = l->impl->value_lin(); *elems = (int64_t)c.B * 4; break;
        case CDRL_BUF_SAMPLE: *ptr = l->impl->sample_buffer(); *elems = (int64_t)c.B * c.A; break;
        case CDRL_BUF_METRICS_R: *ptr = l->impl->metrics_repr(); *elems = 16; break;
        default: cdrl::set_error("unknown buffer id %d", which); return -1;
    }
    return 0;
}

int cdrl_learner_named_buffer(const cdrl_learner* l, const char* name, void** ptr, int64_t* bytes) {
    CHECK_L(l);
    if (!name || !ptr || !bytes) return -1;
    if (!l->impl->named_buffer(name, ptr, bytes)) {
        cdrl::set_error("unknown named buffer %s (or learner not bound)", name);
        return -1;
    }
    return 0;
}

int cdrl_learner_check_guards(cdrl_learner* l, void* stream, int64_t* bad_bands, int64_t* first_bad_offset) {
    CHECK_L(l);
    return l->impl->check_guards(S(stream), bad_bands, first_bad_offset);
}

int cdrl_gae_returns(const float* rewards, const float* values_be, int N, double gamma, double lambda, float scale,
                     float* returns, float* returns_be, float* adv_raw, float* adv, double* scratch, void* stream) {
    if (!rewards || !values_be || !returns || !returns_be || !adv_raw || !adv || !scratch) {
        cdrl::set_error("cdrl_gae_returns: null argument");
        return -1;
    }
    return gae_returns(rewards, values_be, N, gamma, lambda, scale, returns, returns_be, adv_raw, adv, scratch, S(stream));
}

int64_t cdrl_gae_segments_scratch_doubles(int N, int nseg) {
    if (nseg < 1 || N < nseg) return 0;
    return 2 * ((int64_t)N + nseg);
}

int cdrl_gae_returns_segments(const float* rewards, const float* values_be, const int32_t* seg_off, int nseg, int N, double gamma,
                              double lambda, float scale, float* returns, float* returns_be, float* adv_raw, float* adv,
                              double* scratch, void* stream) {
    if (!rewards || !values_be || !seg_off || !returns || !returns_be || !adv_raw || !adv || !scratch) {
        cdrl::set_error("cdrl_gae_returns_segments: null argument");
        return -1;
    }
    if (nseg < 1) {
        cdrl::set_error("cdrl_gae_returns_segments: S = %d segments (at least one)", nseg);
        return -1;
    }
    if (N < nseg) {
        cdrl::set_error("cdrl_gae_returns_segments: N = %d rows for S = %d segments (every segment holds at least one row)", N, nseg);
        return -1;
    }
    if ((int64_t)N + nseg > INT32_MAX) {
        cdrl::set_error("cdrl_gae_returns_segments: N + S = %lld padded entries exceed the 32-bit row offsets", (long long)N + nseg);
        return -1;
    }
    return gae_returns_segments(rewards, values_be, seg_off, nseg, N, gamma, lambda, scale, returns, returns_be, adv_raw, adv, scratch,
                                S(stream));
}

int64_t cdrl_vtrace_segments_scratch_doubles(int N, int nseg) {
    if (nseg < 1 || N < nseg) return 0;
    return 4 * (int64_t)N;
}

int cdrl_vtrace_segments(const float* rewards, const float* values_be, const float* alpha, const float* beta, const float* actions,
                         const float* log_prob_old, const int32_t* seg_off, int nseg, int N, int A, double gamma, double lambda,
                         double rho_bar, double c_bar, float scale, float* returns, float* returns_be, float* adv_raw, float* adv,
                         float* rho, double* scratch, void* stream) {
    if (!rewards || !values_be || !alpha || !beta || !actions || !log_prob_old || !seg_off || !returns || !returns_be || !adv_raw || !adv
        || !rho || !scratch) {
        cdrl::set_error("cdrl_vtrace_segments: null argument");
        return -1;
    }
    if (nseg < 1) {
        cdrl::set_error("cdrl_vtrace_segments: S = %d segments (at least one)", nseg);
        return -1;
    }
    if (N < nseg) {
        cdrl::set_error("cdrl_vtrace_segments: N = %d rows for S = %d segments (every segment holds at least one row)", N, nseg);
        return -1;
    }
    if (A < 1 || A > 8) {
        cdrl::set_error("cdrl_vtrace_segments: A = %d actions (1..8)", A);
        return -1;
    }
    if ((int64_t)N + nseg > INT32_MAX) {
        cdrl::set_error("cdrl_vtrace_segments: N + S = %lld padded entries exceed the 32-bit row offsets", (long long)N + nseg);
        return -1;
    }
    if (!(rho_bar >= 0.0) || !(c_bar >= 0.0)) {
        cdrl::set_error("cdrl_vtrace_segments: rho_bar = %g, c_bar = %g (clips must not be negative)", rho_bar, c_bar);
        return -1;
    }
    return vtrace_segments(rewards, values_be, alpha, beta, actions, log_prob_old, seg_off, nseg, N, A, gamma, lambda, rho_bar, c_bar,
                           scale, returns, returns_be, adv_raw, adv, rho, scratch, S(stream));
}

int64_t cdrl_pwconv_x3_packed_bytes(int K) { return pw_x3_packed_bytes(K); }
int64_t cdrl_pwconv_x3_packed_bytes_n(int K, int N) { return pw_x3_packed_bytes_n(K, N); }
int cdrl_pwconv_x3_partial_rows(int G, int Mg, int N, int K) { return pw_x3_partial_rows(G, Mg, N, K); }

int cdrl_pwconv_x3_pack(const float* W, int K, int N, int sbk, int sbn, void* packed, void* stream) {
    if (!W || !packed) return -1;
    // one-entry table through a temporary device copy (test / tooling entry point; the engine packs all layers in one launch)
    PwX3Pack e = pw_x3_pack_entry(W, packed, K, N, sbk, sbn);
    PwX3Pack* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), sizeof(e)) != hipSuccess) return -2;
    int rc = hipMemcpy(d, &e, sizeof(e), hipMemcpyHostToDevice) == hipSuccess ? pw_x3_pack_many(d, 1, S(stream)) : -2;
    (void)hipStreamSynchronize(S(stream));
    (void)hipFree(d);
    return rc;
}

int cdrl_pwconv_x3(const float* A, int lda, int a_coff, const float* pro_stats, const void* W_packed, const float* bias, float* C,
                   int ldc, int c_coff, int G, int Mg, int N, int K, double* part, void* stream) {
    if (!A || !W_packed || !C) {
        cdrl::set_error("cdrl_pwconv_x3: null argument");
        return -1;
    }
    return pw_x3(make_view(const_cast<float*>(A), lda, a_coff), pro_stats, W_packed, bias, make_view(C, ldc, c_coff), G, Mg, N, K,
                 part, S(stream));
}

int cdrl_pwconv_x3_wide_bwd_rows(int Mg) { return pw_x3_wide_bwd_rows(Mg); }

int cdrl_pwconv_x3_wide_bwd(const float* dz, int ld_dz, int dz_coff, int dz_shuffle, int act, const float* y, const float* stats,
                            const float* coef, const void* W_packed, float* da, int ldda, int da_coff, int accumulate, int G, int Mg,
                            int Cin, int Cout, double* part2, const float* ey, const float* epi_stats, double* part, void* stream) {
    if (!dz || !y || !stats || !coef || !W_packed || !da) {
        cdrl::set_error("cdrl_pwconv_x3_wide_bwd: null argument");
        return -1;
    }
    PwBnBwd bb{y, stats, coef, dz_shuffle, act ? ACT_RELU6 : ACT_NONE, part2};
    return pw_x3_wide_bwd(make_view(const_cast<float*>(dz), ld_dz, dz_coff), bb, W_packed, make_view(da, ldda, da_coff), accumulate, G, Mg,
                          Cin, Cout, ey, epi_stats, part, S(stream));
}

int64_t cdrl_pwconv_bwd_fused_workspace(int G, int Mg, int N, int K, int which, int act_type) {
    return which == 0 ? pw_bwd_fused_qpart_elems(G, Mg, N, K, act_type) : pw_bwd_fused_dbpart_elems(G, Mg, N, K, act_type);
}

int cdrl_pwconv_bwd_fused(const float* dz, int ld_dz, int dz_coff, int dz_shuffle, int act, const float* y, const float* stats,
                          const float* coef, const float* a, int lda, int a_coff, const float* a_stats, const float* a_gamma,
                          const float* a_beta, float* a_dgamma, float* a_dbeta, float* a_coef, const float* W, const void* W_packed,
                          float* da, int ldda, int da_coff, int accumulate, float* dW, float* db, float* qpart, double* dbpart, int G,
                          int Mg, int N, int K, int act_type, void* stream) {
    if (!dz || !y || !stats || !coef || !a || !W || !W_packed || !da || !dW || !db || !qpart || !dbpart) {
        cdrl::set_error("cdrl_pwconv_bwd_fused: null argument");
        return -1;
    }
    PwBwdFused f;
    f.dz = make_view(const_cast<float*>(dz), ld_dz, dz_coff);
    f.dz_shuffle = dz_shuffle;
    f.act = act;
    f.y = y;
    f.stats = stats;
    f.coef = coef;
    f.a = make_view(const_cast<float*>(a), lda, a_coff);
    f.a_stats = a_stats;
    f.a_gamma = a_gamma;
    f.a_beta = a_beta;
    f.a_dgamma = a_dgamma;
    f.a_dbeta = a_dbeta;
    f.a_coef = a_coef;
    f.W = W;
    f.Wp = W_packed;
    f.da = make_view(da, ldda, da_coff);
    f.accumulate = accumulate;
    f.dW = dW;
    f.db = db;
    f.qpart = qpart;
    f.dbpart = dbpart;
    f.G = G;
    f.Mg = Mg;
    f.N = N;
    f.K = K;
    f.at = act_type;
    CDRL_TRY(pw_bwd_fused(f, S(stream)));
    return pw_bwd_fused_reduce(f, S(stream));
}

int64_t cdrl_gemm_x3_packed_bytes(int N, int K) { return gemm_x3_packed_bytes(N, K); }

int cdrl_gemm_x3_pack(const float* B, int K, int N, int sbk, int sbn, void* packed, void* stream) {
    if (!B || !packed) return -1;
    GemmX3Pack e = gemm_x3_pack_entry(B, packed, K, N, sbk, sbn);
    GemmX3Pack* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), sizeof(e)) != hipSuccess) return -2;      // tooling entry point; the engine packs in one launch
    int rc = hipMemcpy(d, &e, sizeof(e), hipMemcpyHostToDevice) == hipSuccess ? gemm_x3_pack_many(d, 1, S(stream)) : -2;
    (void)hipStreamSynchronize(S(stream));
    (void)hipFree(d);
    return rc;
}

int cdrl_gemm_x3(const float* A, int lda, int a_coff, const void* B_packed, const float* bias, float* C, int ldc, int c_coff, int M,
                 int N, int K, int accumulate, int act_type, void* stream) {
    if (!A || !B_packed || !C) {
        cdrl::set_error("cdrl_gemm_x3: null argument");
        return -1;
    }
    return gemm_x3(make_view(const_cast<float*>(A), lda, a_coff), B_packed, bias, make_view(C, ldc, c_coff), M, N, K, accumulate,
                   S(stream), act_type != 0, act_type);
}

int cdrl_f32_to_bf16(const float* x, void* y, int64_t n, void* stream) {
    if (!x || !y) return -1;
    return f32_to_bf16(x, y, n, S(stream));
}

int cdrl_bf16_to_f32(const void* x, float* y, int64_t n, void* stream) {
    if (!x || !y) return -1;
    return bf16_to_f32(x, y, n, S(stream));
}

int cdrl_pwconv_bf16_partial_rows(int G, int Mg, int N, int K) { return pw_bf16_partial_rows(G, Mg, N, K); }

int64_t cdrl_pwconv_bf16_packed_elems(int K) { return pw_bf16_packed_elems(K); }

int cdrl_pwconv_bf16_pack(const float* W, int K, int N, void* packed, void* stream) {
    if (!W || !packed) return -1;
    return pw_bf16_pack(W, K, N, packed, S(stream));
}

int cdrl_pwconv_bf16(const void* A, int lda, int a_coff, const float* pro_stats, const float* W, const void* W_packed,
                     const float* bias, void* C, int ldc, int c_coff, int G, int Mg, int N, int K, double* part, void* stream) {
    if (!A || (!W && !W_packed) || !C) {
        cdrl::set_error("cdrl_pwconv_bf16: null argument");
        return -1;
    }
    return pw_bf16(A, lda, a_coff, pro_stats, W, bias, C, ldc, c_coff, G, Mg, N, K, part, S(stream), W_packed);
}

int cdrl_gru_step_fwd(const float* xp, const float* hprev, const float* R, const float* b1, float* z, float* r, float* hh,
                      float* hp, float* hnew, int B, int u, void* stream) {
    if (!xp || !hprev || !R || !b1 || !z || !r || !hh || !hp || !hnew) {
        cdrl::set_error("cdrl_gru_step_fwd: null argument");
        return -1;
    }
    return gru_step_fwd(xp, hprev, R, b1, z, r, hh, hp, hnew, View{nullptr, 0, 0}, B, u, S(stream));
}

int cdrl_gru_step_bwd(const float* dh, int ld_dh, const float* z, const float* r, const float* hh, const float* hp,
                      const float* hprev, const float* RT, float* dxp, float* dhp, float* dhprev, int B, int u, void* stream) {
    if (!dh || !z || !r || !hh || !hp || !hprev || !RT || !dxp || !dhp) {
        cdrl::set_error("cdrl_gru_step_bwd: null argument");
        return -1;
    }
    return gru_step_bwd(make_view(const_cast<float*>(dh), ld_dh), z, r, hh, hp, hprev, RT, dxp, dhp, dhprev, B, u, S(stream));
}

int cdrl_gather_rows(const float* src, const int32_t* idx, float* dst, int nrows, int64_t row_elems, void* stream) {
    if (!src || !idx || !dst) {
        cdrl::set_error("cdrl_gather_rows: null argument");
        return -1;
    }
    return gather_rows(src, idx, dst, nrows, row_elems, S(stream));
}

int cdrl_gemm_nn(const float* A, int lda, int a_coff, const float* B, int sbk, int sbn, const float* bias, float* C,
                 int ldc, int c_coff, int M, int N, int K, int accumulate, void* stream) {
    const cdrl_view a{const_cast<float*>(A), lda, a_coff}, c{C, ldc, c_coff};
    return cdrl_gemm_nn_ex(&a, B, sbk, sbn, bias, &c, M, N, K, accumulate, nullptr, nullptr, 0, nullptr, stream);
}

int64_t cdrl_gemm_tn_workspace_elems(int M, int N, int K) { return gemm_tn_part_elems(M, N, K); }

int cdrl_gemm_tn(const float* A, int lda, int a_coff, const float* D, int ldd, int d_coff, float* out, int M, int N,
                 int K, float* workspace, int accumulate, int act_type, void* stream) {
    return gemm_tn(make_view(const_cast<float*>(A), lda, a_coff), make_view(const_cast<float*>(D), ldd, d_coff), out, M, N,
                   K, workspace, accumulate, S(stream), 1, nullptr, nullptr, act_type != 0, act_type);
}

int cdrl_stem_fwd(const float* x, const float* w, const float* bias, float* y, int B, int T, int H, int W, int Cout,
                  void* stream) {
    return stem_fwd(x, w, bias, y, B, T, H, W, Cout, S(stream));
}

int cdrl_stem_fwd_stats_rows(int B, int T, int H, int W, int Cout) { return stem_fwd_stats_nb(B, T, H, W, Cout); }

int cdrl_stem_fwd_stats(const float* x, const float* w, const float* bias, float* y, double* part, int B, int T, int H, int W, int Cout,
                        int act_type, void* stream) {
    return stem_fwd_stats(x, w, bias, y, part, B, T, H, W, Cout, S(stream), act_type);
}

int64_t cdrl_stem_bwd_workspace_doubles(int B, int T, int H, int W, int Cout) {
    return stem_bwd_part_elems(B, T, H, W, Cout);
}

int cdrl_stem_bwd_filter(const float* x, const float* dy, float* dw, float* db, int B, int T, int H, int W, int Cout,
                         double* workspace, void* stream) {
    return stem_bwd_filter(x, dy, dw, db, B, T, H, W, Cout, workspace, S(stream));
}

int cdrl_dwconv_fwd(const float* a, const float* w, const float* bias, float* y, int N, int H, int W, int C, int stride,
                    void* stream) {
    return dw_fwd(make_view(const_cast<float*>(a), C), w, bias, y, N, H, W, C, stride, S(stream));
}

int cdrl_dwconv_bwd_data(const float* dy, const float* w, float* da, int N, int H, int W, int C, int stride, void* stream) {
    return dw_bwd_data(dy, w, make_view(da, C), N, H, W, C, stride, 0, S(stream));
}

int64_t cdrl_dwconv_bwd_workspace_doubles(int N, int H, int W, int C, int stride) {
    return dw_bwd_part_elems(N, H, W, C, stride);
}

int cdrl_dwconv_bwd_filter(const float* a, const float* dy, float* dw, float* db, int N, int H, int W, int C, int stride,
                           double* workspace, void* stream) {
    return dw_bwd_filter(make_view(const_cast<float*>(a), C), dy, dw, db, N, H, W, C, stride, workspace, S(stream));
}

int64_t cdrl_augment_workspace_floats(int T, int H, int W) { return (int64_t)2 * T * H * W * 3 + 5 * T; }

int cdrl_augment_images(const float* in, float* out, int T, int H, int W, const cdrl_aug_plan* plan, float* workspace,
                        void* stream) {
    static_assert(sizeof(cdrl_aug_plan) == sizeof(AugPlan), "cdrl_aug_plan / AugPlan layout mismatch");
    if (!plan || in == out) {
        set_error("cdrl_augment_images: null plan or aliased in/out");
        return -1;
    }
    AugPlan p;
    memcpy(&p, plan, sizeof(p));
    return augment_images(in, out, T, H, W, p, workspace, S(stream));
}

int64_t cdrl_augment_batch_workspace_floats(int E, int T, int H, int W) { return augment_batch_workspace_floats(E, T, H, W); }

int cdrl_augment_images_batch(const float* in, float* out, int E, int T, int H, int W, const cdrl_aug_plan* plans_dev,
                              float* workspace, void* stream) {
    return augment_images_batch(in, out, E, T, H, W, reinterpret_cast<const AugPlan*>(plans_dev), workspace, S(stream));
}

int cdrl_occlusion_baseline(const float* image, float* baseline, int T, int H, int W, int mode, void* stream) {
    return occlusion_baseline(image, baseline, T, H, W, mode, S(stream));
}

int cdrl_occlusion_rows(const float* image, const float* baseline, const float* road, const float* vehicle, const float* navigation,
                        int T, int H, int W, int Dr, int Dv, int Dn, int gh, int gw, int per_frame, int modalities, int first,
                        int count, float* out_image, float* out_road, float* out_vehicle, float* out_navigation, void* stream) {
    const OcclusionRowsArgs a = {image, baseline, road, vehicle, navigation, out_image, out_road, out_vehicle, out_navigation,
                                 T, H, W, Dr, Dv, Dn, gh, gw, per_frame != 0, modalities != 0, first, count};
    return occlusion_rows(a, S(stream));
}

int cdrl_occlusion_scores(const float* alpha, const float* beta, const float* value, int N, int A, double* scores, void* stream) {
    return occlusion_scores(alpha, beta, value, N, A, scores, S(stream));
}

int cdrl_occlusion_maps(const double* scores, int K, int F, int gh, int gw, int H, int W, int upsample, int normalize, float* maps,
                        void* stream) {
    return occlusion_maps(scores, K, F, gh, gw, H, W, upsample, normalize, maps, S(stream));
}

int64_t cdrl_views_workspace_floats(int V, int T, int H, int W) { return views_workspace_floats(V, T, H, W); }

int cdrl_views_batch(const float* rows, int N, float* out, int V, int T, int H, int W, const cdrl_view_plan* plans_dev,
                     float* workspace, void* stream) {
    static_assert(sizeof(cdrl_view_plan) == sizeof(ViewPlan), "cdrl_view_plan / ViewPlan layout mismatch");
    return views_batch(rows, N, out, V, T, H, W, reinterpret_cast<const ViewPlan*>(plans_dev), workspace, S(stream));
}

int64_t cdrl_stem_block_bwd_workspace_doubles(int B, int T, int H, int W, int Cout) {
    const StemPlan sp = stem_plan(B, T, H, W, Cout, 0, false, false, true);
    return sp.pr_part_doubles + sp.ws_doubles;
}

int cdrl_stem_plan(int B, int T, int H, int W, int Cout, int act_type, int pooled, int db_adjacent, int y_aligned, int32_t* out, int n_out) {
    if (bad_act_type(act_type)) return -1;
    if (!out && n_out > 0) {
        cdrl::set_error("cdrl_stem_plan: no field array");
        return -1;
    }
    if (B < 1 || T < 1 || H < 3 || W < 3 || Cout < 1) {
        cdrl::set_error("cdrl_stem_plan: B %d, T %d, H %d, W %d, Cout %d: at least one frame of 3 x 3 pixels and one channel", B, T, H, W, Cout);
        return -1;
    }
    const StemPlan p = stem_plan(B, T, H, W, Cout, act_type, pooled != 0, db_adjacent != 0, y_aligned != 0);
    const int32_t v[] = {p.Ho, p.Wo, p.Hp, p.Wp, p.fwd_vec, p.st_refusal, p.st_form, p.R, p.NB, p.nbpg, p.px, p.NP, p.lds, p.units_max, p.part_rows,
                         p.pf.vec, p.pf.cx, p.pf.cy, p.pf.nloop, p.pf.rb, p.pf.nb, p.pr.form, p.pr.pooled, p.pr.g.nb, p.fg_form, p.ff_refusal, p.ff_form,
                         p.NCH, p.ff_rowstats, p.rows_per, p.nblk, p.slices_max, p.single_reduce, (int32_t)p.part_doubles, (int32_t)p.ws_doubles,
                         (int32_t)p.pr_part_doubles};
    int n = 0;
    for (int32_t x : v) {
        if (n < n_out) out[n] = x;
        ++n;
    }
    return n;
}

int cdrl_stem_block_bwd(const float* x, const float* y, const float* stats, const uint8_t* argmax, const float* dp, int B, int T,
                        int H, int W, int Cout, float* dgamma, float* dbeta, float* coef, float* dw, float* db,
                        double* workspace, int act_type, void* stream) {
    return cdrl_stem_block_bwd_pooled(x, y, stats, argmax, dp, nullptr, B, T, H, W, Cout, dgamma, dbeta, coef, dw, db, workspace, act_type, stream);
}

int cdrl_stem_block_bwd_pooled(const float* x, const float* y, const float* stats, const uint8_t* argmax, const float* dp,
                               const float* pooled, int B, int T, int H, int W, int Cout, float* dgamma, float* dbeta, float* coef,
                               float* dw, float* db, double* workspace, int act_type, void* stream) {
    const StemPlan sp = stem_plan(B, T, H, W, Cout, act_type, pooled != nullptr, db == dw + 27 * Cout, true);
    const int Ho = sp.Ho, Wo = sp.Wo;
    hipStream_t st = S(stream);
    PoolSrc ps = make_pool_src(argmax, dp, Ho, Wo);
    ps.pa = pooled;
    const int nb = sp.pr.g.nb;
    double* part = workspace;
    double* fpart = workspace + sp.pr_part_doubles;
    CDRL_TRY(pool_bn_bwd_reduce(ps, y, T, B, Cout, stats, part, st, act_type));
    CDRL_TRY(bn_bwd_finalize(part, nb, T, B * Ho * Wo, Cout, stats, dgamma, dbeta, coef, st));
    return stem_bwd_filter_fused(x, ps, y, stats, coef, dw, db, B, T, H, W, Cout, fpart, st, act_type);
}

int cdrl_pwconv_fused_partial_rows(int G, int Mg, int N, int K) { return pw_nn_shape_plan(G, Mg, N, K).nbpg; }

int cdrl_pwconv_fused(const float* a, int lda, int a_coff, const float* pro_stats, const float* w, int sbk, int sbn,
                      const float* bias, float* c, int ldc, int c_coff, int accumulate, int G, int Mg, int N, int K,
                      int epilogue, const float* epi_y, const float* epi_stats, double* part, void* stream) {
    return pw_nn(make_view(const_cast<float*>(a), lda, a_coff), pro_stats, w, sbk, sbn, bias, make_view(c, ldc, c_coff),
                 accumulate, G, Mg, N, K, epilogue, epi_y, epi_stats, part, S(stream));
}

int64_t cdrl_pwconv_pack_elems(int N, int K) { return pw_packed_elems(N, K); }

int cdrl_pwconv_pack(const float* W, int K, int N, int sbk, int sbn, float* packed, int bf16, void* stream) {
    if (!W || !packed) return -1;
    // one-entry table through a temporary device copy (test / tooling entry point; the engine packs all layers in one launch)
    PwPack e = pw_pack_entry(W, packed, K, N, sbk, sbn, bf16 != 0);
    PwPack* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), sizeof(e)) != hipSuccess) return -2;
    int rc = hipMemcpy(d, &e, sizeof(e), hipMemcpyHostToDevice) == hipSuccess ? pw_pack_many(d, 1, S(stream)) : -2;
    (void)hipStreamSynchronize(S(stream));
    (void)hipFree(d);
    return rc;
}

int cdrl_pwconv_fused_packed(const float* a, int lda, int a_coff, const float* pro_stats, const float* w, int sbk, int sbn,
                             const float* bias, float* c, int ldc, int c_coff, int accumulate, int G, int Mg, int N, int K,
                             int epilogue, const float* epi_y, const float* epi_stats, double* part, const float* w_packed,
                             int packed_bf16, int act_type, void* stream) {
    if (!w_packed) {
        cdrl::set_error("cdrl_pwconv_fused_packed: null packed weights");
        return -1;
    }
    return pw_nn(make_view(const_cast<float*>(a), lda, a_coff), pro_stats, w, sbk, sbn, bias, make_view(c, ldc, c_coff),
                 accumulate, G, Mg, N, K, epilogue, epi_y, epi_stats, part, S(stream), nullptr, w_packed, packed_bf16 != 0, act_type);
}

static int64_t al256(int64_t x) { return (x + 255) / 256 * 256; }

int64_t cdrl_pwconv_bn_bwd_workspace_bytes(int G, int Mg, int N, int K) {
    const int64_t nbr = vcol_geom(Mg, N).nb, nbp = std::max(pw_nn_shape_plan(G, Mg, K, N).nbpg, pw_x3_wide_bwd_rows(Mg));
    return al256((int64_t)G * nbr * 2 * N * 8) + al256((int64_t)G * nbp * N * 8) + al256(gemm_tn_part_elems(G * Mg, N, K, G) * 4);
}

static int pwconv_bn_bwd_impl(const float* dout, int dout_ld, int dout_coff, int shuffle_ctot, int relu6, const float* y,
                              const float* stats, const float* x, int x_ld, int x_coff, const float* x_pro_stats, const float* w,
                              int G, int Mg, int N, int K, float* dgamma, float* dbeta, float* coef, float* dx, int dx_ld,
                              int dx_coff, int accumulate, float* dw, float* db, void* workspace, const float* wt_packed,
                              int packed_bf16, int act_type, void* stream) {
    hipStream_t st = S(stream);
    const int act = relu6 ? ACT_RELU6 : ACT_NONE;
    View vd = make_view(const_cast<float*>(dout), dout_ld, dout_coff), vy = make_view(const_cast<float*>(y), N);
    View vx = make_view(const_cast<float*>(x), x_ld, x_coff);
    // dx[m,k] = sum_n dy[m,n] W[k,n]: GEMM with "K" = N (reduction over the conv outputs) and "N" = K
    const View vdx = make_view(dx, dx_ld, dx_coff);
    const PwX3BwdPlan xb = pw_x3_wide_bwd_plan(vd, vdx, G, Mg, K, N, shuffle_ctot, false, accumulate, true);
    const int nbr = vcol_geom(Mg, N).nb, nbp = pw_nn_shape_plan(G, Mg, K, N).nbpg;
    char* ws = static_cast<char*>(workspace);
    double* part = reinterpret_cast<double*>(ws);
    ws += al256((int64_t)G * nbr * 2 * N * 8);
    double* part2 = reinterpret_cast<double*>(ws);
    ws += al256((int64_t)G * std::max(nbp, xb.rows) * N * 8);
    float* tn = reinterpret_cast<float*>(ws);
    CDRL_TRY(bn_bwd_reduce(vd, shuffle_ctot, vy, G, Mg, N, stats, act, part, st, nullptr, nullptr, nullptr, 0, act_type));
    CDRL_TRY(bn_bwd_finalize(part, nbr, G, Mg, N, stats, dgamma, dbeta, coef, st));
    PwBnBwd bb{y, stats, coef, shuffle_ctot, act, part2};
    if (!act_type && !packed_bf16 && xb.ok) {
        // 232-channel shapes, float32: the one-tile-per-workgroup split-precision kernel the engine runs (gemm_pw_x3.hip); the packed
        // operand is built here through a temporary device buffer (test / tooling entry point)
        void* wp = nullptr;
        PwX3Pack* d = nullptr;
        if (hipMalloc(&wp, (size_t)pw_x3_packed_bytes_n(N, K)) != hipSuccess) return -2;
        if (hipMalloc(reinterpret_cast<void**>(&d), sizeof(PwX3Pack)) != hipSuccess) {
            (void)hipFree(wp);
            return -2;
        }
        PwX3Pack e = pw_x3_pack_entry(w, wp, N, K, 1, N);
        int rc = hipMemcpy(d, &e, sizeof(e), hipMemcpyHostToDevice) == hipSuccess ? pw_x3_pack_many(d, 1, st) : -2;
        if (rc == 0) rc = pw_x3_wide_bwd(vd, bb, wp, vdx, accumulate, G, Mg, K, N, nullptr, nullptr, nullptr, st);
        if (rc == 0) rc = reduce_partials(part2, G * xb.rows, N, N, db, 0, st);
        (void)hipStreamSynchronize(st);
        (void)hipFree(d);
        (void)hipFree(wp);
        if (rc != 0) return rc;
    } else {
        CDRL_TRY(pw_nn(vd, nullptr, w, 1, N, nullptr, vdx, accumulate, G, Mg, K, N, 0, nullptr, nullptr, nullptr,
                       st, &bb, wt_packed, packed_bf16 != 0, act_type));
        CDRL_TRY(reduce_partials(part2, G * nbp, N, N, db, 0, st));
    }
    TnBnBwd tb{y, stats, coef, shuffle_ctot, act};
    return gemm_tn(vx, vd, dw, G * Mg, N, K, tn, 0, st, G, x_pro_stats, &tb, wt_packed && packed_bf16 != 0, act_type);
}

int cdrl_pwconv_bn_bwd(const float* dout, int dout_ld, int dout_coff, int shuffle_ctot, int relu6, const float* y,
                       const float* stats, const float* x, int x_ld, int x_coff, const float* x_pro_stats, const float* w,
                       int G, int Mg, int N, int K, float* dgamma, float* dbeta, float* coef, float* dx, int dx_ld,
                       int dx_coff, int accumulate, float* dw, float* db, void* workspace, int act_type, void* stream) {
    return pwconv_bn_bwd_impl(dout, dout_ld, dout_coff, shuffle_ctot, relu6, y, stats, x, x_ld, x_coff, x_pro_stats, w, G, Mg, N, K,
                              dgamma, dbeta, coef, dx, dx_ld, dx_coff, accumulate, dw, db, workspace, nullptr, 0, act_type, stream);
}

int cdrl_pwconv_bn_bwd_packed(const float* dout, int dout_ld, int dout_coff, int shuffle_ctot, int relu6, const float* y,
                              const float* stats, const float* x, int x_ld, int x_coff, const float* x_pro_stats, const float* w,
                              int G, int Mg, int N, int K, float* dgamma, float* dbeta, float* coef, float* dx, int dx_ld,
                              int dx_coff, int accumulate, float* dw, float* db, void* workspace, const float* wt_packed,
                              int packed_bf16, int act_type, void* stream) {
    if (!wt_packed) {
        cdrl::set_error("cdrl_pwconv_bn_bwd_packed: null packed weights");
        return -1;
    }
    return pwconv_bn_bwd_impl(dout, dout_ld, dout_coff, shuffle_ctot, relu6, y, stats, x, x_ld, x_coff, x_pro_stats, w, G, Mg, N, K,
                              dgamma, dbeta, coef, dx, dx_ld, dx_coff, accumulate, dw, db, workspace, wt_packed, packed_bf16, act_type, stream);
}

int64_t cdrl_dwconv_bn_workspace_doubles(int G, int B, int H, int W, int C, int stride) {
    const DwfPlan p = dwf_plan(B, G, H, W, C, stride);
    if (p.fwd.refusal == DWF_REFUSE_STRIDE) return 0;
    const int64_t nb_out = vcol_geom(B * p.Ho * p.Wo, C).nb, nb_in = vcol_geom(B * H * W, C).nb;
    const int64_t nbm = nb_out > nb_in ? nb_out : nb_in;
    return p.stats_part_elems + p.filter_part_elems + (int64_t)G * nbm * 3 * C;
}

// the plan as plain numbers, field order in include/cdrl.h: nothing here decides anything.  cdrl_dwconv_bn_plan reports the first
// `count` = 22 of them (its callers size their arrays by that count), cdrl_dwconv_bn_plan_ex all of them.
static int dwconv_bn_plan_fields(int G, int B, int H, int W, int C, int stride, int32_t* out, int n_out, int count) {
    if (stride != 1 && stride != 2) return dwf_refuse("dwf_plan", DwfPlan(), DWF_REFUSE_STRIDE);
    if (G < 1 || B < 1 || H < 1 || W < 1 || C < 1 || (!out && n_out > 0)) {
        cdrl::set_error("dwf_plan: bad shape %dx%dx%dx%dx%d or null output", G, B, H, W, C);
        return -1;
    }
    const DwfPlan p = dwf_plan(B, G, H, W, C, stride);
    const DwsGeom& d = p.strip;
    const int32_t v[] = {p.vec, p.nch, p.cchunk, p.cy, p.fpb, p.nb, p.vec_bwd, p.fpb_bwd, p.nb_bwd, p.bwd.form, d.sw, d.R, d.F, d.nch, d.cy,
                         same_pad_before(W, 2),        // (= p.pl, the PL of form 2, for stride 2; reported for stride 1 as well)
                         p.lds_bwd_over, p.fwd.refusal == DWF_REFUSE_LDS, p.cx, p.cx_bwd, p.cy_bwd, d.cx,
                         d.cchunk, d.S, (int32_t)p.fwd.lds, (int32_t)p.bwd.lds, p.fwd.grid, p.bwd.grid, d.tile_floats * (int32_t)sizeof(float),
                         p.fwd.refusal, p.bwd.refusal};
    int n = 0;
    for (int32_t x : v) {
        if (n == count) break;
        if (n < n_out) out[n] = x;
        ++n;
    }
    return n;
}

int cdrl_dwconv_bn_plan(int G, int B, int H, int W, int C, int stride, int32_t* out, int n_out) {
    return dwconv_bn_plan_fields(G, B, H, W, C, stride, out, n_out, 22);
}

int cdrl_dwconv_bn_plan_ex(int G, int B, int H, int W, int C, int stride, int32_t* out, int n_out) {
    return dwconv_bn_plan_fields(G, B, H, W, C, stride, out, n_out, 1 << 30);
}

int cdrl_dwconv_bn_fwd(const float* x, const float* pre_stats, const float* w, const float* bias, float* y, int G, int B,
                       int H, int W, int C, int stride, const float* gamma, const float* beta, float* moving_mean,
                       float* moving_var, int bessel, float* post_stats, double* workspace, int act_type, void* stream) {
    const DwfPlan p = dwf_plan(B, G, H, W, C, stride);
    CDRL_TRY(dwf_fwd(p, DwfFwdArgs{x, pre_stats, w, bias, y, workspace, S(stream), act_type}));
    return bn_finalize(workspace, p.nb, G, B * p.Ho * p.Wo, C, gamma, beta, moving_mean, moving_var, bessel, 1, post_stats, S(stream));
}

int cdrl_dwconv_bn_bwd(const float* x, const float* pre_stats, const float* dout, const float* y, const float* post_stats,
                       const float* w, int G, int B, int H, int W, int C, int stride, float* dx, float* dw, float* db,
                       float* dgamma_post, float* dbeta_post, float* coef_post, float* dgamma_pre, float* dbeta_pre,
                       float* coef_pre, double* workspace, int act_type, void* stream) {
    const DwfPlan p = dwf_plan(B, G, H, W, C, stride);
    if (p.bwd.refusal == DWF_REFUSE_STRIDE) return dwf_refuse("dwf_bwd", p, p.bwd.refusal);
    const int Mo = B * p.Ho * p.Wo, Mi = B * H * W;
    double* part_bn = workspace;
    double* part_w = part_bn + p.stats_part_elems;
    double* part_r = part_w + p.filter_part_elems;
    hipStream_t st = S(stream);
    View vd = make_view(const_cast<float*>(dout), C), vy = make_view(const_cast<float*>(y), C);
    CDRL_TRY(bn_bwd_reduce(vd, 0, vy, G, Mo, C, post_stats, ACT_NONE, part_r, st, nullptr, nullptr, nullptr, 0, act_type));
    CDRL_TRY(bn_bwd_finalize(part_r, vcol_geom(Mo, C).nb, G, Mo, C, post_stats, dgamma_post, dbeta_post, coef_post, st));
    CDRL_TRY(dwf_bwd(p, DwfBwdArgs{x, pre_stats, dout, y, post_stats, coef_post, w, make_view(dx, C), part_bn, part_w, st, act_type}));
    CDRL_TRY(reduce_partials(part_w, G * p.nb_bwd, 9 * C, (int64_t)10 * C, dw, 0, st));
    CDRL_TRY(reduce_partials(part_w + 9 * C, G * p.nb_bwd, C, (int64_t)10 * C, db, 0, st));
    if (pre_stats) {
        CDRL_TRY(bn_bwd_finalize(part_bn, p.nb_bwd, G, Mi, C, pre_stats, dgamma_pre, dbeta_pre, coef_pre, st));
        View vx = make_view(const_cast<float*>(x), C);
        CDRL_TRY(bn_bwd_apply(make_view(dx, C), 0, vx, G, Mi, C, pre_stats, coef_pre, ACT_NONE, dx, part_r, st, nullptr, 0, act_type));
    }
    return 0;
}

int cdrl_maxpool_fwd(const float* a, float* p, uint8_t* argmax, int N, int H, int W, int C, void* stream) {
    return maxpool_fwd(a, p, argmax, N, H, W, C, S(stream));
}

int cdrl_maxpool_bwd(const uint8_t* argmax, const float* dp, float* da, int N, int H, int W, int C, void* stream) {
    return maxpool_bwd(argmax, dp, da, N, H, W, C, S(stream));
}

int cdrl_bn_train_fwd(const float* y, int G, int Mg, int C, const float* gamma, const float* beta, float* moving_mean,
                      float* moving_var, int bessel, int relu6, float* out, int out_ld, int out_coff, int shuffle_ctot,
                      float* stats, double* workspace, int act_type, void* stream) {
    View yv = make_view(const_cast<float*>(y), C);
    const int nb = vcol_geom(Mg, C).nb;
    CDRL_TRY(colstats(yv, G, Mg, C, workspace, S(stream), act_type));
    CDRL_TRY(bn_finalize(workspace, nb, G, Mg, C, gamma, beta, moving_mean, moving_var, bessel, 1, stats, S(stream)));
    return bn_apply(yv, G, Mg, C, stats, relu6 ? ACT_RELU6 : ACT_NONE, make_view(out, out_ld, out_coff), shuffle_ctot,
                    S(stream), nullptr, nullptr, act_type);
}

int cdrl_bn_train_bwd(const float* dout, int dout_ld, int dout_coff, int shuffle_ctot, const float* y, int G, int Mg,
                      int C, const float* stats, int relu6, float* dgamma, float* dbeta, float* dy, float* coef,
                      double* workspace, int act_type, void* stream) {
    View yv = make_view(const_cast<float*>(y), C);
    View dv = make_view(const_cast<float*>(dout), dout_ld, dout_coff);
    const int nb = vcol_geom(Mg, C).nb;
    const int act = relu6 ? ACT_RELU6 : ACT_NONE;
    CDRL_TRY(bn_bwd_reduce(dv, shuffle_ctot, yv, G, Mg, C, stats, act, workspace, S(stream), nullptr, nullptr, nullptr, 0, act_type));
    CDRL_TRY(bn_bwd_finalize(workspace, nb, G, Mg, C, stats, dgamma, dbeta, coef, S(stream)));
    return bn_bwd_apply(dv, shuffle_ctot, yv, G, Mg, C, stats, coef, act, dy, workspace, S(stream), nullptr, 0, act_type);
}

// ---- BatchNorm family at op level with the argument forms the engine uses (full views, identity pass-through, pooled gradient) ----
static inline View view_of(const cdrl_view* v) {
    View r{nullptr, 0, 0};
    if (v) r = make_view(static_cast<float*>(v->p), v->ld, v->coff);
    return r;
}

// columns [coff, coff + C) of a view, plain or through the shuffle map of a ctot-channel tensor, stay inside a row
static bool view_ok(const char* fn, const char* name, const cdrl_view* v, int C, int shuffle_ctot) {
    const bool ok = v && v->p && v->coff >= 0 &&
                    (shuffle_ctot ? (shuffle_ctot % 2 == 0 && v->coff + C <= shuffle_ctot && shuffle_ctot <= v->ld) : v->coff + C <= v->ld);
    if (!ok) cdrl::set_error("%s: view %s is null or its %d channels (shuffle %d) do not fit its rows", fn, name, C, shuffle_ctot);
    return ok;
}

static bool bn_args_ok(const char* fn, int G, int Mg, int C, int shuffle_ctot, int bcast_rows, bool pass_a, bool pass_b, int at) {
    if (bad_act_type(at)) return false;
    if (G < 1 || Mg < 1 || C < 1 || shuffle_ctot < 0 || bcast_rows < 0 || pass_a != pass_b ||
        (bcast_rows && (Mg % bcast_rows != 0 || shuffle_ctot || pass_a))) {
        cdrl::set_error("%s: bad shape G %d Mg %d C %d, shuffle %d, bcast_rows %d, or half a pass-through pair", fn, G, Mg, C, shuffle_ctot, bcast_rows);
        return false;
    }
    return true;
}

int cdrl_bn_apply(const cdrl_view* y, int G, int Mg, int C, const float* stats, int relu6, const cdrl_view* out, int shuffle_ctot,
                  const cdrl_view* pass_src, const cdrl_view* pass_dst, int act_type, void* stream) {
    if (!bn_args_ok("cdrl_bn_apply", G, Mg, C, shuffle_ctot, 0, pass_src != nullptr, pass_dst != nullptr, act_type)) return -1;
    if (!view_ok("cdrl_bn_apply", "y", y, C, 0) || !view_ok("cdrl_bn_apply", "out", out, C, shuffle_ctot)) return -1;
    if (pass_src && (!view_ok("cdrl_bn_apply", "pass_src", pass_src, C, 0) || !view_ok("cdrl_bn_apply", "pass_dst", pass_dst, C, shuffle_ctot)))
        return -1;
    if (!stats && (act_type || relu6)) {
        cdrl::set_error("cdrl_bn_apply: the copy form (stats = NULL) is float32 without activation");
        return -1;
    }
    const View ps = view_of(pass_src), pd = view_of(pass_dst);
    return bn_apply(view_of(y), G, Mg, C, stats, relu6 ? ACT_RELU6 : ACT_NONE, view_of(out), shuffle_ctot, S(stream),
                    pass_src ? &ps : nullptr, pass_dst ? &pd : nullptr, act_type);
}

int cdrl_bn_bwd(const cdrl_view* dout, int shuffle_ctot, const cdrl_view* y, int G, int Mg, int C, const float* stats, int relu6,
                float* dgamma, float* dbeta, float* dy, float* coef, double* workspace, const cdrl_view* pass_gsrc,
                const cdrl_view* pass_gdst, int bcast_rows, int act_type, void* stream) {
    if (!bn_args_ok("cdrl_bn_bwd", G, Mg, C, shuffle_ctot, bcast_rows, pass_gsrc != nullptr, pass_gdst != nullptr, act_type)) return -1;
    if (!view_ok("cdrl_bn_bwd", "dout", dout, C, shuffle_ctot) || !view_ok("cdrl_bn_bwd", "y", y, C, 0)) return -1;
    if (pass_gsrc && (!view_ok("cdrl_bn_bwd", "pass_gsrc", pass_gsrc, C, shuffle_ctot) || !view_ok("cdrl_bn_bwd", "pass_gdst", pass_gdst, C, 0)))
        return -1;
    const View dv = view_of(dout), yv = view_of(y), pgs = view_of(pass_gsrc), pgd = view_of(pass_gdst);
    const int nb = vcol_geom(Mg, C).nb;
    const int act = relu6 ? ACT_RELU6 : ACT_NONE;
    double* part2 = workspace + (int64_t)G * nb * 2 * C;
    hipStream_t st = S(stream);
    CDRL_TRY(bn_bwd_reduce(dv, shuffle_ctot, yv, G, Mg, C, stats, act, workspace, st, nullptr, pass_gsrc ? &pgs : nullptr,
                           pass_gdst ? &pgd : nullptr, bcast_rows, act_type));
    CDRL_TRY(bn_bwd_finalize(workspace, nb, G, Mg, C, stats, dgamma, dbeta, coef, st));
    return bn_bwd_apply(dv, shuffle_ctot, yv, G, Mg, C, stats, coef, act, dy, part2, st, nullptr, bcast_rows, act_type);
}

int cdrl_bn_plan(const cdrl_view* y, const cdrl_view* out, const cdrl_view* dout, int shuffle_ctot, int G, int Mg, int C, int has_stats,
                 int relu6, const cdrl_view* pass_src, const cdrl_view* pass_dst, const cdrl_view* pass_gsrc, const cdrl_view* pass_gdst,
                 const float* dy, int bcast_rows, int act_type, int32_t* fields, int n_out) {
    if (!bn_args_ok("cdrl_bn_plan", G, Mg, C, shuffle_ctot, bcast_rows, pass_src != nullptr, pass_dst != nullptr, act_type)) return -1;
    if (!y || !out || !dout || (pass_gsrc != nullptr) != (pass_gdst != nullptr) || (!fields && n_out > 0)) {
        cdrl::set_error("cdrl_bn_plan: y, out and dout views are required, pass-through views come in pairs");
        return -1;
    }
    const View ps = view_of(pass_src), pd = view_of(pass_dst), pgs = view_of(pass_gsrc), pgd = view_of(pass_gdst);
    const BnPlan plans[3] = {
        bn_apply_plan(view_of(y), Mg, C, has_stats != 0, view_of(out), shuffle_ctot, pass_src ? &ps : nullptr, pass_dst ? &pd : nullptr),
        bn_bwd_reduce_plan(view_of(dout), shuffle_ctot, view_of(y), Mg, C, relu6 ? ACT_RELU6 : ACT_NONE, false, pass_gsrc ? &pgs : nullptr,
                           pass_gdst ? &pgd : nullptr, bcast_rows),
        bn_bwd_apply_plan(view_of(dout), view_of(y), Mg, C, dy, false)};
    int n = 0;
    for (const BnPlan& p : plans) {
        const int32_t f[] = {p.form, p.vec, p.cx, p.cy, p.nloop, p.rb, p.nb, p.al0, p.al1, p.al2};
        for (int32_t v : f) {
            if (n < n_out) fields[n] = v;
            ++n;
        }
    }
    return n;
}

// ---- fused 1x1-conv backward: the plan the launchers dispatch on, and the entry with the finalize-on-load arguments ----
static void pwb_fill(PwBwdFused& f, const cdrl_view* dz, int dz_shuffle, const cdrl_view* a, const cdrl_view* da, int accumulate, int G, int Mg,
                     int N, int K, const float* a_stats, const float* a_gamma, const float* a_beta, float* a_dgamma, float* a_dbeta,
                     float* a_coef, const double* fin_part, int fin_nb, double* fin_tot, float* o_dgamma, float* o_dbeta, int act_type) {
    f.dz = view_of(dz);
    f.dz_shuffle = dz_shuffle;
    f.a = view_of(a);
    f.da = view_of(da);
    f.accumulate = accumulate;
    f.G = G;
    f.Mg = Mg;
    f.N = N;
    f.K = K;
    f.a_stats = a_stats;
    f.a_gamma = a_gamma;
    f.a_beta = a_beta;
    f.a_dgamma = a_dgamma;
    f.a_dbeta = a_dbeta;
    f.a_coef = a_coef;
    f.fin_part = fin_part;
    f.fin_nb = fin_nb;
    f.fin_tot = fin_tot;
    f.o_dgamma = o_dgamma;
    f.o_dbeta = o_dbeta;
    f.at = act_type;
}

int cdrl_pwconv_bwd_plan(const cdrl_view* dz, int dz_shuffle, const cdrl_view* a, const cdrl_view* da, int accumulate, int G, int Mg, int N,
                         int K, const float* a_stats, const float* a_gamma, const float* a_beta, const float* a_dgamma, const float* a_dbeta,
                         const float* a_coef, const double* fin_part, int fin_nb, const double* fin_tot, const float* o_dgamma,
                         const float* o_dbeta, int act_type, int32_t* fields, int n_out) {
    if (bad_act_type(act_type)) return -1;
    if (!dz || !a || !da || dz_shuffle < 0 || (!fields && n_out > 0)) {
        cdrl::set_error("cdrl_pwconv_bwd_plan: the dz, a and da views are required (their pointers may be null), shuffle >= 0");
        return -1;
    }
    PwBwdFused f;
    pwb_fill(f, dz, dz_shuffle, a, da, accumulate, G, Mg, N, K, a_stats, a_gamma, a_beta, const_cast<float*>(a_dgamma), const_cast<float*>(a_dbeta),
             const_cast<float*>(a_coef), fin_part, fin_nb, const_cast<double*>(fin_tot), const_cast<float*>(o_dgamma), const_cast<float*>(o_dbeta),
             act_type);
    const PwbPlan p = pw_bwd_fused_plan(f);
    if (!p.ok) cdrl::set_error("%s", p.why);
    const int32_t v[] = {p.ok, p.refusal, p.form, p.kp, p.np, p.bm, p.tiles, p.nbpg, p.wp_ks, p.shuf, p.anorm, p.acc, p.fin, p.coef_needed,
                         p.lds_bytes, (int32_t)p.qpart_elems, (int32_t)p.dbpart_elems, (int32_t)p.spart_offset};
    int n = 0;
    for (int32_t x : v) {
        if (n < n_out) fields[n] = x;
        ++n;
    }
    return n;
}

int cdrl_pwconv_bwd_fused_fin(const cdrl_view* dz, int dz_shuffle, int act, const float* y, const float* stats, const float* coef,
                              const cdrl_view* a, const float* a_stats, const float* a_gamma, const float* a_beta, float* a_dgamma,
                              float* a_dbeta, float* a_coef, const float* W, const void* W_packed, const cdrl_view* da, int accumulate,
                              float* dW, float* db, float* qpart, double* dbpart, const double* fin_part, int fin_nb, double* fin_tot,
                              float* o_dgamma, float* o_dbeta, int G, int Mg, int N, int K, int act_type, void* stream) {
    const char* fn = "cdrl_pwconv_bwd_fused_fin";
    if (bad_act_type(act_type)) return -1;
    if (G < 1 || Mg < 1 || N < 1 || K < 1 || dz_shuffle < 0) {
        cdrl::set_error("%s: bad shape G %d Mg %d N %d K %d, shuffle %d", fn, G, Mg, N, K, dz_shuffle);
        return -1;
    }
    if (!view_ok(fn, "dz", dz, N, dz_shuffle) || !view_ok(fn, "a", a, K, 0) || !view_ok(fn, "da", da, K, 0)) return -1;
    // (coef: read only without finalize-on-load -- the plan's coef_needed)
    if (!y || !stats || (!coef && !fin_part) || !W || !W_packed || !dW || !db || !qpart || !dbpart) {
        cdrl::set_error("%s: null argument", fn);
        return -1;
    }
    PwBwdFused f;
    pwb_fill(f, dz, dz_shuffle, a, da, accumulate, G, Mg, N, K, a_stats, a_gamma, a_beta, a_dgamma, a_dbeta, a_coef, fin_part, fin_nb, fin_tot,
             o_dgamma, o_dbeta, act_type);
    f.act = act;
    f.y = y;
    f.stats = stats;
    f.coef = coef;
    f.W = W;
    f.Wp = W_packed;
    f.dW = dW;
    f.db = db;
    f.qpart = qpart;
    f.dbpart = dbpart;
    CDRL_TRY(pw_bwd_fused(f, S(stream)));
    return pw_bwd_fused_reduce(f, S(stream));
}

// ---- filter-gradient GEMM family: the plan gemm_tn dispatches on, the entry with its whole contract, and the partial reduce ----
// the K / N columns of a view (D: through the shuffle map) stay inside a row; pointers are not looked at
static const char* tn_views_fit(const cdrl_view* a, const cdrl_view* d, int N, int K, int has_dpro, int shuffle_ctot, int relu6) {
    if (!a || !d) return "the a and d views are required (their pointers may be null in the plan query)";
    if (shuffle_ctot < 0 || ((shuffle_ctot || relu6) && !has_dpro)) return "the shuffle gather and the ReLU6 mask belong to the D prologue";
    if (a->coff < 0 || a->coff + K > a->ld) return "the K channels of view a do not fit its rows";
    if (d->coff < 0 || (shuffle_ctot ? (shuffle_ctot % 2 != 0 || d->coff + N > shuffle_ctot || shuffle_ctot > d->ld) : d->coff + N > d->ld))
        return "the N channels of view d (through its shuffle) do not fit its rows";
    return nullptr;
}

int cdrl_gemm_tn_plan(const cdrl_view* a, const cdrl_view* d, int M, int N, int K, int G, int has_a_stats, int has_dpro, int shuffle_ctot,
                      int relu6, int bf16_operands, int act_type, int32_t* fields, int n_out) {
    if (bad_act_type(act_type)) return -1;
    if (!fields && n_out > 0) {
        cdrl::set_error("cdrl_gemm_tn_plan: no field array");
        return -1;
    }
    TnPlan p{};
    p.kernel = -1;
    const char* bad = tn_views_fit(a, d, N, K, has_dpro, shuffle_ctot, relu6);
    if (bad) {
        p.refusal = 4;
        p.why = bad;
    } else {
        p = gemm_tn_plan(view_of(a), view_of(d), M, N, K, G, has_a_stats != 0, has_dpro != 0, shuffle_ctot, bf16_operands != 0, act_type);
    }
    if (!p.ok) cdrl::set_error("cdrl_gemm_tn_plan: %s", p.why);
    const int32_t v[] = {p.ok, p.refusal, p.kernel, p.mode, p.apro, p.dpro, p.NJW, p.WK, p.NSPL, p.RS, p.RS2, p.U, p.gy, p.gz, p.nspg, p.nsplit,
                         p.rows_per, p.part_slots, (int32_t)p.part_elems, p.reduce_form, p.dhalf};
    int n = 0;
    for (int32_t x : v) {
        if (n < n_out) fields[n] = x;
        ++n;
    }
    return n;
}

int64_t cdrl_gemm_tn_ex_workspace_elems(int M, int N, int K, int G) {
    if (G < 1 || M < 1 || N < 1 || K < 1 || M % G != 0) return 0;
    return gemm_tn_part_elems(M, N, K, G);
}

int cdrl_gemm_tn_ex(const cdrl_view* a, const float* a_stats, const cdrl_view* d, const float* dpro_y, const float* dpro_stats,
                    const float* dpro_coef, int shuffle_ctot, int relu6, float* out, int M, int N, int K, int G, float* workspace,
                    int accumulate, int bf16_operands, int act_type, void* stream) {
    if (bad_act_type(act_type)) return -1;
    const char* bad = tn_views_fit(a, d, N, K, dpro_y != nullptr, shuffle_ctot, relu6);
    if (bad) {
        cdrl::set_error("cdrl_gemm_tn_ex: %s", bad);
        return -1;
    }
    if (!a->p || !d->p || !out || !workspace || (dpro_y && (!dpro_stats || !dpro_coef))) {
        cdrl::set_error("cdrl_gemm_tn_ex: null tensor, or a D prologue without its stats / coef");
        return -1;
    }
    const TnBnBwd tb{dpro_y, dpro_stats, dpro_coef, shuffle_ctot, relu6 ? ACT_RELU6 : ACT_NONE};
    return gemm_tn(view_of(a), view_of(d), out, M, N, K, workspace, accumulate, S(stream), G, a_stats, dpro_y ? &tb : nullptr,
                   bf16_operands != 0, act_type);
}

static bool reduce_args_ok(const char* fn, int nparts, int64_t n, int64_t stride) {
    if (nparts < 1 || n < 1 || stride < n) {
        cdrl::set_error("%s: nparts %d, n %lld, stride %lld: at least one partial and one output, rows no shorter than n", fn, nparts,
                        (long long)n, (long long)stride);
        return false;
    }
    return true;
}

int cdrl_reduce_partials_plan(uint64_t part_addr, int nparts, int64_t n, int64_t stride, int32_t* fields, int n_out) {
    if (!reduce_args_ok("cdrl_reduce_partials_plan", nparts, n, stride) || (!fields && n_out > 0)) return -1;
    const ReduceF32Plan p = reduce_partials_f32_plan((uintptr_t)part_addr, nparts, n, stride);
    const int32_t v[] = {p.form, (int32_t)p.grid, p.bx, p.by};
    int k = 0;
    for (int32_t x : v) {
        if (k < n_out) fields[k] = x;
        ++k;
    }
    return k;
}

int cdrl_reduce_partials_f32(const float* part, int nparts, int64_t n, int64_t stride, float* out, int accumulate, void* stream) {
    if (!reduce_args_ok("cdrl_reduce_partials_f32", nparts, n, stride)) return -1;
    if (!part || !out) {
        cdrl::set_error("cdrl_reduce_partials_f32: null argument");
        return -1;
    }
    return reduce_partials_f32(part, nparts, n, stride, out, accumulate, S(stream));
}

// ---- dense GEMM family: the plan gemm_nn dispatches on, the entry with its whole contract, the activations, the bias-gradient sums ----
static const char* nn_view_fits(const cdrl_view* v, int cols) {
    if (!v) return "a view is missing";
    if (v->coff < 0 || cols < 0 || v->coff + cols > v->ld) return "the columns of a view do not fit its rows";
    return nullptr;
}

int cdrl_gemm_nn_plan(const cdrl_view* a, uint64_t b_addr, int sbk, int sbn, int M, int N, int K, int has_workspace, int32_t* fields,
                      int n_out) {
    const char* bad = (!fields && n_out > 0) ? "no field array" : nn_view_fits(a, K);
    if (bad) {
        cdrl::set_error("cdrl_gemm_nn_plan: %s", bad);
        return -1;
    }
    const NnPlan p = gemm_nn_plan(view_of(a), reinterpret_cast<const float*>((uintptr_t)b_addr), sbk, sbn, M, N, K, has_workspace != 0);
    const int32_t v[] = {p.kernel, p.NT, p.WR, p.BT, p.VEC, p.gx, p.gy, p.gz, p.kchunk, (int32_t)p.ws_elems, p.reduce_grid, p.act_fused, p.a16, p.b16};
    int n = 0;
    for (int32_t x : v) {
        if (n < n_out) fields[n] = x;
        ++n;
    }
    return n;
}

// ---- 1x1-conv forward / backward-data family: the plans pw_nn, pw_x3 and pw_x3_wide_bwd launch from ----
// fields always written (a refusal shows its code in fields[1]); 0 when the plan is ok, -1 with the refusal sentence otherwise
static int pw_plan_result(const char* fn, bool views, const int32_t* v, int nf, int ok, const char* why, int32_t* fields, int n_fields) {
    if (!views || !fields || n_fields != nf) {
        cdrl::set_error("%s: the views (their pointers may be null) and an array of exactly %d fields are required", fn, nf);
        return -1;
    }
    std::copy(v, v + nf, fields);
    if (!ok) cdrl::set_error("%s", why);
    return ok ? 0 : -1;
}

int cdrl_pwconv_plan(const cdrl_view* a, const cdrl_view* c, uint64_t y_addr, int G, int Mg, int N, int K, int pro, int epi, int accumulate,
                     int packed, int packed_bf16, int act_type, int has_part, int32_t* fields, int n_fields) {
    PwNnPlan p{};
    if (a && c)
        p = pw_nn_plan(view_of(a), view_of(c), G, Mg, N, K, pro, epi, accumulate, packed != 0, packed_bf16 != 0, act_type, has_part != 0,
                       reinterpret_cast<const float*>((uintptr_t)y_addr));
    const int32_t v[] = {p.ok, p.refusal, p.ksm, p.nt, p.pro, p.epi, p.mode, p.acc, p.wc, p.wr, p.bm, p.tiles_g, p.nbpg, p.tpb, p.gx, p.gy, p.occ,
                         p.lds_bytes, (int32_t)p.packed_elems};
    return pw_plan_result("cdrl_pwconv_plan", a && c, v, (int)(sizeof(v) / sizeof(v[0])), p.ok, p.why, fields, n_fields);
}

int cdrl_pwconv_ex(const cdrl_view* a, const float* pro_stats, const float* bwd_y, const float* bwd_coef, int bwd_shuffle, int bwd_relu6,
                   double* part2, const float* w, int sbk, int sbn, const float* bias, const cdrl_view* c, int accumulate, int G, int Mg, int N,
                   int K, int epilogue, const float* epi_y, const float* epi_stats, double* part, const float* w_packed, int packed_bf16,
                   int act_type, void* stream) {
    if (bad_act_type(act_type)) return -1;
    if (!a || !c || !a->p || !c->p || !w || bwd_shuffle < 0 || (bwd_y && (!pro_stats || !bwd_coef)) || (epilogue == 2 && (!epi_y || !epi_stats))) {
        cdrl::set_error("cdrl_pwconv_ex: null tensor, a BatchNorm-backward prologue without its stats / coef, or epilogue 2 without epi_y / epi_stats");
        return -1;
    }
    const PwBnBwd bb{bwd_y, pro_stats, bwd_coef, bwd_shuffle, bwd_relu6 ? ACT_RELU6 : ACT_NONE, part2};
    return pw_nn(view_of(a), bwd_y ? nullptr : pro_stats, w, sbk, sbn, bias, view_of(c), accumulate, G, Mg, N, K, epilogue, epi_y, epi_stats, part,
                 S(stream), bwd_y ? &bb : nullptr, w_packed, packed_bf16 != 0, act_type);
}

int cdrl_pwconv_x3_plan(const cdrl_view* a, const cdrl_view* c, int G, int Mg, int N, int K, int pro, int epi, int packed, int nbpg,
                        int32_t* fields, int n_fields) {
    PwX3Plan p{};
    if (a && c) p = pw_x3_plan(view_of(a), view_of(c), G, Mg, N, K, pro != 0, epi != 0, packed != 0, nbpg);
    const int32_t v[] = {p.ok, p.refusal, p.form, p.kp, p.nt, p.pro, p.epi, p.bm, p.tiles_g, p.nbpg, p.gx, p.gy, (int32_t)p.packed_bytes};
    return pw_plan_result("cdrl_pwconv_x3_plan", a && c, v, (int)(sizeof(v) / sizeof(v[0])), p.ok, p.why, fields, n_fields);
}

int cdrl_pwconv_x3_wide_bwd_plan(const cdrl_view* dz, const cdrl_view* c, int G, int Mg, int N, int K, int dz_shuffle, int epi, int accumulate,
                                 int operands, int32_t* fields, int n_fields) {
    PwX3BwdPlan p{};
    if (dz && c) p = pw_x3_wide_bwd_plan(view_of(dz), view_of(c), G, Mg, N, K, dz_shuffle, epi != 0, accumulate, operands != 0);
    const int32_t v[] = {p.ok, p.refusal, p.sh, p.epi, p.acc, p.rows, p.gx, p.gy};
    return pw_plan_result("cdrl_pwconv_x3_wide_bwd_plan", dz && c, v, (int)(sizeof(v) / sizeof(v[0])), p.ok, p.why, fields, n_fields);
}

int64_t cdrl_gemm_nn_workspace_elems(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 1) return 0;
    return gemm_nn_splitk_elems(M, N, K);
}

int cdrl_gemm_nn_ex(const cdrl_view* a, const float* B, int sbk, int sbn, const float* bias, const cdrl_view* c, int M, int N, int K,
                    int accumulate, float* workspace, float* act_out, int act, int* act_done, void* stream) {
    if (act_done) *act_done = 0;
    const char* bad = nn_view_fits(a, K);
    if (!bad) bad = nn_view_fits(c, N);
    if (!bad && (!a->p || !c->p || !B)) bad = "null tensor";
    if (!bad && act_out && !workspace) bad = "act_out is written by the split-K reduce: it needs the workspace";
    if (!bad && (act < ACT_NONE || act > ACT_SIGMOID)) bad = "unknown activation";
    if (bad) {
        cdrl::set_error("cdrl_gemm_nn_ex: %s (M %d N %d K %d act %d)", bad, M, N, K, act);
        return -1;
    }
    bool done = false;
    const int rc = gemm_nn(view_of(a), B, sbk, sbn, bias, view_of(c), M, N, K, accumulate, S(stream), workspace, act_out, act,
                           act_done ? &done : nullptr);
    if (act_done) *act_done = done ? 1 : 0;
    return rc;
}

static bool flat_args_ok(const char* fn, bool ptrs, int64_t n, int act) {
    if (!ptrs || n < 1 || act < ACT_NONE || act > ACT_SIGMOID) {
        cdrl::set_error("%s: null tensor, n %lld < 1 or unknown activation %d", fn, (long long)n, act);
        return false;
    }
    return true;
}

int cdrl_act_fwd(const float* z, float* a, int64_t n, int act, void* stream) {
    if (!flat_args_ok("cdrl_act_fwd", z && a, n, act)) return -1;
    return act_fwd(z, a, n, act, S(stream));
}

int cdrl_act_bwd(const float* z, const float* da, float* dz, int64_t n, int act, void* stream) {
    if (!flat_args_ok("cdrl_act_bwd", z && da && dz, n, act)) return -1;
    return act_bwd(z, da, dz, n, act, S(stream));
}

int cdrl_colsum_partial_rows(int rows, int C) {
    if (rows < 1 || C < 1) return 0;
    return vcol_geom(rows, C).nb;
}

int cdrl_colsum(const cdrl_view* x, int rows, int C, double* part, void* stream) {
    if (rows < 1 || C < 1 || !part) {
        cdrl::set_error("cdrl_colsum: rows %d, C %d or a null partial buffer", rows, C);
        return -1;
    }
    if (!view_ok("cdrl_colsum", "x", x, C, 0)) return -1;
    return colsum(view_of(x), rows, C, part, S(stream));
}

int cdrl_reduce_partials_cx(int nparts, int n1, int n2) {
    if (nparts < 1 || n1 < 1 || n2 < 0) return 0;
    return reduce_partials_cx(nparts, n1 + n2);
}

int cdrl_reduce_partials(const double* part, int nparts, int n1, int n2, int64_t stride, float* out1, float* out2, int accumulate,
                         void* stream) {
    if (nparts < 1 || n1 < 1 || n2 < 0 || stride < (int64_t)n1 + n2 || !part || !out1 || (n2 > 0 && !out2)) {
        cdrl::set_error("cdrl_reduce_partials: nparts %d, n1 %d, n2 %d, stride %lld, or a null tensor", nparts, n1, n2, (long long)stride);
        return -1;
    }
    if (n2 == 0) return reduce_partials(part, nparts, n1, stride, out1, accumulate, S(stream));
    return reduce_partials2(part, nparts, n1, n2, stride, out1, out2, accumulate, S(stream));
}

int cdrl_permute_bt(const float* src, float* dst, int B, int T, int D, void* stream) {
    if (!src || !dst || B < 1 || T < 1 || D < 1) {
        cdrl::set_error("cdrl_permute_bt: null tensor or bad shape B %d T %d D %d", B, T, D);
        return -1;
    }
    return permute_bt(src, dst, B, T, D, S(stream));
}

int cdrl_bn_act_gap_fwd(const float* y, const float* stats, float* out, int G, int frames_per_group, int P, int C, int relu6,
                        int act_type, void* stream) {
    if (bad_act_type(act_type)) return -1;
    if (!y || !stats || !out || G < 1 || frames_per_group < 1 || P < 1 || C < 1) {
        cdrl::set_error("cdrl_bn_act_gap_fwd: null tensor or bad shape G %d frames %d P %d C %d", G, frames_per_group, P, C);
        return -1;
    }
    return bn_act_gap_fwd(y, stats, out, G, frames_per_group, P, C, relu6 ? ACT_RELU6 : ACT_NONE, S(stream), act_type);
}

int cdrl_gather_view(const cdrl_view* src, int shuffle_ctot, int rows, int C, const cdrl_view* dst, int accumulate, void* stream) {
    if (rows < 1 || C < 1 || shuffle_ctot < 0) {
        cdrl::set_error("cdrl_gather_view: bad shape rows %d C %d shuffle %d", rows, C, shuffle_ctot);
        return -1;
    }
    if (!view_ok("cdrl_gather_view", "src", src, C, shuffle_ctot) || !view_ok("cdrl_gather_view", "dst", dst, C, 0)) return -1;
    return gather_view(view_of(src), shuffle_ctot, rows, C, view_of(dst), accumulate, S(stream));
}

int64_t cdrl_bn_inference_stats_table_bytes(int n) { return (int64_t)(n > 0 ? n : 0) * (int64_t)sizeof(BnInfEntry); }

int cdrl_bn_inference_stats(int n, const float* const* gamma, const float* const* beta, const float* const* moving_mean,
                            const float* const* moving_var, float* const* stats, const int* G, const int* C, void* table_dev,
                            void* stream) {
    if (n < 1 || n > 1024 || !gamma || !beta || !moving_mean || !moving_var || !stats || !G || !C || !table_dev) {
        cdrl::set_error("cdrl_bn_inference_stats: 1..1024 layers, no null array");
        return -1;
    }
    BnInfEntry tab[1024];
    int max_c = 0;
    for (int i = 0; i < n; ++i) {
        if (!gamma[i] || !beta[i] || !moving_mean[i] || !moving_var[i] || !stats[i] || G[i] < 1 || C[i] < 1) {
            cdrl::set_error("cdrl_bn_inference_stats: layer %d has a null vector or a bad shape", i);
            return -1;
        }
        tab[i] = BnInfEntry{gamma[i], beta[i], moving_mean[i], moving_var[i], stats[i], G[i], C[i]};
        if (C[i] > max_c) max_c = C[i];
    }
    // the table lives on this frame: the copy goes through the stream, and the call waits for it before the frame goes away
    CDRL_HIP(hipMemcpyAsync(table_dev, tab, (size_t)n * sizeof(BnInfEntry), hipMemcpyHostToDevice, S(stream)));
    CDRL_HIP(hipStreamSynchronize(S(stream)));
    return bn_inference_stats_many(static_cast<const BnInfEntry*>(table_dev), n, max_c, S(stream));
}

int cdrl_bn_small_fwd(const float* y, int M, int C, const float* gamma, const float* beta, float* moving_mean,
                      float* moving_var, float* stats, float* out, void* stream) {
    return bn_small_fwd(make_view(const_cast<float*>(y), C), M, C, gamma, beta, moving_mean, moving_var, stats, make_view(out, C),
                        S(stream));
}

int cdrl_bn_small_bwd(const float* dout, const float* y, int M, int C, const float* stats, float* dgamma, float* dbeta,
                      float* coef, float* dx, void* stream) {
    return bn_small_bwd(make_view(const_cast<float*>(dout), C), make_view(const_cast<float*>(y), C), M, C, stats, dgamma, dbeta,
                        coef, dx, S(stream));
}

int cdrl_bn_small_bwd_pair(const float* doutA, const float* doutB, const float* y, int M, int C, const float* statsA,
                           const float* statsB, float* dgammaA, float* dbetaA, float* coefA, float* dgammaB, float* dbetaB,
                           float* coefB, float* dx, void* stream) {
    if (!doutA || !doutB || !y || !statsA || !statsB || !dgammaA || !dbetaA || !coefA || !dgammaB || !dbetaB || !coefB || !dx) {
        set_error("cdrl_bn_small_bwd_pair: null argument");
        return -1;
    }
    if (M < 1 || C < 1) {
        set_error("cdrl_bn_small_bwd_pair: M = %d, C = %d", M, C);
        return -1;
    }
    return bn_small_bwd_pair(make_view(const_cast<float*>(doutA), C), make_view(const_cast<float*>(doutB), C),
                             make_view(const_cast<float*>(y), C), M, C, statsA, statsB, dgammaA, dbetaA, coefA, dgammaB, dbetaB, coefB,
                             dx, S(stream));
}

static int make_head_set(HeadSet& hs, int nheads, const int* n, const float* const* w, const float* const* b, float* const* dw,
                         float* const* db) {
    if (nheads < 1 || nheads > HEADS_MAX) {
        set_error("linear_heads: %d heads not supported", nheads);
        return -1;
    }
    memset(&hs, 0, sizeof(hs));
    hs.nheads = nheads;
    int off = 0;
    for (int h = 0; h < nheads; ++h) {
        hs.n[h] = n[h];
        hs.off[h] = off;
        hs.w[h] = w[h];
        hs.b[h] = b ? b[h] : nullptr;
        hs.gw[h] = dw ? dw[h] : nullptr;
        hs.gb[h] = db ? db[h] : nullptr;
        off += n[h];
    }
    return off;
}

int cdrl_linear_heads_fwd(const float* a, int nheads, const int* n, const float* const* w, const float* const* b, float* lin,
                          int B, int K, void* stream) {
    HeadSet hs;
    const int L = make_head_set(hs, nheads, n, w, b, nullptr, nullptr);
    if (L < 0) return L;
    return heads_fwd(a, K, hs, lin, L, B, K, S(stream));
}

int cdrl_linear_heads_bwd(const float* a, int nheads, const int* n, const float* const* w, const float* dlin, float* da,
                          float* const* dw, float* const* db, int B, int K, void* stream) {
    HeadSet hs;
    const int L = make_head_set(hs, nheads, n, w, nullptr, dw, db);
    if (L < 0) return L;
    return heads_bwd(a, K, hs, dlin, L, da, K, B, K, S(stream));
}

int cdrl_maxpool_bn_fwd(const float* y, const float* stats, int G, int frames_per_group, float* p, uint8_t* argmax,
                        int N, int H, int W, int C, int act_type, void* stream) {
    return maxpool_bn_fwd(y, stats, G, frames_per_group, p, argmax, N, H, W, C, S(stream), act_type);
}

int cdrl_bn_train_bwd_pooled(const uint8_t* argmax, const float* dp, int H, int W, const float* y, int G, int Mg, int C,
                             const float* stats, float* dgamma, float* dbeta, float* dy, float* coef, double* workspace,
                             void* stream) {
    View yv = make_view(const_cast<float*>(y), C);
    View none = make_view(nullptr, 0);
    PoolSrc ps = make_pool_src(argmax, dp, H, W);
    const int nb = vcol_geom(Mg, C).nb;
    CDRL_TRY(bn_bwd_reduce(none, 0, yv, G, Mg, C, stats, ACT_RELU6, workspace, S(stream), &ps));
    CDRL_TRY(bn_bwd_finalize(workspace, nb, G, Mg, C, stats, dgamma, dbeta, coef, S(stream)));
    return bn_bwd_apply(none, 0, yv, G, Mg, C, stats, coef, ACT_RELU6, dy, workspace, S(stream), &ps);
}

int cdrl_beta_ppo_loss(const float* lin, const float* adv, const float* old_logp, const float* speed,
                       const float* similarity, const float* u, const float* du_da, const float* du_db, float clip_ratio,
                       float entropy_coef, int B, int A, float grad_scale, float* dlin, float* metrics, float* aux,
                       float* hp_scratch16, void* stream) {
    DevHP h;
    memset(&h, 0, sizeof(h));
    h.clip_ratio = clip_ratio;
    h.entropy_coef = entropy_coef;
    CDRL_HIP(hipMemcpyAsync(hp_scratch16, &h, sizeof(h), hipMemcpyHostToDevice, S(stream)));
    PolicyLossArgs a;
    a.lin = lin; a.adv = adv; a.old_logp = old_logp; a.speed = speed; a.similarity = similarity;
    a.u = u; a.du_da = du_da; a.du_db = du_db; a.hp = hp_scratch16; a.dlin = dlin; a.metrics = metrics; a.aux = aux;
    a.B = B; a.A = A; a.inv_world = grad_scale;
    return policy_loss(a, S(stream));
}

int cdrl_beta_clone_loss(const float* lin, const float* u, const float* weight, const float* speed, const float* similarity,
                         float entropy_coef, float aux_weight, int B, int A, float grad_scale, float* dlin, float* metrics, float* aux,
                         void* stream) {
    CloneLossArgs a;
    a.lin = lin; a.u = u; a.weight = weight; a.speed = speed; a.similarity = similarity; a.hp = nullptr;
    a.entropy_coef = entropy_coef; a.aux_weight = aux_weight; a.dlin = dlin; a.metrics = metrics; a.aux = aux;
    a.B = B; a.A = A; a.grad_scale = grad_scale;
    return clone_loss(a, S(stream));
}

int cdrl_beta_mixed_policy_loss(const float* lin, const float* adv, const float* old_logp, const float* speed,
                                const float* similarity, const float* u, const float* du_da, const float* du_db, const float* demo_u,
                                const float* demo_w, float clip_ratio, float entropy_coef, int B, int A, float grad_scale, float* dlin,
                                float* metrics, float* aux, float* hp_scratch16, cdrl_demo_stats* demo_block, void* stream) {
    MixedPolicyLossArgs m;
    PolicyLossArgs& a = m.ppo;
    a.lin = lin; a.adv = adv; a.old_logp = old_logp; a.speed = speed; a.similarity = similarity;
    a.u = u; a.du_da = du_da; a.du_db = du_db; a.hp = hp_scratch16; a.dlin = dlin; a.metrics = metrics; a.aux = aux;
    a.B = B; a.A = A; a.inv_world = grad_scale;
    m.demo_u = demo_u; m.demo_w = demo_w; m.block = reinterpret_cast<cdrl::DemoBlock*>(demo_block);
    if (!adv || !old_logp || !speed || !similarity || !hp_scratch16) {
        cdrl::set_error("cdrl_beta_mixed_policy_loss: a null adv / old_logp / speed / similarity / hp_scratch16");
        return -1;
    }
    // (the wrapper's own refusals first: nothing is enqueued for a refused call)
    if (A < 1 || A > 8 || B < 1 || !lin || !u || !demo_u || !demo_w || !dlin || !metrics) return mixed_policy_loss(m, S(stream));
    DevHP h;
    memset(&h, 0, sizeof(h));
    h.clip_ratio = clip_ratio;
    h.entropy_coef = entropy_coef;
    CDRL_HIP(hipMemcpyAsync(hp_scratch16, &h, sizeof(h), hipMemcpyHostToDevice, S(stream)));
    return mixed_policy_loss(m, S(stream));
}

int cdrl_beta_kl(const float* lin, const float* anchor, int B, int A, float kl_coef, float grad_scale, float* dlin, float* metrics,
                 void* stream) {
    if (!metrics) {
        cdrl::set_error("cdrl_beta_kl: null metrics");
        return -1;
    }
    if (!(kl_coef >= 0.0f)) {
        cdrl::set_error("cdrl_beta_kl: kl_coef = %g must not be negative", (double)kl_coef);
        return -1;
    }
    BetaKlArgs a;
    a.lin = lin; a.anchor = anchor; a.dlin = dlin; a.trust = nullptr; a.kl_coef = kl_coef; a.metrics = metrics;
    a.B = B; a.A = A; a.inv_world = grad_scale;
    return beta_kl(a, S(stream));
}

int cdrl_beta_score(const float* dist, const float* value, const float* u, const float* returns_be, const float* speed,
                    const float* similarity, int rows, int count, int A, double* block, double* pit, void* stream) {
    static_assert(CDRL_SCORE_BINS == SCORE_BINS && CDRL_SCORE_HEAD == SCORE_HEAD && CDRL_SCORE_PER_ACTION == SCORE_PER_ACTION &&
                      CDRL_SCORE_BLOCK(8) == score_block_doubles(8),
                  "cdrl.h and score_block.h disagree on the score block");
    BetaScoreArgs a;
    a.dist = dist; a.value = value; a.u = u; a.returns_be = returns_be; a.speed = speed; a.similarity = similarity;
    a.rows = rows; a.count = count; a.A = A; a.block = block; a.pit = pit;
    return beta_score(a, S(stream));
}

int64_t cdrl_ntxent_workspace_floats(int B, int D) { return ntxent_workspace_floats(B, D); }

int cdrl_ntxent_loss(const float* z, int B, int D, float temperature, float grad_scale, float* dz, float* metrics, float* workspace,
                     void* stream) {
    NtxentArgs a;
    a.z = z; a.dz = dz; a.metrics = metrics; a.workspace = workspace;
    a.B = B; a.D = D; a.temperature = temperature; a.grad_scale = grad_scale;
    return ntxent_loss(a, S(stream));
}

int cdrl_value_loss(const float* lin, const float* returns, const float* speed, const float* similarity, int B,
                    float exp_scale, float grad_scale, float* dlin, float* metrics, float* values, void* stream) {
    ValueLossArgs a;
    a.lin = lin; a.returns = returns; a.speed = speed; a.similarity = similarity; a.dlin = dlin; a.metrics = metrics;
    a.values = values; a.B = B; a.exp_scale = exp_scale; a.inv_world = grad_scale;
    return value_loss(a, S(stream));
}

}  // extern "C"

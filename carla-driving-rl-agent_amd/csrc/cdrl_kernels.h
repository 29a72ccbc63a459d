// Internal C++ launch API of libcdrl_hip.so.  Every function enqueues work on `st`, never
// allocates, never synchronises, and returns 0 on success (<0: see cdrl::last_error()).
#pragma once
#include "cdrl_common.h"
#include "trust_block.h"
#include "demo_block.h"

namespace cdrl {

// ---------------------------------------------------------------- BatchNorm family (bn.hip)
// Per-group column statistics of y (rows grouped contiguously: group g = rows [g*Mg,(g+1)*Mg)).
// part layout: [G][nb][2][C] (sum, sum of squares); nb from col_geom(Mg, C).
// at (here and below): element type of the ACTIVATION tensors the pointers / views refer to -- 0: float32, 1: bf16 (storage only:
// everything computed, reduced or kept as statistics stays float32 / double; configuration 3)
int colstats(View y, int G, int Mg, int C, double* part, hipStream_t st, int at = 0);
// Turns partials (training) or moving statistics (inference) into per-(group,channel) mean /
// invstd / scale / shift and applies the T sequential EMA updates.
int bn_finalize(const double* part, int nb, int G, int Mg, int C, const float* gamma, const float* beta,
                float* mov_mean, float* mov_var, int bessel, int training, float* stats /*[4][G][C]*/,
                hipStream_t st);
// One launch for the inference-mode statistics blocks of many BatchNorm layers (the training == 0 branch of bn_finalize, batched)
struct BnInfEntry {
    const float *gamma, *beta, *mov_mean, *mov_var;
    float* stats;           // [4][G][C]
    int G, C;
};
int bn_inference_stats_many(const BnInfEntry* tab_dev, int n, int max_c, hipStream_t st);
// dst = act(scale*y + shift); optional de-interleave shuffle on the destination channel index.
// stats == nullptr -> plain copy.
// pass_src / pass_dst: optional second tensor with the same C channels copied through the same shuffle store (the
// identity half of a ShuffleNet unit: concat + shuffle of both halves in one launch)
int bn_apply(View y, int G, int Mg, int C, const float* stats, int act, View dst, int shuffle_ctot,
             hipStream_t st, const View* pass_src = nullptr, const View* pass_dst = nullptr, int at = 0);
// single-group BatchNorm over few rows, one launch per direction (G = 1, no activation, no shuffle; training mode)
int bn_small_fwd(View x, int M, int C, const float* gamma, const float* beta, float* mov_mean, float* mov_var, float* stats,
                 View out, hipStream_t st);
int bn_small_bwd(View dout, View x, int M, int C, const float* stats, float* dgamma, float* dbeta, float* coef, float* dx,
                 hipStream_t st);
// backward of two such BatchNorms A and B over the SAME input x in one launch: per-BatchNorm outputs bit-identical to bn_small_bwd on
// each alone, dx = dxA + dxB (one float32 addition per element)
int bn_small_bwd_pair(View doutA, View doutB, View x, int M, int C, const float* statsA, const float* statsB, float* dgammaA,
                      float* dbetaA, float* coefA, float* dgammaB, float* dbetaB, float* coefB, float* dx, hipStream_t st);
// Gradient source "through a 3x3/s2 SAME max-pool": d(a)[n,iy,ix,c] = sum of dp over the windows whose
// saved argmax points at (iy,ix).  Lets the stem BatchNorm backward read the pooled gradient directly
// (the 255 MB pre-pool gradient tensor is never written or re-read).
struct PoolSrc {
    const uint8_t* argmax;   // [N][Ho][Wo][C]
    const float* dp;         // [N][Ho][Wo][C]
    int H, W, Ho, Wo, pt, pl;
    const float* pa = nullptr;   // optional: the pooled ACTIVATED output [N][Ho][Wo][C] of the forward; lets
                                 // pool_bn_bwd_reduce skip the gather of the pre-pool values (see there)
};
// Backward: reduce (sum dz, sum dz*xhat) -> part [G][nb][2][C]
int bn_bwd_reduce(View da, int shuffle_ctot, View y, int G, int Mg, int C, const float* stats, int act,
                  double* part, hipStream_t st, const PoolSrc* pool = nullptr, const View* pass_gsrc = nullptr,
                  const View* pass_gdst = nullptr, int bcast_rows = 0, int at = 0);
// bcast_rows > 0 (here and in bn_bwd_apply): `da` holds ONE row per bcast_rows rows of y and is divided by bcast_rows on load --
// the gradient of a global average pool over bcast_rows pixels, never materialised (head of the tower)     // pass_*: gradient of the identity half gathered in the same pass
// Same sums for a BN+ReLU6 that feeds a 3x3/s2 max-pool, in scatter form over the POOLED gradient (ps.dp, ps.argmax);
// y: the BN's raw input [G*frames_per_group][ps.H][ps.W][C]; part [G][nb][2][C], nb = vcol_geom(frames*Ho*Wo, C).nb
int pool_bn_bwd_reduce(const PoolSrc& ps, const float* y, int G, int frames_per_group, int C, const float* stats, double* part,
                       hipStream_t st, int at = 0);
// dgamma/dbeta (+= over groups; `accumulate` keeps previous content) and coefficients coef[3][G][C]
int bn_bwd_finalize(const double* part, int nb, int G, int Mg, int C, const float* stats, float* dgamma,
                    float* dbeta, float* coef, hipStream_t st);
// dy = k1*(dz - k2 - xhat*k3) (dense [G*Mg][C]); also column sums of dy -> part2 [G][nb][C]
int bn_bwd_apply(View da, int shuffle_ctot, View y, int G, int Mg, int C, const float* stats,
                 const float* coef, int act, float* dy, double* part2, hipStream_t st, const PoolSrc* pool = nullptr,
                 int bcast_rows = 0, int at = 0);
// out[i] (+)= sum_p part[p*stride + i], i < n
int reduce_partials(const double* part, int nparts, int n, int64_t stride, float* out, int accumulate,
                    hipStream_t st);
// two outputs from one partial row: columns [0, n1) -> out1, [n1, n1+n2) -> out2 (filter + bias in one launch)
int reduce_partials2(const double* part, int nparts, int n1, int n2, int64_t stride, float* out1, float* out2, int accumulate,
                     hipStream_t st);
// the CX (outputs per block: 16 or 4) of the reduce_partials_kernel both launch for nparts partials of n = n1 + n2 outputs
int reduce_partials_cx(int nparts, int n);
// column sums of a view: part [nb][C] with nb = col_geom(rows, C).nb
int colsum(View x, int rows, int C, double* part, hipStream_t st);
// dst(view) = src(view) gathered through the shuffle map on the *source* (backward of shuffle)
int gather_view(View src, int shuffle_ctot, int rows, int C, View dst, int accumulate, hipStream_t st);
// What the three launchers above dispatch on (they call these and launch what the plan says; cdrl_bn_plan reports the same structs).
// form: 0 the generic vcolreduce-style kernel, 1 the fast kernel (bn_apply_shuf_kernel / bn_bwd_reduce_shuf_kernel /
// bn_bwd_apply_fast_kernel); vec .. nb: the vcol_geom the launch uses; al0..al2: the alignment flags the generic kernel receives --
// apply: y, dst, pass_src; reduce: da, y, pass_gdst; backward apply: da, y, dy (a misaligned dy is refused by form 0).
struct BnPlan {
    int form, vec, cx, cy, nloop, rb, nb;
    int al0, al1, al2;
};
BnPlan bn_apply_plan(View y, int Mg, int C, bool has_stats, View dst, int shuffle_ctot, const View* pass_src, const View* pass_dst);
BnPlan bn_bwd_reduce_plan(View da, int shuffle_ctot, View y, int Mg, int C, int act, bool pool, const View* pass_gsrc,
                          const View* pass_gdst, int bcast_rows);
BnPlan bn_bwd_apply_plan(View da, View y, int Mg, int C, const float* dy, bool pool);
// elementwise activation on dense [n] arrays
int act_fwd(const float* z, float* a, int64_t n, int act, hipStream_t st);
int act_bwd(const float* z, const float* da, float* dz, int64_t n, int act, hipStream_t st);
int fill(float* p, int64_t n, float v, hipStream_t st);
// (B,T,D) -> (T*B, D)
int permute_bt(const float* src, float* dst, int B, int T, int D, hipStream_t st);
// dst[i,:] = src[idx[i],:]
int gather_rows(const float* src, const int* idx, float* dst, int nrows, int64_t row_elems, hipStream_t st);

// ---------------------------------------------------------------- GEMM (gemm.hip)
// C[M,N] (view) (+)= A[M,K] (view) * B(k,n) + bias[n];  B(k,n) = Bp[k*sbk + n*sbn].
// fp32 MFMA (v_mfma_f32_32x32x2_f32): results are bit-identical to a k-ordered fmaf chain.
// splitk_ws (>= gemm_nn_splitk_elems floats, or null): enables split-K for small-M / long-K products
int64_t gemm_nn_splitk_elems(int M, int N, int K);
// The one dispatch decision of gemm_nn: which kernel, which instantiation, which grid, how much workspace.  gemm_nn_plan is address
// arithmetic only (reads no memory, launches nothing); gemm_nn launches from it and cdrl_gemm_nn_plan reports it.
// Instantiations: gemm_nn_kernel<NT, BT, VEC, WR> for (NT, WR) in {(1, 4), (3, 4), (2, 2), (4, 2)}, gemm_nn_rt_kernel<3, BT>.
struct NnPlan {
    int kernel;                 // -1 empty product (M or N < 1), 0 gemm_nn_kernel, 1 gemm_nn_rt_kernel, 2 split-K: gemm_nn_kernel with
                                // gridDim.z = gz slabs into the workspace, then splitk_reduce_kernel
    int NT, WR, BT, VEC;        // template arguments (kernel 1: NT = RT = 3, WR 0, VEC 0)
    int gx, gy, gz;             // grid; gz = number of K splits (1 unless kernel 2)
    int kchunk;                 // K range of one split (a multiple of 32; 1 << 30 without split-K)
    int64_t ws_elems;           // floats of workspace split-K writes: gz * M * N (<= gemm_nn_splitk_elems)
    int reduce_grid;            // blocks of splitk_reduce_kernel (0 unless kernel 2)
    int act_fused;              // kernel 2: the reduce can write act_out (gemm_nn does so when act_out and act_done are given)
    int a16, b16;               // 16-byte alignment of the A rows / of the weight rows (what kernel 1 needs next to N >= 129, K >= 64, M >= 2048)
};
NnPlan gemm_nn_plan(View A, const float* Bp, int sbk, int sbn, int M, int N, int K, bool has_workspace);
int gemm_nn(View A, const float* Bp, int sbk, int sbn, const float* bias, View C, int M, int N, int K,
            int accumulate, hipStream_t st, float* splitk_ws = nullptr,
            float* act_out = nullptr, int act = 0, bool* act_done = nullptr);
// act_out / act / act_done: when the product goes through split-K, its reduce also writes act(C) to the dense [M][N] act_out and
// sets *act_done (the caller runs act_fwd otherwise)
// Cout[K,N] = sum_m A[m,K]^T * D[m,N]  (split over M; partial buffer `part` >= gemm_tn_part_elems)
// G > 1: rows are G equal BatchNorm groups; pro_stats ([4][G][K]) != null applies A <- scale[g][k]*A + shift[g][k] on load.
// dpro != null: D[m,n] <- k1*(dz - k2 - xhat*k3) on load (BatchNorm-backward apply; D views the gradient w.r.t. the BN
// output, optionally through the channel-shuffle gather / ReLU6 mask); needs gemm_tn_dpro_supported(N) and G groups.
struct TnBnBwd {
    const float* y;         // raw BN input [M][N] dense
    const float* stats;     // [4][G][N]
    const float* coef;      // [3][G][N]
    int shuffle_ctot;
    int act;
};
bool gemm_tn_dpro_supported(int N);
int64_t gemm_tn_part_elems(int M, int N, int K, int G = 1);
// The one dispatch decision of gemm_tn: which kernel, which instantiation, which grid, how many partials, which reduce.  gemm_tn_plan
// fills it from the shapes, the views' leading dimensions / offsets and CDRL_TN_LDS_F32 (reads no memory, launches nothing); gemm_tn
// launches from it and cdrl_gemm_tn_plan reports it.
struct TnPlan {
    int ok, refusal;            // refusal (ok == 0): 1 G < 1 or M % G != 0, 2 bf16 storage without bf16 operands, 3 an operand of 2 GB or more
    const char* why;
    int kernel;                 // 0 tn_direct_kernel, 1 tn_direct_tr_kernel, 2 tn_lds_kernel; -1: an empty product, nothing is launched
    int mode;                   // the kernel's MODE template argument
    int apro, dpro;             // operand prologues (template arguments)
    int NJW, WK, NSPL, RS, RS2, U;          // direct kernels: wave mapping and batch depth (0 for the LDS kernel)
    int gy, gz, nspg, nsplit, rows_per;     // grid = (nsplit = G * nspg, gy, gz); rows per workgroup
    int part_slots;             // partials [part_slots][K][N]: nsplit * RS (direct), nsplit (LDS)
    int64_t part_elems;
    int reduce_form;            // reduce_partials_f32_plan for a 16-byte aligned workspace
    int dhalf;                  // LDS kernel: some thread gathers its last column pair as (s - 1, s) (shuffle, N = 2 mod 4)
};
TnPlan gemm_tn_plan(View A, View D, int M, int N, int K, int G, bool apro, bool dpro, int shuffle_ctot, bool bf16_operands, int at);
// bf16_operands: both operands rounded to bf16 AFTER their prologues, v_mfma_f32_32x32x16_bf16 over 16-row steps (configuration 3)
int gemm_tn(View A, View D, float* Cout, int M, int N, int K, float* part, int accumulate, hipStream_t st, int G = 1,
            const float* pro_stats = nullptr, const TnBnBwd* dpro = nullptr, bool bf16_operands = false, int at = 0);

// LDS-staged form (gemm_tn_lds.hip): same contract as gemm_tn; gemm_tn dispatches to it for the shapes it takes (K, N >= 96 and
// gemm_tn_lds_supported).  mode: 2 bf16 tensors, 1 float32 tensors with bf16 operands, 0 float32 operands on v_mfma_f32_32x32x2_f32
// (the float32 engine's arithmetic), 3 float32-accurate product from three bf16 planes per operand on v_mfma_f32_32x32x16_bf16 (six
// plane products).  gemm_tn_lds_plan fills the grid fields, part_slots and dhalf of a plan; gemm_tn_lds launches from the plan.
bool gemm_tn_lds_supported(View A, View D, int N, int K, int shuffle_ctot);
int64_t gemm_tn_lds_part_elems(int M, int N, int K, int G = 1);
void gemm_tn_lds_plan(TnPlan& p, int M, int N, int K, int G, int shuffle_ctot);
int gemm_tn_lds(const TnPlan& p, View A, View D, float* Cout, int M, int N, int K, float* part, int accumulate, hipStream_t st, int G,
                const float* pro_stats, const TnBnBwd* dpro);

// ---------------------------------------------------------------- fused pointwise conv (gemm_pw.hip)
// Persistent skinny GEMM for K, N <= 128: C[m,n] (+)= sum_k pro(A[m,k]) W(k,n) + bias[n] over G groups of Mg rows.
//   pro_stats != null : A <- scale[g][k]*A + shift[g][k]  (BatchNorm apply of the previous layer)
//   epilogue 1        : part[g][b][2][N] = (sum c, sum c^2)            -> bn_finalize(part, nb = pw_nn_plan().nbpg)
//   epilogue 2        : part[g][b][2][N] = (sum c, sum c*xhat(ey))     -> bn_bwd_finalize(part, nb = ...nbpg)
// What pw_nn launches for a call and why it refuses one: the ONE place that knows the column-tile count (N > 128: four tiles per
// block and gy = 2), the K padding, which (ksm, nt) pairs are instantiated (nt == 3 needs ksm <= 32, ksm == 128 needs nt == 4), the
// row split, the grid and the dynamic LDS size.  Address arithmetic only: launches nothing, reads no memory.  The geometry fields
// are filled whenever G, Mg, N >= 1, also for a refused call (the partial-row queries read them).  DESIGN.md 3.9.
enum PwRefusal {
    PW_OK = 0,
    PW_REFUSE_DIMS = 1,         // G < 1, Mg < 1, N < 1 or K < 2: nothing to launch
    PW_REFUSE_SHAPE = 2,        // K or N above 256, K odd
    PW_REFUSE_TILE = 3,         // a (ksm, nt) pair that is not instantiated
    PW_REFUSE_ALIGN = 4,        // odd leading dimension / channel offset, pointer not 8-byte aligned
    PW_REFUSE_PRO_EPI = 5,      // prologue / epilogue outside 0..2, or the pairs (1, 2) and (2, 1)
    PW_REFUSE_PART = 6,         // an epilogue without its partial buffer
    PW_REFUSE_2GB = 7,          // an operand of 2 GB or more (32-bit buffer offsets)
    PW_REFUSE_STORAGE = 8,      // bf16 activation storage without packed bf16 weights
    PW_REFUSE_COUNT = 9,
};
struct PwNnPlan {
    int ok, refusal;
    int ksm, nt, pro, epi, mode, acc;   // pw_nn_kernel<KSM, NT, PRO, EPI, MODE, ACC>; acc only with epi == 0 (else a run-time read-modify-write)
    int wc, wr, bm;             // wave columns / rows, rows per tile
    int tiles_g, nbpg, tpb;     // tiles per group, workgroups (= partial rows) per group, most tiles one workgroup walks
    int gx, gy;                 // grid
    int occ;                    // resident workgroups per CU the grid target counts with
    int lds_bytes;              // dynamic LDS
    int64_t packed_elems;       // floats of the packed weights (pw_packed_elems)
    char why[160];              // the refusal in words
};
// BatchNorm-backward prologue: A[m,k] = k1*(dz - k2 - xhat*k3), dz = (A view, gathered through the shuffle map when
// shuffle_ctot != 0) masked by ReLU6 of the BN output when act == ACT_RELU6, xhat from the BN's raw input y [M][K].
struct PwBnBwd {
    const float* y;
    const float* stats;     // [4][G][K]
    const float* coef;      // [3][G][K]
    int shuffle_ctot;
    int act;
    double* part2;          // optional [G][nbpg][K]: column sums of the transformed A (bias gradient partials)
};
// A: the operand view -- with the BatchNorm-backward prologue (pro == 2) the dz view, and y = that prologue's raw BatchNorm input
PwNnPlan pw_nn_plan(View A, View C, int G, int Mg, int N, int K, int pro, int epi, int accumulate, bool packed, bool packed_bf16, int at,
                    bool has_part, const float* y = nullptr);
// the shape-only reads of the plan: dense, aligned views, no prologue / epilogue
inline PwNnPlan pw_nn_shape_plan(int G, int Mg, int N, int K) { return pw_nn_plan(make_view(nullptr, K), make_view(nullptr, N), G, Mg, N, K, 0, 0, 0, false, false, 0, false); }
inline bool pw_nn_supported(View A, int N, int K) { return pw_nn_plan(A, make_view(nullptr, N), 1, 1, N, K, 0, 0, 0, false, false, 0, false).ok; }
// Wp (optional): B pre-packed in MFMA fragment order by pw_pack_many (pw_packed_elems(N, K) floats)
// wp_bf16: Wp holds bf16 fragments (PwPack::bf16) -> bf16-operand variant (both MFMA operands rounded to bf16, float32
// tensors / accumulation / statistics: the compute mode of configuration 3)
int pw_nn(View A, const float* pro_stats, const float* W, int sbk, int sbn, const float* bias, View C, int accumulate, int G,
          int Mg, int N, int K, int epilogue, const float* ey, const float* epi_stats, double* part, hipStream_t st,
          const PwBnBwd* bnbwd = nullptr, const float* Wp = nullptr, bool wp_bf16 = false, int at = 0);
struct PwPack {             // one operand to pack: B(k, n) = w[k * sbk + n * sbn], K x N
    const float* w;
    float* wp;
    int K, N, sbk, sbn, ksm, ntiles;
    int bf16;               // 1: bf16 fragments of the bf16-operand variant (same element count, half the bytes)
};
int64_t pw_packed_elems(int N, int K);
PwPack pw_pack_entry(const float* w, float* wp, int K, int N, int sbk, int sbn, bool bf16 = false);
int pw_pack_many(const PwPack* tab_dev, int n, hipStream_t st);
// out[i] (+)= sum_p part[p*stride + i] for float partials (double accumulation, fixed order)
// The kernel is chosen by reduce_partials_f32_plan (address arithmetic only): form 0 tn_reduce_few_kernel, 1 / 2 / 3
// tn_reduce_v4_kernel<16 / 4 / 1>, 4 / 5 tn_reduce_kernel<16 / 4> (any alignment, any n)
struct ReduceF32Plan {
    int form;
    unsigned grid;
    int bx, by;                 // block
};
ReduceF32Plan reduce_partials_f32_plan(uintptr_t part_addr, int nparts, int64_t n, int64_t stride);
int reduce_partials_f32(const float* part, int nparts, int64_t n, int64_t stride, float* out, int accumulate,
                        hipStream_t st);

// ---------------------------------------------------------------- convolutions (conv.hip)
// x: (B,T,H,W,3) reference layout -> y: [(t*B+b)][Ho][Wo][Cout], 3x3 stride 2 valid.
int stem_fwd(const float* x, const float* w, const float* bias, float* y, int B, int T, int H, int W, int Cout,
             hipStream_t st);
// stem conv + (sum, sum^2) partials of its output per time slice: part [T][nb][2][Cout], nb = stem_fwd_stats_nb()
bool stem_fwd_stats_supported(int Cout);
int stem_fwd_stats_nb(int B, int T, int H, int W, int Cout);
int stem_fwd_stats(const float* x, const float* w, const float* bias, float* y, double* part, int B, int T, int H, int W, int Cout,
                   hipStream_t st, int at = 0);
int64_t stem_bwd_part_elems(int B, int T, int H, int W, int Cout);
// Geometry of the band form of stem_fwd_stats (conv.hip: stem_fwd_band_kernel takes it by value)
struct StemFwdGeom {
    int R, NB, nbpg, xs_floats, px;     // band rows, bands per frame, workgroups per time slice, LDS floats of a band, 16-byte chunks per thread
    size_t lds;
    bool ok;
};
// Pool forward / scatter-form BatchNorm sums of the stem block: the geometry their launchers (maxpool_bn_fwd in conv.hip,
// pool_bn_bwd_reduce in bn.hip) dispatch on, as functions of (rows, C) only
inline VColGeom stem_pool_fwd_geom(int rows, int C) { return vcol_geom(rows, C, 4096); }
struct PoolReducePlan {
    int form;       // 1: pool_bn_bwd_reduce_v4_kernel (4 channels per thread, one channel-lane pass), 0: the generic vcolreduce skeleton
    int pooled;     // the v4 kernel takes mask and xhat from the pooled activated output (ps.pa given)
    VColGeom g;
};
inline PoolReducePlan pool_bn_reduce_plan(int Mg, int C, bool has_pooled) {
    PoolReducePlan p;
    p.g = vcol_geom(Mg, C, NB_STATS);
    p.form = p.g.vec == 4 && p.g.nloop == 1;
    p.pooled = p.form && has_pooled;
    return p;
}
// Every host decision of the stem block conv 3x3/s2 'valid' -> BatchNorm + ReLU6 -> max-pool 3x3/s2 'same' in one place: stem_fwd,
// stem_fwd_stats(_nb), maxpool_bn_fwd, pool_bn_bwd_reduce, stem_bwd_filter(_fused) and the workspace queries take theirs from here, and
// cdrl_stem_plan reports the struct.  A function of the shape, the storage type and three facts about the pointers; reads no memory.
enum { STEM_REFUSE_COUT = 1, STEM_REFUSE_2GB = 2, STEM_REFUSE_ALIGN = 3 };
struct StemPlan {
    int Ho, Wo, Hp, Wp;                 // conv output, pooled output
    int fwd_vec;                        // stem_fwd: 1 four channels per thread, 0 stem_fwd_scalar_kernel (Cout % 4 or y not 16-byte aligned)
    int st_refusal;                     // stem_fwd_stats: 0, STEM_REFUSE_COUT (Cout % 4 or > 64), STEM_REFUSE_ALIGN
    int st_form;                        // 0 stem_fwd_band_kernel, 1 stem_fwd_stats_kernel (window form)
    int R, NB, nbpg, px, NP, lds;       // band: rows, bands per frame, workgroups per slice, 16-byte chunks per thread; pixels per thread; LDS bytes
    int units_max;                      // (frame, band) units the busiest workgroup walks (window form: 1 row range)
    int st_rb;                          // window form: rows per workgroup
    int part_rows;                      // rows of the [T][part_rows][2][Cout] partials
    StemFwdGeom geom;
    VColGeom pf;                        // maxpool_bn_fwd
    PoolReducePlan pr;                  // pool_bn_bwd_reduce
    int64_t pr_part_doubles;            // T * pr.g.nb * 2 * Cout
    int fg_form;                        // stem_bwd_filter: 0 stem_bwd_mfma_kernel<false>, 2 column reduce (Cout > 32)
    int ff_refusal;                     // stem_bwd_filter_fused: 0, STEM_REFUSE_COUT (Cout % 4 or > 32), STEM_REFUSE_2GB
    int ff_form;                        // 1 stem_bwd_mfma_kernel<true>, -1 refused
    int NCH;                            // 16-byte channel chunks per half-wave lane of the fused kernel (unfused: 1)
    int ff_rowstats;                    // fused: 1 the form that reads its slice's seven values per row (slices_max > 2), 0 two staged slices
    int rows_per, nblk;                 // rows per workgroup, workgroups (column reduce: rb, nb of col_geom)
    int slices_max;                     // time slices the rows of one workgroup can come from
    int single_reduce;                  // fused: db == dw + 27 * Cout, one reduce over the 28 * Cout columns
    int64_t part_doubles, ws_doubles;   // workspace doubles the filter gradient writes / stem_bwd_part_elems
};
StemPlan stem_plan(int B, int T, int H, int W, int Cout, int at, bool pooled, bool db_adjacent, bool y_aligned);
// stem filter gradient with the stem BatchNorm's backward apply + max-pool gather fused into the operand load (dy is
// never materialised); y: raw stem conv output, stats/coef: the stem BN's [4|3][T][Cout] blocks
bool stem_bwd_fused_supported(int Cout);
int stem_bwd_filter_fused(const float* x, const PoolSrc& ps, const float* y, const float* stats, const float* coef, float* dw,
                          float* db, int B, int T, int H, int W, int Cout, double* part, hipStream_t st, int at = 0);
int stem_bwd_filter(const float* x, const float* dy, float* dw, float* db, int B, int T, int H, int W, int Cout,
                    double* part, hipStream_t st);
// depthwise 3x3, TF 'SAME' (asymmetric) padding, stride 1|2.  N = frames.
int dw_fwd(View a, const float* w, const float* bias, float* y, int N, int H, int W, int C, int stride,
           hipStream_t st);
int dw_bwd_data(const float* dy, const float* w, View da, int N, int H, int W, int C, int stride, int accumulate,
                hipStream_t st);
// dw_bwd_data fused with the BatchNorm-backward reduction of the layer that produced the depthwise input
// (a = act(bn(y_pre))): writes da AND the per-group partial sums (sum dz, sum dz*xhat) of that BN.
int dw_bwd_data_bnreduce(const float* dy, const float* w, View da, int N, int H, int W, int C, int stride, int G,
                         const float* y_pre, const float* stats_pre, int act_pre, double* part, hipStream_t st);
int64_t dw_bwd_part_elems(int N, int H, int W, int C, int stride);
int dw_bwd_filter(View a, const float* dy, float* dw, float* db, int N, int H, int W, int C, int stride,
                  double* part, hipStream_t st);
// ---- fused depthwise block (dwfused.hip): whole frames staged in LDS.  G groups x B frames per group.
// Every host decision of the family is one DwfPlan filled by dwf_plan: dwf_fwd / dwf_bwd launch from it, the engine
// and the op-level entry points size their partial rows and workspaces from it, cdrl_dwconv_bn_plan reports it.
// strip form of the backward (round 5): thread = channel pair x row strip of `sw` pixels; ok == false (every field 0) -> pixel-mapped
struct DwsGeom {
    bool ok = false;
    int sw = 0, S = 0, R = 0, F = 0;           // S strips per row, R strips per thread and tile batch (stride 1), F frames per tile batch
    int cchunk = 0, nch = 0, cx = 0, cy = 0;   // channels per chunk, chunks per frame, channel-pair lanes x strip lanes
    int wdp = 0, tile_floats = 0;              // padded tile width (stride 2; 0 for stride 1), floats of the D tile
    size_t lds = 0;
};
// a tile over this even at the smallest channel chunk is refused (forward, pixel-mapped backward)
static constexpr size_t DWF_LDS_LIMIT = 150 * 1024;
enum DwfRefusal {
    DWF_OK = 0,
    DWF_REFUSE_STRIDE = 1,      // stride is not 1 or 2
    DWF_REFUSE_LDS = 2,         // the frame's tile exceeds DWF_LDS_LIMIT
    DWF_REFUSE_OFFSETS = 3,     // strip forms: a gradient view of 2 GB or more (32-bit buffer offsets)
};
struct DwfLaunch {              // what one direction launches
    int refusal = DWF_OK;
    int form = 0;               // backward: 0 pixel-mapped, 1 stride-1 strips, 2 stride-2 strips; forward: 0
    int a0 = 0, a1 = 0;         // the form's template arguments: (stride, VEC) | (SW, R) | (PL, 0)
    int grid = 0, bx = 0, by = 0;
    size_t lds = 0;
};
struct DwfPlan {
    int G = 0, B = 0, H = 0, W = 0, C = 0, stride = 0, dx_ld = 0;
    int Ho = 0, Wo = 0, pt = 0, pl = 0;                        // 'same' output size and top / left padding at `stride`
    int vec = 0, nch = 0, cchunk = 0, cx = 0, cy = 0;          // forward lanes; nch, cchunk also of the pixel-mapped backward
    int fpb = 0, nb = 0;                                       // forward: frames per workgroup, partial rows per group (B / fpb)
    int vec_bwd = 0, cx_bwd = 0, cy_bwd = 0;                   // pixel-mapped backward lanes (fewer channels per thread: register budget)
    size_t lds_fwd = 0, lds_bwd = 0;                           // tiles of the forward / the pixel-mapped backward
    bool lds_bwd_over = false;                                 // lds_bwd > DWF_LDS_LIMIT, whichever form runs
    int fpb_bwd = 0, nb_bwd = 0;                               // backward, the form that runs: frames per workgroup, partial rows per group
    DwsGeom strip;
    DwfLaunch fwd, bwd;
    int64_t stats_part_elems = 0, filter_part_elems = 0;       // doubles: [G][max(nb, nb_bwd)][2 | 10][C], either direction fits
};
// dx_ld: leading dimension of the gradient view the backward writes (0: dense, C)
DwfPlan dwf_plan(int B, int G, int H, int W, int C, int stride, int dx_ld = 0);
int dwf_refuse(const char* who, const DwfPlan& p, int refusal);      // sets the refusal's message, returns -1
// y = dw3x3(pre_stats ? relu6(scale*x+shift) : x) + bias and the per-block (sum y, sum y^2) partials of the
// BatchNorm that follows (layout of bn_finalize with nb = plan.nb).
struct DwfFwdArgs {
    const float *x, *pre_stats, *w, *bias;
    float* y;
    double* part;
    hipStream_t st;
    int at;
};
int dwf_fwd(const DwfPlan& p, const DwfFwdArgs& a);
// dout: gradient w.r.t. the output of the BatchNorm (no activation) that follows the depthwise conv; y2: the raw
// depthwise output; post_stats / post_coef: that BN's statistics and backward coefficients (k1,k2,k3).
// Writes the filter / bias partials (part_w: reduce with reduce_partials over G*nb_bwd parts, row stride 10*C) and
//   pre_stats != null: dx = ReLU6-masked gradient at the pre-BN's output + its (sum dz, sum dz*xhat) partials
//   pre_stats == null: dx = gradient w.r.t. x.
struct DwfBwdArgs {
    const float *x, *pre_stats, *dout, *y2, *post_stats, *post_coef, *w;
    View dx;                    // no wider than the plan's dx_ld
    double *part_bn, *part_w;
    hipStream_t st;
    int at;
};
int dwf_bwd(const DwfPlan& p, const DwfBwdArgs& a);
int maxpool_fwd(const float* a, float* p, uint8_t* argmax, int N, int H, int W, int C, hipStream_t st);
int maxpool_bwd(const uint8_t* argmax, const float* dp, float* da, int N, int H, int W, int C, hipStream_t st);
// fused BN-apply + ReLU6 + max-pool on the raw conv output y (frames of group g = [g*frames_per_group, ...))
int maxpool_bn_fwd(const float* y, const float* stats, int G, int frames_per_group, float* p, uint8_t* argmax, int N,
                   int H, int W, int C, hipStream_t st, int at = 0);
PoolSrc make_pool_src(const uint8_t* argmax, const float* dp, int H, int W);
// out[n][c] = mean_p act(scale[g][c] * y[n*P + p][c] + shift[g][c]): BatchNorm apply + activation + global average pool fused
int bn_act_gap_fwd(const float* y, const float* stats, float* out, int G, int frames_per_group, int P, int C, int act, hipStream_t st,
                   int at = 0);

// batched transposes W[cin][cout] -> WT[cout][cin] of many small matrices in one launch (gemm.hip)
struct PwTranspose {
    const float* w;
    float* wt;
    int cin, cout;
};
// one launch: grid = (tiles, n) with tiles >= max over the entries of ceil(cin/32) * ceil(cout/32)
int transpose_many(const PwTranspose* tab_dev, int n, int tiles, hipStream_t st);

// ---------------------------------------------------------------- float32 pointwise conv on the bf16 matrix pipe (gemm_pw_x3.hip)
// exact 3-way bf16 split of both operands, six bf16 MFMAs per K = 16 step, float32 in / out; W packed by pw_x3_pack_many
struct PwX3Pack {
    const float* w;
    __bf16* wp;
    int K, N, sbk, sbn, kp;
};
// What pw_x3 launches: form 0 the persistent kernel pw_x3_kernel<KP, NT, PRO, EPI> (K, N <= 128), form 1 pw_x3_wide_kernel<PRO, EPI>
// (K or N above 128: one 32-row tile per workgroup, column blocks of 128, KP = 256).  Alignment per form: both need a 16-byte aligned
// pointer; form 0 even K / leading dimension / channel offset (16-byte buffer loads need dword alignment only, columns beyond K inside
// the last chunk are zeroed), form 1 multiples of 4.  form / kp / nt are filled before anything is refused.
enum PwX3Refusal {
    PWX3_OK = 0,
    PWX3_REFUSE_DIMS = 1,       // G < 1, Mg < 1 or N < 1
    PWX3_REFUSE_SHAPE = 2,      // K below 4 or above 256, N above 256, K odd (form 0) / not a multiple of 4 (form 1)
    PWX3_REFUSE_ALIGN = 3,
    PWX3_REFUSE_PACKED = 4,     // no packed weights
    PWX3_REFUSE_2GB = 5,
    PWX3_REFUSE_NBPG = 6,       // a caller-supplied workgroup count outside [1, tiles] (form 1: other than tiles)
    PWX3_REFUSE_COUNT = 7,
};
struct PwX3Plan {
    int ok, refusal;
    int form, kp, nt, pro, epi;
    int bm, tiles_g, nbpg;      // nbpg = partial rows per group
    int gx, gy;
    int64_t packed_bytes;
    char why[160];
};
PwX3Plan pw_x3_plan(View A, View C, int G, int Mg, int N, int K, bool pro, bool epi, bool packed, int nbpg = 0);
inline int pw_x3_partial_rows(int G, int Mg, int N, int K) { return pw_x3_plan(make_view(nullptr, K), make_view(nullptr, N), G, Mg, N, K, false, false, true).nbpg; }
int64_t pw_x3_packed_bytes(int K);                 // N <= 128 (one column block)
int pw_x3_ksteps(int K);                           // K = 16 steps per plane of that pack
int64_t pw_x3_packed_bytes_n(int K, int N);        // any N <= 256: column blocks of 128
PwX3Pack pw_x3_pack_entry(const float* w, void* wp, int K, int N, int sbk, int sbn);
int pw_x3_pack_many(const PwX3Pack* tab_dev, int n, hipStream_t st);
// nbpg > 0: workgroups (= partial rows) per group chosen by the caller (the engine keeps pw_nn_plan's count)
// backward-data of the wide convs (128 < K or N <= 256) with the BatchNorm-backward prologue, one 32-row tile per workgroup: C[M][N] (+)=
// dy W^T, Wp = pw_x3_pack_entry(W, wp, K, N, 1, K) (B(k = conv output channel, n = conv input channel)); one part2 / part row per tile.
// pw_x3_wide_bwd_kernel<SH, EPI, ACC>; N = conv input channels (columns of the output), K = conv output channels (columns of dz / y).
// Alignment: dz 16-byte aligned with an even leading dimension; dense dz multiples of 4 in leading dimension and offset (one 16-byte
// load per chunk), shuffled dz an even offset and an even half width (8-byte loads of adjacent source pairs).
enum PwX3BwdRefusal {
    PWX3B_OK = 0,
    PWX3B_REFUSE_DIMS = 1,      // G < 1 or Mg < 1
    PWX3B_REFUSE_SHAPE = 2,     // neither K nor N above 128, one above 256, K not a multiple of 4
    PWX3B_REFUSE_ALIGN = 3,
    PWX3B_REFUSE_OPERANDS = 4,  // packed weights, y, stats or coef missing
    PWX3B_REFUSE_EPI_ACC = 5,   // epilogue and accumulate are not instantiated together
    PWX3B_REFUSE_2GB = 6,
    PWX3B_REFUSE_COUNT = 7,
};
struct PwX3BwdPlan {
    int ok, refusal;
    int sh, epi, acc;
    int rows;                   // 32-row tiles per group = part2 / part rows per group
    int gx, gy;
    char why[160];
};
PwX3BwdPlan pw_x3_wide_bwd_plan(View dz, View C, int G, int Mg, int N, int K, int shuffle_ctot, bool epi, int accumulate, bool operands);
inline int pw_x3_wide_bwd_rows(int Mg) { return pw_x3_wide_bwd_plan(make_view(nullptr, 4), make_view(nullptr, 4), 1, Mg, 0, 0, 0, false, 0, true).rows; }
int pw_x3_wide_bwd(View dz, const PwBnBwd& bb, const void* Wp, View C, int accumulate, int G, int Mg, int N, int K, const float* ey,
                   const float* epi_stats, double* part, hipStream_t st);
int pw_x3(View A, const float* pro_stats, const void* Wp, const float* bias, View C, int G, int Mg, int N, int K, double* part,
          hipStream_t st, int nbpg = 0);


// ---------------------------------------------------------------- fused backward of a pointwise conv (gemm_pw_bwd.hip)
// ONE pass over (dz, y, a): BatchNorm-backward apply on load, da = dy W^T, Q = a^T dy (or xhat(a)^T dy), db partials; then
// pw_bwd_fused_reduce: dW, db and -- when a is a BatchNorm output applied on load (a_stats) -- that BatchNorm's backward sums
// (dgamma, dbeta, coefficients) from Q, with no pass over da.  Float32 tensors, float32-accurate (three-way bf16 operand split).
struct PwBwdFused {
    View dz;                // gradient w.r.t. the output of the BatchNorm behind the conv
    int dz_shuffle = 0;     // channel-shuffle gather on the dz columns (ctot), 0 = none
    int act = 0;            // ACT_RELU6: mask from that BatchNorm's output
    const float* y = nullptr;       // raw conv output [G*Mg][N] dense
    const float* stats = nullptr;   // [4][G][N] of that BatchNorm
    const float* coef = nullptr;    // [3][G][N] backward coefficients (bn_bwd_finalize)
    View a;                 // conv input [G*Mg][K]
    const float* a_stats = nullptr; // [4][G][K]: a = BatchNorm(a_raw) applied on load (no activation); null: plain input
    const float* a_gamma = nullptr; // with a_stats: parameters / gradient outputs of that BatchNorm
    const float* a_beta = nullptr;
    float* a_dgamma = nullptr;
    float* a_dbeta = nullptr;
    float* a_coef = nullptr;        // [3][G][K]
    const float* W = nullptr;       // conv weights [K][N]
    const void* Wp = nullptr;       // pw_x3 packing of B(k = n_out, n = k_in) = W[n * N + k]  (pw_x3_pack_entry(W, wp, N, K, 1, N))
    View da;                // gradient w.r.t. the conv input (the raw a for a_stats: gradient w.r.t. the BatchNorm OUTPUT)
    int accumulate = 0;
    float* dW = nullptr;    // [K][N]
    float* db = nullptr;    // [N]
    float* qpart = nullptr; // pw_bwd_fused_qpart_elems floats
    double* dbpart = nullptr;       // pw_bwd_fused_dbpart_elems doubles
    int N = 0, K = 0, G = 1, Mg = 0;
    int at = 0;             // 1: dz, y, a, da are bf16 in HBM (bf16 activation storage; one bf16 plane per MFMA operand)
    // float32 form, optional: the finalize of the BatchNorm behind the conv on load (no bn_bwd_finalize launch in front, `coef` unused):
    // fin_part = its [G][fin_nb][2][N] backward sums, fin_tot = [G][2][N] doubles of scratch, o_dgamma / o_dbeta [N] written by the reduce
    const double* fin_part = nullptr;
    double* fin_tot = nullptr;
    int fin_nb = 0;
    float* o_dgamma = nullptr;
    float* o_dbeta = nullptr;
};
// What pw_bwd_fused / pw_bwd_fused_reduce launch for a call, and why they refuse one (pw_bwd_fused_plan: the launchers, the size queries
// below and cdrl_pwconv_bwd_plan all take their numbers from it; nothing launches for a call it refuses).
enum PwbRefusal {
    PWB_OK = 0,
    PWB_REFUSE_SHAPE = 1,       // K or N odd, outside 8..128, or padded 128 -> 64; G or Mg < 1
    PWB_REFUSE_ALIGN = 2,       // odd leading dimension / channel offset, pointer not 8-byte aligned
    PWB_REFUSE_PADDING = 3,     // bf16 storage: K and N padded differently
    PWB_REFUSE_2GB = 4,         // an operand of 2 GB or more (32-bit buffer offsets)
    PWB_REFUSE_GROUPS = 5,      // G > 8 (the reduce kernel's slots)
    PWB_REFUSE_FIN = 6,         // finalize-on-load under bf16 storage, without fin_tot / fin_nb, or without o_dgamma / o_dbeta
    PWB_REFUSE_ANORM = 7,       // a_stats without gamma / beta or the dgamma / dbeta / coef outputs
};
struct PwbPlan {
    int ok, refusal;
    int form;                   // 0: float32 tensors (pwb_kernel), 1: bf16 storage (pwb16_kernel)
    int kp, np, bm;             // padded input / output channels, rows per tile
    int tiles, nbpg;            // tiles per group, workgroups (= partial tiles) per group
    int wp_ks;                  // K = 16 steps per plane of the packed W^T
    int shuf, anorm, acc, fin;  // the instantiation's template flags; fin: finalize-on-load (a kernel argument)
    int coef_needed;            // 0 with fin: k1 comes from the statistics block, k2 / k3 from fin_part -- `coef` is never read
    int lds_bytes;              // dynamic LDS of the main kernel
    int64_t qpart_elems, dbpart_elems;      // workspace sizes in floats / doubles
    int64_t spart_offset;       // doubles into dbpart where the directly accumulated BatchNorm sums start (bf16 storage + a_stats), else 0
    char why[192];              // the refusal in words
};
PwbPlan pw_bwd_fused_plan(const PwBwdFused& f);
bool pw_bwd_fused_supported(View dz, View a, View da, int N, int K, int at = 0);
int pw_bwd_fused_nbpg(int G, int Mg, int N, int K, int at = 0);
int64_t pw_bwd_fused_qpart_elems(int G, int Mg, int N, int K, int at = 0);
int64_t pw_bwd_fused_dbpart_elems(int G, int Mg, int N, int K, int at = 0);
int pw_bwd_fused(const PwBwdFused& f, hipStream_t st);
int pw_bwd_fused_reduce(const PwBwdFused& f, hipStream_t st);

// general form (gemm_x3.hip): any K (multiple of 4), any N; B packed once per pass by gemm_x3_pack_many into [3][K/16][2][Npad][8]
struct GemmX3Pack {
    const float* w;
    __bf16* wp;
    int K, N, sbk, sbn, KS, NP;
};
bool gemm_x3_supported(View A, int K);
int64_t gemm_x3_packed_bytes(int N, int K);
GemmX3Pack gemm_x3_pack_entry(const float* w, void* wp, int K, int N, int sbk, int sbn);
int gemm_x3_pack_many(const GemmX3Pack* tab_dev, int n, hipStream_t st);
// every pack table of a training pass + the W^T transposes of its backward in ONE launch (gemm_pw.hip, pack_bodies.h)
int pack_all(const GemmX3Pack* tg, int ng, const PwPack* tp, int np, const PwX3Pack* t3, int n3, const PwTranspose* tt, int nt,
             int transpose_tiles, hipStream_t st);
// bf16_operands: one product per step on the first plane only (operands rounded to bf16: configuration 3's compute mode)
int gemm_x3(View A, const void* Bp, const float* bias, View C, int M, int N, int K, int accumulate, hipStream_t st,
            bool bf16_operands = false, int at = 0);

// ---------------------------------------------------------------- bf16 pointwise conv (gemm_pw_bf16.hip)
// bf16 activations (A, C), float32 master weights / bias / BatchNorm blocks, bf16 MFMA with float32 accumulate; optional
// BN-apply prologue (pro_stats [4][G][K]) and statistics epilogue (part [G][nbpg][2][N], nbpg = pw_bf16_partial_rows)
bool pw_bf16_supported(int lda, int a_coff, int N, int K);
int pw_bf16_partial_rows(int G, int Mg, int N, int K);
// Wp (optional): the weights pre-packed as bf16 MFMA fragments by pw_bf16_pack (pw_bf16_packed_elems(K) bf16 elements)
int pw_bf16(const void* A, int lda, int a_coff, const float* pro_stats, const float* W, const float* bias, void* C, int ldc,
            int c_coff, int G, int Mg, int N, int K, double* part, hipStream_t st, const void* Wp = nullptr);
int64_t pw_bf16_packed_elems(int K);
int pw_bf16_pack(const float* W, int K, int N, void* Wp, hipStream_t st);
int f32_to_bf16(const float* x, void* y, int64_t n, hipStream_t st);
int bf16_to_f32(const void* x, float* y, int64_t n, hipStream_t st);

// ---------------------------------------------------------------- linear output heads (heads.hip)
#define HEADS_MAX 4
#define HEADS_MAX_OUT 8
struct HeadSet {
    int nheads;
    int n[HEADS_MAX], off[HEADS_MAX];      // outputs of head h and its first column in lin
    const float* w[HEADS_MAX];             // [K][n]
    const float* b[HEADS_MAX];             // [n]
    float* gw[HEADS_MAX];                  // gradients (null for inference-only heads)
    float* gb[HEADS_MAX];
};
// lin[b][off_h + n] = b_h[n] + sum_k a[b][k] W_h[k][n]   (a: [B][lda], lin: [B][ldl])
int heads_fwd(const float* a, int lda, const HeadSet& hs, float* lin, int ldl, int B, int K, hipStream_t st);
// da[b][k] = sum_c dlin[b][c] W[k][c] (overwrite; da may be null), dW_h = a^T dlin_h, db_h = column sums of dlin_h
int heads_bwd(const float* a, int lda, const HeadSet& hs, const float* dlin, int ldl, float* da, int ldda, int B, int K,
              hipStream_t st);

// ---------------------------------------------------------------- GRU (rnn.hip)
// gates of step t: xp,hp [B][3u]; hprev [B][u]; saves z,r,hh; writes hnew
// one fused kernel per GRU time step and direction (rnn.hip): recurrent product + gate math / gate derivatives + product
// against R^T; `out` (optional) is a second destination of h_new, `dh` a strided view, dhprev == null for the first step
bool gru_step_supported(int u);
int gru_step_fwd(const float* xp, const float* hprev, const float* R, const float* b1, float* z, float* r, float* hh, float* hp,
                 float* hnew, View out, int B, int u, hipStream_t st);
int gru_step_bwd(View dh, const float* z, const float* r, const float* hh, const float* hp, const float* hprev, const float* RT,
                 float* dxp, float* dhp, float* dhprev, int B, int u, hipStream_t st);

// ---------------------------------------------------------------- losses (loss.hip)
struct PolicyLossArgs {
    const float* lin;        // [B][2A+2] linear head outputs: alpha_pre(A) beta_pre(A) similarity_pre speed_pre
    const float* adv;        // [B]
    const float* old_logp;   // [B][A]
    const float* speed;      // [B]
    const float* similarity; // [B]
    const float* u;          // [B][A] Beta samples (or stored actions)
    const float* du_da;      // [B][A] or nullptr
    const float* du_db;      // [B][A] or nullptr
    const float* hp;         // device hyper-parameter block (DevHP)
    float* dlin;             // [B][2A+2]
    float* metrics;          // [16]
    float* aux;              // optional [B][4A]: alpha, beta, log_prob, entropy
    int B, A;
    float inv_world;         // gradient scale for data-parallel averaging (1/world_size)
};
int policy_loss(const PolicyLossArgs& a, hipStream_t st);
struct CloneLossArgs {       // behaviour cloning: weighted Beta negative log-likelihood of expert actions
    const float* lin;        // [B][2A+2] as PolicyLossArgs::lin
    const float* u;          // [B][A] expert action in the unit interval
    const float* weight;     // [B] or nullptr (= 1)
    const float* speed;      // [B] or nullptr; speed and similarity come together
    const float* similarity; // [B] or nullptr
    const float* hp;         // device hyper-parameter block (DevHP) whose entropy_coef is read, or nullptr: entropy_coef below
    float entropy_coef, aux_weight;
    float* dlin;             // [B][2A+2]
    float* metrics;          // [16]; 0..7 written: total, clone, entropy, speed, similarity, mean weight, mean logp, mode error
    float* aux;              // optional [B][4A]: alpha, beta, log_prob, entropy
    int B, A;
    float grad_scale;
};
int clone_loss(const CloneLossArgs& a, hipStream_t st);
// Mixed policy loss (demo.hip): row b is a demonstration row iff demo_w[b] > 0 -- weighted negative Beta
// log-likelihood of demo_u[b], averaged over the ND such rows; its adv / old_logp / u / du_da / du_db are not read -- and a PPO row
// otherwise (the surrogate of policy_loss, averaged over the NP = B - ND others).  Entropy and auxiliary terms over all B rows.
struct MixedPolicyLossArgs {
    PolicyLossArgs ppo;      // metrics: 0..6 as policy_loss ([1], [5], [6] over the PPO rows), [7] demonstration term, [8] mean logp and
                             // [9] mean absolute mode error of the demonstration rows, [10] ND
    const float* demo_u;     // [B][A] expert action in the unit interval
    const float* demo_w;     // [B]
    DemoBlock* block;        // device block that thread 0 adds metrics[7..10] and a pass count to; or null
};
int mixed_policy_loss(const MixedPolicyLossArgs& a, hipStream_t st);
// Trust-region guard (trust.hip): the analytic KL(Beta(anchor) || Beta(policy)) of a policy minibatch, summed over a
// row's actions and averaged over the rows, behind policy_loss and in front of the head's backward.
struct BetaKlArgs {
    const float* lin;        // [B][2A+2] as PolicyLossArgs::lin
    const float* anchor;     // [B][2][A] alpha0, beta0 of the anchor policy
    float* dlin;             // [B][2A+2], accumulated onto when the coefficient is positive; may be null when it is zero
    TrustBlock* trust;       // device block: coefficient and thresholds read from it, statistics and latch written; or null ...
    float kl_coef;           // ... then this coefficient, and nothing but metrics / dlin is written
    float* metrics;          // [3] KL (clamped below at 0), its maximum over the rows, KL / A; or null
    int B, A;
    float inv_world;
};
int beta_kl(const BetaKlArgs& a, hipStream_t st);
int trust_disarm(TrustBlock* trust, hipStream_t st);       // armed = 0, one thread
// the host-written head, passed to the kernel by value (the caller's values may change as soon as the call returns)
int trust_set_params(TrustBlock* trust, float target_kl, float kl_stop_factor, float kl_coef, hipStream_t st);
int trust_reset(TrustBlock* trust, hipStream_t st);        // the device-owned fields to their initial values, one thread
struct ValueLossArgs {
    const float* lin;        // [B][4]: base_pre, exp_pre, speed_pre, similarity_pre
    const float* returns;    // [B][2]
    const float* speed;
    const float* similarity;
    float* dlin;             // [B][4]
    float* metrics;          // [16]
    float* values;           // optional [B][2]
    int B;
    float exp_scale;
    float inv_world;
};
int value_loss(const ValueLossArgs& a, hipStream_t st);
// NT-Xent over pairs of views (ntxent.hip; no reference counterpart): rows i and (i + B/2) mod B of z are the two
// views of one observation.  B even, 2 .. 2048; D >= 1; temperature > 0 (-1 and cdrl_last_error otherwise).
struct NtxentArgs {
    const float* z;          // [B][D] embeddings
    float* dz;               // [B][D] grad_scale * dL/dz, every entry written; not z
    float* metrics;          // [16]; 0..5 written (loss, top-1 accuracy, pair cosine, negatives' cosine, mean norm, temperature), 6..15 zero
    float* workspace;        // ntxent_workspace_floats(B, D) floats, 16-byte aligned
    int B, D;
    float temperature, grad_scale;
};
int64_t ntxent_workspace_floats(int B, int D);      // -1: B or D refused
int ntxent_loss(const NtxentArgs& a, hipStream_t st);
// inference heads: alpha,beta,(mean,std) and value(base,exp) from linear outputs
int policy_dist(const float* lin, float* out /*[B][4A]: alpha,beta,mean,std*/, int B, int A, hipStream_t st);
int value_act(const float* lin, float* out /*[B][4] base,exp,speed,sim*/, int B, float exp_scale, hipStream_t st);

// ---------------------------------------------------------------- Beta sampling (sample.hip)
// u ~ Beta(alpha, beta) (as a Gamma ratio) with pathwise derivatives du/dalpha, du/dbeta (implicit
// reparameterisation of the two Gamma samples).  Element (row, col): alpha[row*ld + col].
int beta_sample(const float* alpha, const float* beta, int rows, int A, int ld, uint64_t seed, uint64_t offset, float* u,
                float* du_da, float* du_db, hipStream_t st, float* logp = nullptr, double* gammas = nullptr);
// evaluation-time action from the predict block dist [rows][4][A] (mode 0: the sample of beta_sample, 1: the mode of the Beta), its
// log-density, and per-row running sums for the active rows (stats [rows][3A + 2] doubles, may be null); arguments checked here
int beta_act(const float* dist, const float* value, int rows, int A, int mode, uint64_t seed, uint64_t offset, const int32_t* active,
             float* action, float* logp, double* stats, hipStream_t st);
int gamma_implicit_grad(const double* a, const double* g, int n, double* out, hipStream_t st);
int philox_words(uint64_t seed, uint64_t offset, uint64_t idx0, int n, int nblocks, uint32_t* out, hipStream_t st);

// ---------------------------------------------------------------- rollout-time augmentation (augment.hip)
struct AugPlan {           // same layout as cdrl_aug_plan (include/cdrl.h)
    int jitter;
    float brightness, contrast, saturation, hue;
    int blur_size;
    float blur_kernel[75];
    int salt_pepper;
    float sp_amount, sp_prob;
    int gauss_noise;
    float gn_amount, gn_std;
    int normalize;
    int cutout_size, cutout_cell;
    int dropout_size;
    float dropout_amount;
    uint64_t seed, offset;
};
// in/out: [T][H][W][3] floats; workspace: 2*T*H*W*3 + 5*T floats
int augment_images(const float* in, float* out, int T, int H, int W, const AugPlan& plan, float* workspace, hipStream_t st);
// E stacks at once: in/out [E][T][H][W][3]; plans_dev: E plans IN DEVICE MEMORY (a blur_size outside {0, 3, 5} is treated as 0: the
// caller checks it before the upload); workspace: augment_batch_workspace_floats floats.  out[e] gets the bytes of
// augment_images(in[e], ..., plans[e]); five launches for any E (the environment is the grid's y dimension).
constexpr int AUG_BATCH_MAX_ENVS = 65535;
int64_t augment_batch_workspace_floats(int E, int T, int H, int W);
int augment_images_batch(const float* in, float* out, int E, int T, int H, int W, const AugPlan* plans_dev, float* workspace,
                         hipStream_t st);

// ---------------------------------------------------------------- contrastive views (views.hip)
constexpr int VIEW_MAX_TAPS = 15;
struct ViewPlan {          // same layout as cdrl_view_plan (include/cdrl.h)
    int32_t crop_y, crop_x, crop_h, crop_w;
    int32_t flip;
    int32_t jitter;
    float brightness, contrast, saturation, hue;
    int32_t drop;
    int32_t blur_taps;
    float blur_w[16];
};
// rows [N][T][H][W][3] -> out [V][T][H][W][3], view v from row v % N with plans_dev[v] (DEVICE memory; contents validated by the
// caller before the upload: the kernels clamp a crop window into the frame and treat a tap count that is even or outside 3..15
// as 0); workspace: views_workspace_floats floats, may not overlap rows or out.  Four launches for any V.
int64_t views_workspace_floats(int V, int T, int H, int W);
int views_batch(const float* rows, int N, float* out, int V, int T, int H, int W, const ViewPlan* plans_dev, float* workspace,
                hipStream_t st);

// ---------------------------------------------------------------- occlusion saliency (explain.hip)
struct OcclusionRowsArgs {
    const float *image, *baseline;                  // [T][H][W][3] each
    const float *road, *vehicle, *navigation;       // [T][Dr], [T][Dv], [T][Dn]
    float* out_image;                               // [count][T][H][W][3]
    float *out_road, *out_vehicle, *out_navigation; // [count][T][D*]
    int T, H, W, Dr, Dv, Dn;
    int gh, gw, per_frame, modalities;
    int first, count;                               // rows [first, first + count) of the N rows; an index >= N is a copy of row 0
};
// one launch each; arguments checked here (-1 and cdrl_last_error)
int occlusion_baseline(const float* image, float* baseline, int T, int H, int W, int mode, hipStream_t st);
int occlusion_rows(const OcclusionRowsArgs& a, hipStream_t st);
// alpha, beta [N][A], value [N][2] (base, exponent) -> scores [N-1][2 + A] doubles: KL, value difference, mean shifts vs row 0
int occlusion_scores(const float* alpha, const float* beta, const float* value, int N, int A, double* scores, hipStream_t st);
// the first F*gh*gw rows of scores [.][K] -> maps [K][F][H][W]; upsample 0 nearest, 1 bilinear
int occlusion_maps(const double* scores, int K, int F, int gh, int gw, int H, int W, int upsample, int normalize, float* maps,
                   hipStream_t st);

// ---------------------------------------------------------------- scoring on held-out rows (score.hip)
struct BetaScoreArgs {
    const float* dist;          // [rows][4][A] alpha, beta, mean, std as learner_predict writes them (mean and std are not read)
    const float* value;         // [rows][4] base, exp, speed, similarity
    const float* u;             // [count][A] expert actions in the unit interval
    const float* returns_be;    // [count][2] (base, exp), or null
    const float *speed, *similarity;    // [count] each, both or neither
    int rows, count, A;         // the first count <= rows rows are scored
    double* block;              // score_block_doubles(A) doubles (score_block.h), read-modify-written
    double* pit;                // [count][A] or null: I_x(alpha, beta) of every scored element, NaN where it was not formed
};
// one launch of one workgroup; arguments checked here (-1 and cdrl_last_error)
int beta_score(const BetaScoreArgs& a, hipStream_t st);

// ---------------------------------------------------------------- optimiser (optim.hip)
// Device hyper-parameter block, refreshed by the host before each step (graph-replay safe).
struct DevHP {
    float lr_policy, lr_value, lr_dynamics;
    float clip_ratio, entropy_coef;
    float clip_norm_policy, clip_norm_value;   // <= 0 : no clipping
    float beta1, beta2, eps;
    int t_policy, t_value, t_dynamics;         // optimizer step counters (incremented on device)
    // Nadam's running product of the momentum schedule, one per optimizer (1 at the start; S_t of the last step).  Behind the
    // counters, so that an upload of the float block (upload_hp: up to t_policy) never overwrites it
    float m_cache_policy, m_cache_value, m_cache_dynamics;
};
struct TensorSeg {      // one parameter tensor inside a flat arena
    int64_t off;
    int64_t n;
    int first_chunk;    // index of its first 1024-element chunk in the chunk table
    int nchunks;
};
// Device half of a chunk table: the trainable tensors of one model cut into 1024-element chunks, one workgroup each.  An empty
// table (no list: the trunk's update, a learner without a trunk table) is ChunkTable{}.
struct ChunkTable {
    TensorSeg* segs = nullptr;
    int* chunk_tensor = nullptr;        // [nchunks] tensor of the chunk
    int64_t* chunk_off = nullptr;       // [nchunks] first element of the chunk, in the model's arena slice
    int ntensors = 0, nchunks = 0;
    double* chunk_part = nullptr;       // [nchunks] sum of squares of the chunk's gradient elements
};
// One model's trainable slice of the four flat arenas (weights, gradients, the optimizer's two slots), n elements.
struct ArenaSlice {
    float* p = nullptr;
    const float* g = nullptr;
    float* m = nullptr;
    float* v = nullptr;
    int64_t n = 0;
};
enum { WHICH_POLICY = 0, WHICH_VALUE = 1, WHICH_TRUNK = 2 };      // the optimizer whose DevHP fields a kernel reads
enum TickMask : int { TICK_POLICY = 1, TICK_VALUE = 2, TICK_TRUNK = 4, TICK_NADAM = 8 };
enum { NOT_TICKED = 0, TICKED = 1 };      // whether the optimizer's step counter was advanced before its update runs
// First stage of the deterministic two-stage norm: tab.chunk_part[c] = float64 sum of squares of chunk c of g (one launch).  Its
// block 0 also advances the step counters of tick_mask (TICK_*; | TICK_NADAM: and their m_caches to S_t of the new count).  The
// second stage, the per-tensor fold, runs inside the consumers (clip_update, stats_fold_norms).
int chunk_sqnorms_tick(const float* g, const ChunkTable& tab, DevHP* hp, int tick_mask, hipStream_t st);
// the tick alone, one thread (the trunk-only apply: no norm is wanted there)
int tick_steps(DevHP* hp, int tick_mask, hipStream_t st);
// One step of optimizer `opt` (CDRL_OPT_*, include/cdrl.h table) over the slice `a`, with the DevHP fields of `which` (WHICH_*); m / v
// are the optimizer's slots in the adam_m / adam_v arenas.  One kernel for every optimizer, Keras Adam included.
// tab: the slice's chunk table, whose chunk_part holds the gradient's partials -- every tensor is clipped by its norm (tf.clip_by_norm)
// when the threshold of `which` is positive; ChunkTable{}: plain 1024-element chunks of the slice, no clip.
// polyak < 1 (heads only): p = a * p_new + c * p_old in the same pass.  ticked: TICKED / NOT_TICKED.
// gate / gate_mode (GATE_MODE_*, below): the gated forms -- nothing is touched when the gate block says skip, and in global mode the
// list's scale from the block replaces the per-tensor clip.
struct GateBlock;
int clip_update(int opt, float polyak, const ArenaSlice& a, const ChunkTable& tab, DevHP* hp, int which, hipStream_t st,
                int ticked = NOT_TICKED, const GateBlock* gate = nullptr, int gate_mode = 0);
// counters to 0, Nadam m_caches to 1 (cdrl_learner_reset_optimizer_steps)
int reset_steps(DevHP* hp, hipStream_t st);
// counters to t[0..2] (policy, value, dynamics), Nadam m_caches to m_cache[0..2], passed to the kernel by value
// (cdrl_learner_set_optimizer_state); the float block in front of t_policy is not written
int set_steps(DevHP* hp, const int t[3], const float m_cache[3], hipStream_t st);
// two device-to-device copies in one launch; gate (or null): nothing is copied when the gate block says skip
int copy_two(float* d0, const float* s0, int64_t n0, float* d1, const float* s1, int64_t n1, hipStream_t st,
             const GateBlock* gate = nullptr);

// Gradient gate (cdrl_config.clip_mode = global and / or skip_nonfinite; include/cdrl.h): the norm of an optimizer's whole gradient
// list, known on the device before any element of the list is applied.  One block per learner (shared like DevHP), written by
// gate_decide in front of the updates of an apply step and read by the gated update / copy kernels behind it.
struct GateBlock {
    float clip_norm_dynamics;              // host-written (upload_hp), the only field the host writes; <= 0: trunk not clipped
    float scale_head, scale_trunk;         // of the apply in flight (1 outside global mode)
    int skip;                              // of the apply in flight
    int skipped[2], applied[2];            // apply steps per head (0 policy, 1 value) since create / gate_reset
    float last_norm[2][2], last_scale[2][2];      // [head][0: the head's list, 1: the trunk's] of that head's last apply
};
enum { GATE_GLOBAL = 1, GATE_GUARD = 2, GATE_TRUNK = 4 /* the apply consumes the trunk's gradient */, GATE_NADAM = 8,
       GATE_HEAD_PARTS = 16 /* the head's chunk partials are wanted whatever the gate needs (train stats) */ };
enum { GATE_MODE_OFF = 0, GATE_MODE_TENSOR = 1 /* skip only, per-tensor clip */, GATE_MODE_GLOBAL = 2 /* skip and list scale */ };
// Chunk partials (chunk_sqnorms_tick's, without the tick) of the head's table and, with GATE_TRUNK, of the trunk's, in one launch.  A
// list whose norm neither the mode nor the guard needs (threshold <= 0 on the device, no guard) is not read.
int gate_chunk_sqnorms(const float* g_head, const ChunkTable& tab_h, const float* g_trunk, const ChunkTable& tab_t, const DevHP* hp,
                       const GateBlock* gate, int head, int flags, hipStream_t st);
// One workgroup: folds the partials into the lists' squared norms (fixed order), writes scales, skip flag, last norms and the
// skipped / applied counter, and -- unless the step is skipped -- ticks the step counters (head; trunk with GATE_TRUNK) and advances
// the Nadam m_caches, as chunk_sqnorms_tick does on the ungated path.
// trust (or null): the apply is also skipped when the trust block says armed && stop, and counted there.
int gate_decide(const ChunkTable& tab_h, const ChunkTable& tab_t, DevHP* hp, GateBlock* gate, int head, int flags, hipStream_t st,
                TrustBlock* trust = nullptr);

// ---------------------------------------------------------------- update diagnostics (train_stats.hip)
// Chunk partials of a chunk table (sum of squares per 1024-element chunk, float64): one wave per chunk, no LDS.  Same partials
// contract as chunk_sqnorms_tick (which also ticks the optimizer counters and is the clip path's): deterministic, no atomics.
int stats_chunk_sqnorms(const float* g, const ChunkTable& tab, hipStream_t st);
// One ring row of an apply step (layout: include/cdrl.h, cdrl_train_stats_layout).  ring = [header int32 words | rows x width floats];
// the row index is header[0] % rows, read on the device.  stats_fold_norms writes sqrt(per-tensor sum of chunk partials) of the head
// (table a) at off_a and of the trunk (table b, may be empty) at off_b; stats_write_row, enqueued BEHIND it, writes everything else,
// zeroes the unused norm slots and advances header[0] (and header[1] when it overwrote an unread row).
enum StatsSlot : int {      // offsets inside a row's scalar block (KIND, T_HEAD, T_DYNAMICS hold int32 bit patterns)
    STATS_KIND = 0, STATS_T_HEAD = 1, STATS_T_DYNAMICS = 2, STATS_LR = 3, STATS_LR_DYNAMICS = 4, STATS_CLIP_RATIO = 5,
    STATS_ENTROPY_COEF = 6, STATS_SPEED = 7, STATS_SIMILARITY = 8, STATS_NSCALARS = 16
};
struct StatsRowArgs {
    float* ring;
    int header, rows, width;
    int kind;                   // 0 policy, 1 value
    const DevHP* hp;
    const float* metrics;       // 16 floats, copied verbatim
    const float* lin;           // [B][ld] linear head outputs
    int B, ld, col_speed, col_similarity;
    int off_scalars, off_metrics, off_norms, off_trunk;
    int n_head, n_trunk;
};
int stats_fold_norms(float* ring, int header, int rows, int width, const ChunkTable& tab_a, int off_a, const ChunkTable& tab_b,
                     int off_b, hipStream_t st);
int stats_write_row(const StatsRowArgs& a, hipStream_t st);
int stats_reset_ring(float* ring, hipStream_t st);

// ---------------------------------------------------------------- GAE (gae.hip)
// rewards [N+1] (bootstrap appended), values_be [N+1][2] -> returns_be [N][2], returns [N], adv_raw [N], adv [N]
int gae_returns(const float* rewards, const float* values_be, int N, double gamma, double lambda, float scale,
                float* returns, float* returns_be, float* adv_raw, float* adv, double* scratch, hipStream_t st);
// S trajectories (N rows in all) in one launch, one workgroup each: seg_off [S+1] (device) row offsets; rewards [N+S] / values_be [N+S][2]
// padded with every segment's bootstrap entry; packed outputs [N]; scratch 2*(N+S) doubles
int gae_returns_segments(const float* rewards, const float* values_be, const int32_t* seg_off, int S, int N, double gamma,
                         double lambda, float scale, float* returns, float* returns_be, float* adv_raw, float* adv, double* scratch,
                         hipStream_t st);

// ---------------------------------------------------------------- V-trace (vtrace.hip)
constexpr int VTRACE_CH = 2048;     // rows per LDS chunk of the two recurrences (3 x 8 bytes each)
// S replayed trajectories in one launch, the layout of gae_returns_segments plus the dense [N][A] alpha / beta / actions / log_prob_old;
// packed outputs [N] and the unclipped ratio rho [N]; scratch 4 * N doubles
int vtrace_segments(const float* rewards, const float* values_be, const float* alpha, const float* beta, const float* actions,
                    const float* log_prob_old, const int32_t* seg_off, int S, int N, int A, double gamma, double lambda, double rho_bar,
                    double c_bar, float scale, float* returns, float* returns_be, float* adv_raw, float* adv, float* rho, double* scratch,
                    hipStream_t st);

}  // namespace cdrl

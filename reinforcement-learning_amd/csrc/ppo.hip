// ppo.hip -- C ABI of include/rlgpu_ppo.h: actor/critic MLPs, action sampling, PPO minibatch
// loss + backward, clip_grad_norm_ + AdamW, on hand-written MFMA / wave kernels.
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/rlgpu_ppo.h"
#include "common.hpp"
#include "mlp_kernels.hpp"
#include "ppo_kernels.hpp"
#include "infer_kernels.hpp"

namespace {

using rlgpu::ceil_div;

// launch a kernel template instantiated on the 16-bit inference format (bf16 / fp16)
#define RLGPU_H16_LAUNCH(F16, KERN, ...)                                                     \
    do {                                                                                     \
        if (F16) hipLaunchKernelGGL(KERN<true>, __VA_ARGS__);                                \
        else hipLaunchKernelGGL(KERN<false>, __VA_ARGS__);                                   \
    } while (0)

// One side of a layer's pre-split weight: bf16 (x6, three) or fp16 (H3, two) planes of `rows` x `ld` elements,
// rows padded to whole B tiles of the mode and ld to mlp::XKMAX, zero filled.  Offsets into Model::wsplit /
// Model::wscale; -1 = none.
struct Side {
    int64_t planes = -1;
    int rows = 0, ld = 0;
    int64_t scale = -1;  // H3: per-row inverse scales of the planes
    int64_t frag = -1;   // H3, mlp::RLN_J rows feeding a full-row kernel: the planes in fragment order (mlp::frag_weight_h3)
    int64_t plane() const { return (int64_t)rows * ld; }  // elements per plane
};

struct Layer {
    int in, out;
    int64_t w, b, g, be;      // offsets into the flat fp32 buffers (g/be = -1 without LayerNorm)
    int in_pad;               // bf16 copy: weight rows padded to a multiple of 8 (16 bytes)
    int64_t hw, hb, hg, hbe;  // offsets into the padded bf16 inference copy
    int64_t fw = -1;          // offset into the fragment-major inference copy (infer::weight_to_frag)
    // the weight as B operand of the x6 / H3 training GEMMs (none for the rank-1 critic head, which has no GEMM):
    // forward B = W [out_pad][in_pad], backward dA B = W^T [in_pad][out_pad]
    Side fwd, bwd;
};

struct Model {
    std::vector<Layer> L;  // hidden layers then the output layer (last; none for the shared head)
    bool head_only = false;  // the shared head: every layer is [Linear -> LayerNorm -> activation]
    int in, out;
    int64_t off, count;
    float lr;
    int mode = 0;  // training GEMM arithmetic (rlgpu_ppo_config.train_gemm)
    int akind = mlp::ACT_LEAKY;  // activation kind of the hidden layers (mlp::act_fwd)
    // fp32 training workspace (per model, so the two models' passes can overlap on two streams)
    std::vector<float*> xhat, act, rstd;
    float *y = nullptr, *dy = nullptr, *dA = nullptr, *dZ = nullptr, *mid = nullptr;  // y: model output
    float* hpart = nullptr;  // rank-1 head dw / db partials, written by the last LayerNorm backward
    // per-layer partial buffers of the deferred reductions (so a backward pass reduces them all at its end):
    // split-K weight-gradient partials of layer l, LayerNorm-backward column partials of hidden layer l, and
    // the loss kernel's output-bias partials
    std::vector<float*> wpart_l, cpart_l;
    float* lpart = nullptr;
    int64_t midn = 0;  // floats per row of a reduction's level-1 sums (m.mid holds kRedJobs x 16 rows)
    uint16_t* wsplit = nullptr;  // split weight planes (x6 / H3 modes)
    int64_t nsplit = 0;
    float* wscale = nullptr;     // H3: per-row inverse scales of the weight planes
    int64_t nscale = 0;
    // H3: 64-shard max |x| slots of the GEMM operand tensors (kAmaxSlots x 64 floats):
    // act[l] at slot l, dZ of layer l at kAmaxDZ + l, the loss gradient dout at kAmaxOut
    float* amax = nullptr;
    float* dX = nullptr;  // gradient w.r.t. the model input (policy / critic behind a shared head)
};
// One Linear layer of a model's 16-bit inference forward (rlgpu_ppo::chain)
struct Link {
    const Layer* L;
    bool hidden;  // [Linear -> LayerNorm -> activation]; false: the output Linear
};
// hidden [Linear -> LayerNorm -> activation] layers of a model (all of the shared head's)
inline int nhid(const Model& m) { return (int)m.L.size() - (m.head_only ? 0 : 1); }
constexpr int kAmaxDZ = RLGPU_MAX_LAYERS, kAmaxOut = 2 * RLGPU_MAX_LAYERS, kAmaxSlots = 2 * RLGPU_MAX_LAYERS + 1;
inline bool split_mode(int mode) { return mode == RLGPU_GEMM_F32X6 || mode == RLGPU_GEMM_F16X3; }

constexpr int kMaxSplits = 256;
// concurrent gemm_f32 workgroups on the device (CUs x RLGPU_GEMM_OCC), set at create: the split-K
// weight gradients are sized to fill whole rounds of workgroups
int g_cus = 256;  // compute units of the device, set at create

// A three-way environment knob: 0 = never, 1 = always, unset (or anything else) = -1, the caller's default.
// Callers keep the value in a function-local static, so each knob is read once per process.
inline int tri_knob(const char* name) {
    const char* e = getenv(name);
    const int v = e ? atoi(e) : -1;
    return v == 0 || v == 1 ? v : -1;
}
inline bool knob_or(int knob, bool dflt) { return knob < 0 ? dflt : knob == 1; }

// Forward / input-gradient H3 GEMMs with output widths that are multiples of 256 on the 256 x 256 tile kernel
// mlp::gemm_h3q, and weight gradients on mlp::gemm_h3qt (same bits as gemm_x6): by default for 1024 or
// more output columns (the C5 leg's 2048-wide layers: 31.6 -> 27.6 ms per 50k minibatch against 128 x 256 tiles,
// profiles/r05ad_h3_quad_ab.txt); at 512 columns
// (K = 512, 16 stages per tile) its one workgroup per CU cannot hide the tile's prologue and epilogue and the
// C2 minibatch takes 1.59 -> 1.70 ms.  RLGPU_H3_QUAD=0: never, 1: for every width that is a multiple of 256.
inline bool h3_quad(int J) {
    static const int knob = tri_knob("RLGPU_H3_QUAD");
    return J % mlp::BQ == 0 && knob_or(knob, J >= 1024);
}
// Hidden layer L of forward_train on the full-row kernel mlp::gemm_h3_rowln (the H3 forward GEMM with its
// LayerNorm + LeakyReLU in the same launch; same bits as gemm_x6 + ln_act_fwd_f32).  Eligible output width:
// exactly 512 columns (mlp::RLN_J: the kernel's tile is the whole row, and its LayerNorm part is
// ln_act_fwd_f32<8>'s column layout); every other width keeps the two-kernel path, and so does every layer of a
// SIGMOID / TANH model (the full-row kernels are single LeakyReLU kernels: gemm_x6 + ln_act_fwd_f32<8, ACT>).  RLGPU_H3_ROWFUSE=0:
// never, 1: every eligible layer; unset: on (C2 minibatch 1.57 -> 1.49 ms, learn phase 126.9 -> 120.2 ms per
// iteration against the two-kernel path, profiles/r07a_rowfuse_bench_pairs.txt).
// The one predicate behind both the launch (forward_train) and the fragment-order planes it reads
// (split_weights); the launch also needs 16-byte loads of its A operand, else it falls back.
constexpr bool kRowFuseDefault = true;
inline bool rowfuse_fwd(const Model& m, const Layer& L) {
    static const int knob = tri_knob("RLGPU_H3_ROWFUSE");
    return m.mode == RLGPU_GEMM_F16X3 && m.akind == mlp::ACT_LEAKY && L.out == mlp::RLN_J && L.fwd.frag >= 0 &&
           knob_or(knob, kRowFuseDefault);
}
// The input-gradient GEMM of layer L on the full-row kernel mlp::gemm_h3_row_lnbwd (the H3 dA GEMM of a layer with
// the LayerNorm + LeakyReLU backward of the hidden layer below it in the same launch; dA is never stored; same
// bits as gemm_x6 + ln_act_bwd<8>).  Eligible: a layer of exactly 512 inputs (mlp::RLN_J) above a hidden layer
// (`below`; null for a model's first layer) of a LeakyReLU / ReLU model; everything else keeps the two-kernel path.
// RLGPU_H3_ROWFUSE_BWD=0: never, 1: every eligible layer; unset: on
// (C2 minibatch 1.49 -> 1.36 ms, learn phase 122.1 -> 110.8 ms per iteration against the two-kernel path,
// profiles/r08a_rowfuse_bwd_bench_pairs.txt).  Independent of RLGPU_H3_ROWFUSE.
// As above: the one predicate behind the launch (backward) and its planes (split_weights).
constexpr bool kRowFuseBwdDefault = true;
inline bool rowfuse_bwd(const Model& m, const Layer& L, const Layer* below) {
    static const int knob = tri_knob("RLGPU_H3_ROWFUSE_BWD");
    return m.mode == RLGPU_GEMM_F16X3 && m.akind == mlp::ACT_LEAKY && below && below->out == mlp::RLN_J && L.in == mlp::RLN_J && L.bwd.frag >= 0 &&
           knob_or(knob, kRowFuseBwdDefault);
}
inline int gemm_slots(int mode) {
    // H3: 146 / 156 VGPRs (forward / weight-gradient instances), 40 KB LDS -> three workgroups per CU
    // (-Rpass-analysis=kernel-resource-usage: occupancy 3 waves / SIMD); x6: two
    if (mode == RLGPU_GEMM_F16X3) return g_cus * 3;
    return g_cus * (split_mode(mode) ? 2 : RLGPU_GEMM_OCC);
}
// K granularity of a split-K chunk: a whole number of stages of either kernel
inline int kgran(int mode) { return split_mode(mode) ? mlp::XKMAX : mlp::BK; }

}  // namespace

struct rlgpu_ppo {
    rlgpu_ppo_config cfg;
    Model M[3];       // policy, critic, shared head (M[2], present when nm == 3)
    int nm = 2;
    bool shared() const { return nm == 3; }
    float* dshared = nullptr;  // the shared head's output gradient: policy dX + critic dX
    int64_t nparams = 0, nhalf = 0;
    float *params = nullptr, *grads = nullptr, *exp_avg = nullptr, *exp_avg_sq = nullptr;
    uint16_t* half = nullptr;
    uint16_t* half_ver = nullptr;  // bf16 policy copy of an old version (self-play), same layout as half
    uint16_t *frag = nullptr, *frag_ver = nullptr;  // the weights of half / half_ver in MFMA fragment order
    int64_t nfrag = 0;
    bool has_ver = false;
    // the guiding policy (rlgpu_ppo_set_guide): a third 16-bit copy + its fragment-order copy, and the f32 logits of one
    // chunk of the fused guide pass [max_rows][A]; all allocated by the first set_guide, none on an unguided handle
    uint16_t *half_guide = nullptr, *frag_guide = nullptr;
    float* guide_f = nullptr;
    bool has_guide = false;
    float* teach_f = nullptr;  // a teacher handle's f32 logits of one chunk [max_rows][A] (rlgpu_ppo_teacher_probs), on first use
    // the training GEMMs' split weight planes are stale (parameters changed since the last split):
    // set by init / refresh_half / the optimizer step, cleared when forward_train re-splits.  With
    // the whole iteration as one batch the planes are rebuilt once per optimizer step, not per
    // minibatch.
    bool split_dirty[3] = {true, true, true};
    int64_t step[3] = {0, 0, 0};  // AdamW step count per model (libtorch keeps it per parameter)
    int32_t opt[3] = {RLGPU_OPT_ADAMW, RLGPU_OPT_ADAMW, RLGPU_OPT_ADAMW};  // rlgpu_ppo_set_optimizer
    bool opt_stepped[3] = {false, false, false};  // the model's optimizer has stepped: its type is fixed
    int hmax = 0;
    float *scratch = nullptr;  // clip partials + coefficients
    hipStream_t aux = nullptr;  // second stream: the critic's minibatch pass overlaps the policy's
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    float* x0 = nullptr;       // gathered minibatch obs, rows padded to x_ld floats
    int x_ld = 0;
    float* x_amax = nullptr;   // H3: 64-shard max |x0| (with both models' slots: one memset per pass)
    float* amax_all = nullptr;
    int64_t amax_count = 0;
    uint16_t* xh = nullptr;    // bf16 obs for inference, rows padded to xh_ld
    int xh_ld = 0;
    uint16_t *zh = nullptr, *ah[2] = {nullptr, nullptr}, *logits_h = nullptr;
    float* logits_f = nullptr;  // fp32 inference (RLGPU_INFER_F32): the policy's logits [max_rows][A]
    // The Linear layers a 16-bit forward of model mi runs through: the shared head's first (for the policy / critic), then
    // the model's -- Model::Forward chained as InferPolicyProbsFromModels / InferCritic do (PPOLearner.cpp:90-91,188-191).
    // The shared head's f32 output re-enters the policy as bf16 (Models.cpp:64), which is exact, so the chain is one 16-bit
    // network.  Built once, at the end of rlgpu_ppo_create (build_chains): the Layer vectors do not move afterwards.
    std::vector<Link> chain[3];
    bool fused_fit[3] = {false, false, false};  // chain[mi]'s widths fit the fused inference kernel
    std::vector<void*> allocs;

    template <class T>
    T* alloc(size_t count) {
        allocs.push_back(nullptr);  // the slot first: a buffer never exists outside the list
        allocs.back() = rlgpu::dev_alloc(count * sizeof(T) + 16);
        return (T*)allocs.back();
    }
};

// inference precision (rlgpu_ppo_config.infer_fp16): the 16-bit copy's type, and whether the policy / critic
// inference runs the fp32 training forward instead (useHalfPrecision = false, Models.cpp:36-68)
inline bool f16(const rlgpu_ppo* h) { return h->cfg.infer_fp16 == RLGPU_INFER_F16; }
inline bool infer_f32(const rlgpu_ppo* h) { return h->cfg.infer_fp16 == RLGPU_INFER_F32; }

namespace {

// ---- learn-phase kernel timing (rlgpu_kernel_timing / rlgpu_kernel_timing_read): HIP events
// around the training GEMM and LayerNorm launches, recorded on the stream each launch goes to (the
// policy's and the critic's passes run on two streams).  Off unless enabled; bench.py reports the
// learn phase's roofline from it.  Work per launch: flops (GEMMs) or algorithmic bytes (row kernels).
namespace ktime {
enum { FWD_GEMM = 0, WGRAD_GEMM = 1, LN_FWD = 2, LN_BWD = 3, NSLOT = 4 };
struct Rec {
    hipEvent_t a, b;
    int slot;
    double work;
};
struct State {
    bool on = false;
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;  // events of cleared records, reused
};
State g;
hipEvent_t event() {
    hipEvent_t e;
    if (!g.pool.empty()) {
        e = g.pool.back();
        g.pool.pop_back();
    } else {
        RLGPU_CHECK_HIP(hipEventCreate(&e));
    }
    return e;
}
void clear() {
    for (auto& r : g.recs) {
        g.pool.push_back(r.a);
        g.pool.push_back(r.b);
    }
    g.recs.clear();
}
// brackets one launch on stream s
struct Span {
    int idx = -1;
    hipStream_t s;
    Span(int slot, double work, hipStream_t s_) : s(s_) {
        if (!g.on) return;
        Rec r{event(), event(), slot, work};
        RLGPU_CHECK_HIP(hipEventRecord(r.a, s));
        g.recs.push_back(r);
        idx = (int)g.recs.size() - 1;
    }
    ~Span() {
        if (idx >= 0) (void)hipEventRecord(g.recs[idx].b, s);
    }
};
}  // namespace ktime

// An fp32 GEMM operand in memory: rows of ld floats, its H3 scale shards (64-shard max |x|; null outside H3), and
// whether the rows are zero-padded up to a multiple of 4 past the bound (so 16-byte loads may straddle it).
// Every A operand of the training passes is one: the gathered obs, act[l], dZ, the loss gradient.
struct Operand {
    const float* X;
    int64_t ld;
    const float* amax;
    bool tail_ok;
};
// 16-byte loads of an operand: 16-byte aligned rows and a bound (K for k-contiguous rows, I / J otherwise) that
// is a multiple of 4 or zero-padded past it (split-K chunk ends are multiples of BK)
inline bool vec_ok(const Operand& x, int bound) {
    return x.ld % 4 == 0 && (uintptr_t)x.X % 16 == 0 && (bound % 4 == 0 || x.tail_ok);
}

// What every training GEMM launch shares: C[I, J] = A . B with A = a, B = fp32 (amax_b: its H3 shards) or pre-split
// planes (bscale: their H3 per-row inverse scales), and the grid of tm x tn output tiles, one K split.  The
// caller adds C / bias and its split-K or plane fields.  h3: the launch is on the fp16x3 arithmetic.
mlp::GemmArgs gemm_args(bool h3, const Operand& a, const void* B, int64_t ldb, const float* amax_b, const float* bscale, int I,
                        int J, int K, int tm, int tn) {
    if (h3 && !(a.amax && (amax_b || bscale))) throw rlgpu::Error(RLGPU_ERR_STATE, "H3 GEMM without operand scales");
    mlp::GemmArgs g{};
    g.A = a.X;
    g.lda = a.ld;
    g.amax_a = a.amax;
    g.B = static_cast<const float*>(B);
    g.ldb = ldb;
    g.amax_b = amax_b;
    g.bscale = bscale;
    g.I = I;
    g.J = J;
    g.K = K;
    g.gx = (int)ceil_div(J, tn);
    g.gy = (int)ceil_div(I, tm);
    g.gz = 1;
    return g;
}
// one workgroup per tile of g's grid
template <class... P>
void launch_gemm(void (*kernel)(mlp::GemmArgs, P...), int threads, hipStream_t s, const mlp::GemmArgs& g, const P&... more) {
    hipLaunchKernelGGL(kernel, dim3(g.gx * g.gy * g.gz), dim3(threads), 0, s, g, more...);
    RLGPU_CHECK_HIP(hipGetLastError());
}
// f(std::bool_constant<a>, std::bool_constant<b>): two run-time flags as template arguments of one launch expression
template <class F>
void with_flags(bool a, bool b, F&& f) {
    if (a && b) f(std::true_type{}, std::true_type{});
    else if (a) f(std::true_type{}, std::false_type{});
    else if (b) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}
// the same for the operand layouts of mlp::gemm_f32
template <class F>
void with_layouts(int la, int lb, F&& f) {
    using IK = std::integral_constant<int, mlp::A_IK>;
    using KI = std::integral_constant<int, mlp::A_KI>;
    using JK = std::integral_constant<int, mlp::B_JK>;
    using KJ = std::integral_constant<int, mlp::B_KJ>;
    if (la == mlp::A_IK && lb == mlp::B_JK) f(IK{}, JK{});
    else if (la == mlp::A_IK && lb == mlp::B_KJ) f(IK{}, KJ{});
    else if (la == mlp::A_KI && lb == mlp::B_KJ) f(KI{}, KJ{});
    else throw rlgpu::Error(RLGPU_ERR_UNSUPPORTED, "gemm layout");
}

// C[I,J] (+ bias) = A . B with the layouts of mlp::gemm_f32, both operands fp32 in memory, K in `splits` chunks
// (partial k of I x ldc floats at C + k I ldc)
void gemm_f32(int mode, int la, int lb, const Operand& a, const Operand& b, float* C, int64_t ldc, const float* bias, int I, int J,
              int K, int splits, hipStream_t s) {
    const bool h3 = mode == RLGPU_GEMM_F16X3;
    const bool av = vec_ok(a, la == mlp::A_IK ? K : I), bv = vec_ok(b, lb == mlp::B_JK ? K : J);
    // H3 weight gradients: 256 x 256 tiles, the same split-K chunks (same bits as gemm_x6)
    const bool quad = h3 && la == mlp::A_KI && lb == mlp::B_KJ && I % mlp::BQ == 0 && h3_quad(J);
    mlp::GemmArgs g = gemm_args(h3, a, b.X, b.ld, b.amax, nullptr, I, J, K, quad ? mlp::BQ : mlp::BM, quad ? mlp::BQ : mlp::BN);
    g.C = C;
    g.bias = bias;
    g.ldc = ldc;
    const int chunk = (int)ceil_div(K, splits);
    g.kchunk = (int)ceil_div(chunk, kgran(mode)) * kgran(mode);
    g.gz = (int)ceil_div(K, g.kchunk);
    g.c_split = (int64_t)I * ldc;
    if (quad) {
        with_flags(av, bv, [&](auto AV, auto BV) { launch_gemm(mlp::gemm_h3qt<AV(), BV()>, 512, s, g); });
        return;
    }
    with_layouts(la, lb, [&](auto LA, auto LB) {
        with_flags(av, bv, [&](auto AV, auto BV) {
            if (mode == RLGPU_GEMM_F32X6) launch_gemm(mlp::gemm_x6<LA(), LB(), AV(), BV(), false, false>, 256, s, g);
            else if (h3) launch_gemm(mlp::gemm_x6<LA(), LB(), AV(), BV(), false, true>, 256, s, g);
            else launch_gemm(mlp::gemm_f32<LA(), LB(), AV(), BV()>, 256, s, g);
        });
    });
}

// C[I,J] (+ bias) = A . B on the x6 GEMM with B given as pre-split planes (a Side's layout: [J_pad][ldbp] k contiguous,
// bplane elements apart).  H3 (bscale given): fp16 planes with per-row inverse scales bscale, A scaled by its shards
void gemm_x6_pre(const Operand& a, const uint16_t* Bp, int ldbp, int64_t bplane, const float* bscale, float* C, int64_t ldc,
                 const float* bias, int I, int J, int K, hipStream_t s) {
    ktime::Span span(ktime::FWD_GEMM, 2.0 * I * J * K, s);
    const bool h3 = bscale != nullptr;
    const bool av = vec_ok(a, K);
    const bool quad = h3 && av && h3_quad(J);  // 256 x 256 tiles (bit-identical to gemm_x6's H3 path)
    mlp::GemmArgs g = gemm_args(h3, a, Bp, ldbp, nullptr, bscale, I, J, K, quad ? mlp::BQ : mlp::BM, quad ? mlp::BQ : mlp::BN);
    g.C = C;
    g.bias = bias;
    g.ldc = ldc;
    g.kchunk = (int)ceil_div(K, mlp::XKMAX) * mlp::XKMAX;
    g.bplane = bplane;
    if (quad) return launch_gemm(mlp::gemm_h3q<true>, 512, s, g);
    with_flags(av, h3, [&](auto AV, auto H3) { launch_gemm(mlp::gemm_x6<mlp::A_IK, mlp::B_JK, AV(), true, true, H3()>, 256, s, g); });
}

// refresh the split weight planes of model m from the current parameters (once per minibatch /
// training forward: the weights change only at the optimizer step, but may be written directly)
void split_weights(const float* P, Model& m, hipStream_t s) {
    if (!split_mode(m.mode)) return;
    for (size_t l = 0; l < m.L.size(); l++) {
        const Layer& L = m.L[l];
        // the fragment-order copies exactly where the full-row kernels will read them (the backward planes are
        // [in rows][out as k]: the forward planes' shape, the same reordering)
        const bool frag[2] = {rowfuse_fwd(m, L), rowfuse_bwd(m, L, l > 0 ? &m.L[l - 1] : nullptr)};
        for (int trans = 0; trans < 2; trans++) {
            const Side& S = trans ? L.bwd : L.fwd;
            if (S.planes < 0) continue;
            uint16_t* planes = m.wsplit + S.planes;
            if (m.mode != RLGPU_GEMM_F16X3) {
                hipLaunchKernelGGL(mlp::split_weight, dim3(ceil_div(S.plane(), 256)), dim3(256), 0, s, P + L.w, L.out, L.in, trans,
                                   S.rows, S.ld, planes);
                continue;
            }
            hipLaunchKernelGGL(mlp::split_weight_h3, dim3(S.rows), dim3(256), 0, s, P + L.w, L.out, L.in, (int64_t)L.in, trans, S.ld,
                               planes, S.plane(), m.wscale + S.scale);
            if (frag[trans])
                hipLaunchKernelGGL(mlp::frag_weight_h3, dim3(S.ld / 16 * (mlp::RLN_J / 32) * 2 * 64 / 256), dim3(256), 0, s, planes,
                                   S.plane(), S.ld, m.wsplit + S.frag);
        }
    }
    RLGPU_CHECK_HIP(hipGetLastError());
}

// split-K count of a weight gradient [out, in] over `rows`: one full round of workgroups
// (tiles x splits ~ gemm_slots), each split at least 4 K steps
int splits_for(int mode, int rows, int out, int in) {
    // H3 weight gradients of 1024 or more columns: counted in 128 x 256 blocks (the chunking gemm_h3qt's
    // 256 x 256 tiles were tuned with, profiles/r05ad_h3_quad_ab.txt)
    const int bn = (mode == RLGPU_GEMM_F16X3 && in >= 1024) ? mlp::BNW : mlp::BN;
    const int tiles = (int)(ceil_div(out, mlp::BM) * ceil_div(in, bn));
    int s = gemm_slots(mode) / tiles;
    const int maxs = rows / (4 * mlp::BK);
    if (s > maxs) s = maxs;
    if (s > kMaxSplits) s = kMaxSplits;
    return s < 1 ? 1 : s;
}

// The reductions of one backward pass, launched together at its end: one mlp::reduce_batch launch per level
// for all of them instead of one or two launches each (the partial buffers are per layer, so nothing is
// overwritten before the flush).  Same summation orders, same bits as the separate launches.
struct Reducer {
    mlp::RedBatch b{};
    Model* m = nullptr;
    void add(const float* part, int nblk, int64_t stride, int n, float* dst, bool splits, hipStream_t s) {
        if (b.njobs == mlp::kRedJobs) flush(s);
        mlp::RedJob& J = b.j[b.njobs];
        J.part = part;
        J.dst = dst;
        J.stride = stride;
        J.nblk = nblk;
        J.n = n;
        J.mid = m->mid + (int64_t)b.njobs * 16 * m->midn;
        if (splits) {
            J.G = 1;
            J.vec = (n % 4 == 0 && stride % 4 == 0 && ((uintptr_t)part & 15) == 0 && ((uintptr_t)dst & 15) == 0) ? 1 : 2;
        } else {
            J.G = nblk >= 256 ? 16 : 1;
            J.vec = 0;
            if ((int64_t)n > m->midn) throw rlgpu::Error(RLGPU_ERR_STATE, "reduction wider than its level-1 buffer");
        }
        b.njobs++;
    }
    void flush(hipStream_t s) {
        if (!b.njobs) return;
        bool two = false;
        int t = 0;
        for (int k = 0; k < b.njobs; k++) {
            const mlp::RedJob& J = b.j[k];
            b.tile0[k] = t;
            t += J.vec == 1 ? (int)ceil_div(J.n, 4096) : J.vec == 2 ? (int)ceil_div(J.n, 1024) : (int)ceil_div(J.n, 64) * J.G;
            two |= J.vec == 0 && J.G > 1;
        }
        b.tile0[b.njobs] = t;
        b.level = 1;
        hipLaunchKernelGGL(mlp::reduce_batch, dim3(t), dim3(1024), 0, s, b);
        RLGPU_CHECK_HIP(hipGetLastError());
        if (two) {
            t = 0;
            for (int k = 0; k < b.njobs; k++) {
                const mlp::RedJob& J = b.j[k];
                b.tile0[k] = t;
                t += (J.vec == 0 && J.G > 1) ? (int)ceil_div(J.n, 64) : 0;
            }
            b.tile0[b.njobs] = t;
            b.level = 2;
            hipLaunchKernelGGL(mlp::reduce_batch, dim3(t), dim3(1024), 0, s, b);
            RLGPU_CHECK_HIP(hipGetLastError());
        }
        b.njobs = 0;
    }
};

// dW += dZ^T . X over n rows: split-K over the rows into the layer's partial buffer `wpart`, reduced in a fixed
// order into gW through R at the end of the pass.  dz: [n][out] (rows zero-padded when tail_ok), x: [n][in]
void weight_grad(Model& m, const Operand& dz, int out, const Operand& x, int in, int n, float* gW, hipStream_t s, Reducer& R,
                 float* wpart) {
    const int splits = splits_for(m.mode, n, out, in);
    const int chunk = (int)ceil_div(ceil_div(n, splits), kgran(m.mode)) * kgran(m.mode);
    {
        ktime::Span span(ktime::WGRAD_GEMM, 2.0 * out * in * (double)n, s);
        gemm_f32(m.mode, mlp::A_KI, mlp::B_KJ, dz, x, wpart, in, nullptr, out, in, n, splits, s);
    }
    const int64_t e = (int64_t)out * in;
    R.add(wpart, (int)ceil_div(n, chunk), e, (int)e, gW, true, s);
}

// row stride of a multi-column loss gradient dout [n, out]: a multiple of 4 floats (the policy loss
// writes the padding columns as zeros)
inline int dout_ld(int out) { return out > 1 ? (out + 3) / 4 * 4 : out; }

// H3 operand scale slots (null in the other modes): slot k of model m, and the gathered obs
inline float* amax_slot(Model& m, int k) { return m.mode == RLGPU_GEMM_F16X3 ? m.amax + (int64_t)k * 64 : nullptr; }
inline const float* wscale_at(const Model& m, int64_t off) {
    return m.mode == RLGPU_GEMM_F16X3 ? m.wscale + off : nullptr;
}

// the gathered minibatch obs (rows of x_ld floats, zero-padded)
inline Operand obs_input(rlgpu_ppo* h) { return {h->x0, h->x_ld, h->x_amax, true}; }
// what model mi reads: the obs, or the shared head's last activation (PPOLearner.cpp:403,474)
inline Operand model_input(rlgpu_ppo* h, int mi) {
    if (mi == 2 || !h->shared()) return obs_input(h);
    Model& sm = h->M[2];
    const int l = nhid(sm) - 1;
    return {sm.act[l], sm.L[l].out, amax_slot(sm, l), false};
}

// C[n, J] = A . W (+ bias) for layer L of model m: forward (J = L.out, K = L.in, with the bias) or -- bwd -- its
// input gradient (J = L.in, K = L.out, A . W as [K][J]).  On the layer's pre-split planes when it has them
// (gemm_x6_pre: the timed span, quad or 128 x 128 tiles), else on the fp32 weight (gemm_f32).
void linear(const float* P, const Model& m, const Layer& L, bool bwd, const Operand& a, int n, float* C, hipStream_t s) {
    const Side& S = bwd ? L.bwd : L.fwd;
    const int J = bwd ? L.in : L.out, K = bwd ? L.out : L.in;
    const float* bias = bwd ? nullptr : P + L.b;
    if (S.planes >= 0)
        gemm_x6_pre(a, m.wsplit + S.planes, S.ld, S.plane(), wscale_at(m, S.scale), C, J, bias, n, J, K, s);
    else
        gemm_f32(m.mode, mlp::A_IK, bwd ? mlp::B_KJ : mlp::B_JK, a, Operand{P + L.w, L.in, nullptr, false}, C, J, bias, n, J, K, 1, s);
}

// The GemmArgs of a full-row kernel (mlp::gemm_h3_rowln / gemm_h3_row_lnbwd) on side S: its fragment-order planes,
// one 64-row x 512-column tile per workgroup; the caller adds C / bias where the kernel has them
mlp::GemmArgs row_args(const Model& m, const Side& S, const Operand& a, int n, int K) {
    return gemm_args(true, a, m.wsplit + S.frag, S.ld, nullptr, wscale_at(m, S.scale), n, mlp::RLN_J, K, mlp::RLN_BM, mlp::RLN_J);
}

// fp32 training forward of model mi on x; keeps activations; writes the output layer to `out` (the
// shared head has none: its last activation stays in m.act).
void forward_train(rlgpu_ppo* h, int mi, const Operand& x, int n, float* out, hipStream_t s) {
    Model& m = h->M[mi];
    const float* P = h->params;
    if (h->split_dirty[mi]) {
        split_weights(P, m, s);
        h->split_dirty[mi] = false;
    }
    const int nh = nhid(m);  // >= 1 (rlgpu_ppo_create)
    const Layer* O = m.head_only ? nullptr : &m.L[nh];
    const bool head1 = O && O->out == 1;  // rank-1 head fused into the last LayerNorm forward
    Operand in = x;
    for (int l = 0; l < nh; l++) {
        const Layer& L = m.L[l];
        const bool fuse = head1 && l == nh - 1;
        // LayerNorm + activation of z = m.xhat[l] into m.act[l] (and the rank-1 head's output)
        const mlp::RowLnArgs ln{L.g >= 0 ? P + L.g : nullptr, L.be >= 0 ? P + L.be : nullptr, h->cfg.leaky_slope, h->cfg.layer_norm,
                                m.act[l], reinterpret_cast<float2*>(m.rstd[l]), amax_slot(m, l), fuse ? P + O->w : nullptr,
                                fuse ? P + O->b : nullptr, fuse ? out : nullptr};
        if (rowfuse_fwd(m, L) && vec_ok(in, L.in)) {  // one launch; without 16-byte loads of `in`, the two below
            ktime::Span span(ktime::FWD_GEMM, 2.0 * n * L.out * L.in, s);
            mlp::GemmArgs g = row_args(m, L.fwd, in, n, L.in);
            g.C = m.xhat[l];
            g.bias = P + L.b;
            g.ldc = L.out;
            launch_gemm(mlp::gemm_h3_rowln, 256, s, g, ln);
        } else {
            linear(P, m, L, false, in, n, m.xhat[l], s);
            // bytes: z read, act written, (mean, rstd) written
            ktime::Span span(ktime::LN_FWD, (double)n * (8.0 * L.out + 8.0), s);
            int lnf_rows = 0;
            const auto lnf = mlp::ln_act_fwd_f32_pick(m.akind, L.out, &lnf_rows, fuse);
            hipLaunchKernelGGL(lnf, dim3(ceil_div(n, lnf_rows)), dim3(256), 0, s, m.xhat[l], ln.gamma, ln.beta, n, L.out, ln.slope,
                               ln.use_ln, ln.act, ln.stats, ln.amax, ln.head_w, ln.head_b, ln.head_out);
            RLGPU_CHECK_HIP(hipGetLastError());
        }
        in = Operand{m.act[l], L.out, amax_slot(m, l), false};
    }
    if (O && !head1) linear(P, m, *O, false, in, n, out, s);
}

// The input gradient of layer l >= 1 (dA = A . W_l, A = the layer's dZ or the loss gradient) and the LayerNorm
// backward of hidden layer l - 1 in one launch of mlp::gemm_h3_row_lnbwd: writes that layer's dZ to dz_out (not A),
// its column partials to m.cpart_l[l - 1] and max |dZ| to its slot; dA is not stored.  False (nothing launched)
// when the pair is not eligible (rowfuse_bwd) or A cannot take 16-byte loads: the caller runs the two kernels.
bool dA_ln_bwd_fused(rlgpu_ppo* h, Model& m, int l, const Operand& a, int n, float* dz_out, hipStream_t s) {
    if (l < 1) return false;
    const Layer& L = m.L[l];
    const Layer& C = m.L[l - 1];  // the consumer: a hidden layer on ln_act_bwd<8>, never the rank-1 head's variant
    if (!rowfuse_bwd(m, L, &C) || !vec_ok(a, L.out)) return false;
    const float* P = h->params;
    ktime::Span span(ktime::FWD_GEMM, 2.0 * n * L.in * L.out, s);
    const mlp::GemmArgs g = row_args(m, L.bwd, a, n, L.out);
    const mlp::RowLnBwdArgs ln{C.g >= 0 ? P + C.g : nullptr, C.be >= 0 ? P + C.be : nullptr, h->cfg.leaky_slope, h->cfg.layer_norm,
                               m.xhat[l - 1], reinterpret_cast<const float2*>(m.rstd[l - 1]), dz_out, m.cpart_l[l - 1],
                               amax_slot(m, kAmaxDZ + l - 1)};
    launch_gemm(mlp::gemm_h3_row_lnbwd, 256, s, g, ln);
    return true;
}

// backward of model mi (input x) from dout into the grad buffer (accumulating).  dout: the loss
// gradient [n, out] of the output layer, or -- the shared head -- the gradient of its last
// activation [n, H].  dout_part: per-block column partials of a multi-column dout (dout_nblk rows of `out`
// floats, written by the loss kernel) for the output bias.
// H3: dout's max |x| is in slot kAmaxOut.  When m.dX is set (a model behind the shared head) the
// gradient w.r.t. the model input is written there too.
void backward(rlgpu_ppo* h, int mi, const Operand& x, int n, const float* dout, hipStream_t s,
              const float* dout_part = nullptr, int dout_nblk = 0) {
    Model& m = h->M[mi];
    const float* P = h->params;
    float* G = h->grads;
    const int nh = nhid(m);  // >= 1 (rlgpu_ppo_create): the output layer never reads the model input
    // layer l's input, as its weight gradient reads it
    const auto input_of = [&](int l) { return l > 0 ? Operand{m.act[l - 1], m.L[l].in, amax_slot(m, l - 1), false} : x; };
    const float* dA_top = m.dA;  // gradient of the last hidden layer's activation
    bool rank1 = false;          // rank-1 output layer folded into the last LayerNorm backward
    // the next layer's dZ when the launch above it already ran its LayerNorm backward (dA_ln_bwd_fused); those
    // launches alternate between m.dZ and m.dA, which no dA occupies on a fused layer, so none runs in place
    float* fused_dz = nullptr;
    // the pass's bias / LayerNorm / weight-gradient reductions, launched together at its end
    Reducer R;
    R.m = &m;
    const Layer* O = m.head_only ? nullptr : &m.L[nh];
    if (!O) {
        dA_top = dout;
    } else if (O->out == 1) {
        // rank-1 head after a LayerNorm: its backward recomputes dA = dv w^T and the activation, and
        // emits the head's dw / db partials (m.hpart) beside its own -- no separate head pass
        rank1 = true;
    } else {
        // the loss kernel provides the bias partials (and, H3, dout's scale): there is no column-sum pass
        if (!dout_part) throw rlgpu::Error(RLGPU_ERR_STATE, "backward: a multi-column dout needs the loss kernel's bias partials");
        // dout rows of dld floats (the policy loss pads them with zeros to a multiple of 4)
        const int dld = dout_ld(O->out);
        const Operand d{dout, dld, amax_slot(m, kAmaxOut), dld > O->out};
        weight_grad(m, d, O->out, input_of(nh), O->in, n, G + O->w, s, R, m.wpart_l[nh]);
        R.add(dout_part, dout_nblk, O->out, O->out, G + O->b, false, s);
        // dA = dout . W_out
        if (dA_ln_bwd_fused(h, m, nh, d, n, m.dZ, s)) fused_dz = m.dZ;
        else linear(P, m, *O, true, d, n, m.dA, s);
    }
    const float* dA_in = dA_top;  // the gradient of the current layer's activation, unless fused_dz
    for (int l = nh - 1; l >= 0; l--) {
        const Layer& L = m.L[l];
        const float* gg = L.g >= 0 ? P + L.g : nullptr;
        const float* bb = L.be >= 0 ? P + L.be : nullptr;
        const bool r1 = rank1 && l == nh - 1;  // dA of the rank-1 head, recomputed in the kernel
        int lnb_rows = 0;
        const auto lnb = mlp::ln_act_bwd_pick(m.akind, L.out, r1, &lnb_rows);
        // this layer's dZ: never the buffer its dA is in
        float* dz = fused_dz ? fused_dz : (dA_in == m.dZ ? m.dA : m.dZ);
        const int nb = (int)ceil_div(n, lnb_rows);
        if (!fused_dz) {
            // bytes: dA (recomputed for the rank-1 head: its dv instead), z, stats read; dZ written
            ktime::Span span(ktime::LN_BWD, (double)n * ((r1 ? 4.0 : 4.0 * L.out) + 8.0 * L.out + 8.0), s);
            hipLaunchKernelGGL(lnb, dim3(nb), dim3(256), 0, s, r1 ? nullptr : dA_in, m.xhat[l],
                               reinterpret_cast<const float2*>(m.rstd[l]), gg, bb, n, L.out, h->cfg.leaky_slope,
                               h->cfg.layer_norm, dz, m.cpart_l[l], amax_slot(m, kAmaxDZ + l), r1 ? dout : nullptr,
                               r1 ? P + O->w : nullptr, r1 ? m.hpart : nullptr);
            RLGPU_CHECK_HIP(hipGetLastError());
        }
        // partials [blk][dbias | dgamma | dbeta] -> flat grads [b][g][be] (contiguous after L.b); the rank-1
        // head's [w | b] are contiguous too
        int ncol = h->cfg.layer_norm ? 3 * L.out : L.out;
        if (r1) R.add(m.hpart, nb, O->in + 1, O->in + 1, G + O->w, false, s);
        R.add(m.cpart_l[l], nb, 3 * (int64_t)L.out, ncol, G + L.b, false, s);
        const Operand d{dz, L.out, amax_slot(m, kAmaxDZ + l), false};
        weight_grad(m, d, L.out, input_of(l), L.in, n, G + L.w, s, R, m.wpart_l[l]);
        float* other = dz == m.dZ ? m.dA : m.dZ;  // free: takes this layer's dA, or the next layer's dZ
        float* dA = l > 0 ? other : m.dX;         // the first layer's only when the input gradient is wanted
        fused_dz = nullptr;
        if (!dA) continue;
        if (dA_ln_bwd_fused(h, m, l, d, n, other, s)) {
            fused_dz = other;
            continue;
        }
        dA_in = dA;
        linear(P, m, L, true, d, n, dA, s);
    }
    R.flush(s);
}

void gather_obs(rlgpu_ppo* h, const float* obs, const int32_t* idx, int64_t start, int n, hipStream_t s) {
    int64_t e = (int64_t)n * h->x_ld;
    // H3: clear every operand-scale slot of this pass, then the gather fills the obs slot
    if (h->amax_all) RLGPU_CHECK_HIP(hipMemsetAsync(h->amax_all, 0, h->amax_count * sizeof(float), s));
    hipLaunchKernelGGL(mlp::gather_rows, dim3(std::min<int64_t>(ceil_div(e, 256), mlp::GATHER_BLOCKS)), dim3(256), 0, s, obs,
                       h->cfg.obs_size, idx, start, n, h->x0, h->x_ld, h->x_amax);
    RLGPU_CHECK_HIP(hipGetLastError());
}

// bf16 inference forward of n <= max_rows rows through h->chain[mi]; returns the 16-bit result [n, out]
// (h->logits_h after an output Linear, else the last activation buffer).  Model::Forward with halfPrec
// (Models.cpp:42-68): every module runs on the bf16 copy, activations rounded to bf16.
const uint16_t* forward_half(rlgpu_ppo* h, int mi, const float* X, int n, hipStream_t s, const uint16_t* weights = nullptr) {
    const uint16_t* P = weights ? weights : h->half;
    const int64_t e = (int64_t)n * h->xh_ld;
    RLGPU_H16_LAUNCH(f16(h), mlp::rows_to_bf16, dim3(ceil_div(e, 256)), dim3(256), 0, s, X, h->cfg.obs_size, n, h->xh, h->xh_ld);
    RLGPU_CHECK_HIP(hipGetLastError());
    const uint16_t* in = h->xh;
    int64_t ld = h->xh_ld;
    int cur = 0;
    for (const Link& k : h->chain[mi]) {
        const Layer& L = *k.L;
        mlp::HGemmArgs g;
        g.A = in;
        g.B = P + L.hw;
        g.bias = P + L.hb;
        g.C = k.hidden ? h->zh : h->logits_h;
        g.lda = ld;
        g.ldb = L.in_pad;
        g.ldc = L.out;
        g.I = n;
        g.J = L.out;
        g.K = L.in_pad;
        g.gx = (int)ceil_div(L.out, mlp::BN);
        g.gy = (int)ceil_div(n, mlp::BM);
        RLGPU_H16_LAUNCH(f16(h), mlp::gemm_bf16, dim3(g.gx * g.gy), dim3(256), 0, s, g);
        RLGPU_CHECK_HIP(hipGetLastError());
        if (!k.hidden) return h->logits_h;
        const uint16_t* gg = L.hg >= 0 ? P + L.hg : nullptr;
        const uint16_t* bb = L.hbe >= 0 ? P + L.hbe : nullptr;
        hipLaunchKernelGGL(f16(h) ? mlp::ln_act_fwd_bf16_any<true>(L.out, h->cfg.activation) : mlp::ln_act_fwd_bf16_any<false>(L.out, h->cfg.activation),
                           dim3(ceil_div(n, mlp::LNF_ROWS)), dim3(256), 0, s, h->zh, gg, bb, n, L.out,
                           h->cfg.leaky_slope, h->cfg.layer_norm, h->ah[cur]);
        RLGPU_CHECK_HIP(hipGetLastError());
        in = h->ah[cur];
        ld = L.out;
        cur ^= 1;
    }
    return in;
}

// fp32 forward of model 0 or 1 (through the shared head, if any) on n <= max_rows rows of X into out:
// the training forward's arithmetic (rlgpu_ppo_forward precision 0, and the fp32 inference)
void forward_f32(rlgpu_ppo* h, int model, const float* X, int n, float* out, hipStream_t s) {
    gather_obs(h, X, nullptr, 0, n, s);
    if (h->shared()) forward_train(h, 2, obs_input(h), n, nullptr, s);
    forward_train(h, model, model_input(h, model), n, out, s);
}

// ---- inference, one path behind every entry point.  A forward runs as the fp32 training forward (RLGPU_INFER_F32), as
// one launch of the fused kernel infer::mlp_infer when every layer fits its LDS tile (inputs / hidden widths <= 512,
// outputs <= 128), or on the layer-by-layer kernels (forward_half), which compute the fused kernel's bits.
unsigned long long* g_infer_trace = nullptr;  // rlgpu_debug_infer_trace
int64_t g_infer_trace_cap = 0;             // its capacity (uint64 entries)

// end of rlgpu_ppo_create: the chains, and whether their widths fit the fused kernel, which ends on an output Linear
void build_chains(rlgpu_ppo* h) {
    for (int mi = 0; mi < 3; mi++) {
        auto& c = h->chain[mi];
        if (mi != 2 && h->shared())
            for (auto& L : h->M[2].L) c.push_back({&L, true});
        const Model& m = h->M[mi];
        for (size_t l = 0; l < m.L.size(); l++) c.push_back({&m.L[l], m.head_only || l + 1 < m.L.size()});
        bool fit = !c.empty() && (int)c.size() <= infer::kMaxLinear && !c.back().hidden;
        for (size_t l = 0; fit && l < c.size(); l++)
            fit = c[l].L->in <= infer::IMAX && c[l].L->out <= (l + 1 < c.size() ? infer::IMAX : infer::IOUT);
        h->fused_fit[mi] = fit;
    }
}
// Model mi runs on the fused kernel.  RLGPU_FUSED_INFER=0 selects the layer-by-layer path; it is read on every
// call, not once per handle: tests/test_ppo.py::test_fused_inference_matches_layer_path flips it on a live handle.
bool fused_ok(const rlgpu_ppo* h, int mi) {
    if (infer_f32(h) || !h->fused_fit[mi]) return false;  // fp32 inference runs the training forward (forward_f32)
    const char* e = getenv("RLGPU_FUSED_INFER");
    return !(e && atoi(e) == 0);
}

// A block of rows of one inference call: X [n, obs_size], masks [n, num_actions] (null for a forward that draws
// nothing), and row0, the block's first row in the sampler's row numbering (cfg.sample_row_offset included).
struct Rows {
    const float* X;
    int64_t n, row0;
    const uint8_t* masks;
    // rows [b, b + m) of the block: the one place that knows the row strides
    Rows sub(const rlgpu_ppo_config& c, int64_t b, int64_t m) const {
        return {X + b * c.obs_size, m, row0 + b, masks ? masks + b * c.num_actions : nullptr};
    }
};
// What a sampling pass does with a block's logits: argmax (det) or the draw of (seed, row, step) into act, its log
// prob into logp (may be null), for the rows with (row_sel[i] != 0) == (sel != 0) (row_sel null: every row).
struct Draw {
    int det;
    uint64_t step;
    int32_t* act;
    float* logp;
    const uint8_t* row_sel = nullptr;
    int sel = 0;
    Draw sub(int64_t b) const { return {det, step, act + b, logp ? logp + b : nullptr, row_sel ? row_sel + b : nullptr, sel}; }
};

// which 16-bit copy of the weights an inference pass reads: the current parameters', the old version's
// (rlgpu_ppo_set_version) or the guiding policy's (rlgpu_ppo_set_guide)
enum class Weights { Current, Version, Guide };
inline const uint16_t* half_of(const rlgpu_ppo* h, Weights w) {
    return w == Weights::Guide ? h->half_guide : (w == Weights::Version ? h->half_ver : h->half);
}
inline const uint16_t* frag_of(const rlgpu_ppo* h, Weights w) {
    return w == Weights::Guide ? h->frag_guide : (w == Weights::Version ? h->frag_ver : h->frag);
}
inline Weights version_if(bool ver) { return ver ? Weights::Version : Weights::Current; }

// One fused forward of model mi over a block with the 16-bit copy `w` names: writes f32 outputs to out_f (d null, the kernel's mode 0) or samples actions (d, mode 1).  fused_args:
// its launch arguments (the one-wave form takes the same); infer_fused: the launch.
infer::InferArgs fused_args(const rlgpu_ppo* h, int mi, Weights w, const Rows& r, float* out_f, const Draw* d) {
    const auto& c = h->chain[mi];
    const int n = (int)r.n;
    infer::InferArgs a{};
    a.X = r.X;
    a.n = n;
    a.in = h->cfg.obs_size;
    a.P = half_of(h, w);
    a.F = frag_of(h, w);
    a.nl = (int)c.size();
    a.width[0] = a.in;
    for (int l = 0; l < a.nl; l++) {
        const Layer& L = *c[l].L;
        a.width[l + 1] = L.out;
        a.fw[l] = L.fw;
        a.hb[l] = L.hb;
        a.hg[l] = L.hg;
        a.hbe[l] = L.hbe;
    }
    a.slope = h->cfg.leaky_slope;
    a.use_ln = h->cfg.layer_norm;
    a.seed = h->cfg.seed;
    a.temp = h->cfg.policy_temperature;
    a.out_f = out_f;
    if (d) {
        a.mode = 1;
        a.masks = r.masks;
        a.row0 = r.row0;
        a.det = d->det;
        a.step = d->step;
        a.act = d->act;
        a.logp = d->logp;
        a.row_sel = d->row_sel;
        a.sel = d->sel;
    }
    return a;
}

// Model mi runs on the one-wave form of the fused kernel too (infer::wave_infer: 16 rows per wavefront): built for
// LeakyReLU / ReLU only.
bool wave_ok(const rlgpu_ppo* h, int mi) { return fused_ok(h, mi) && h->cfg.activation == mlp::ACT_LEAKY; }

// wave: on infer::mlp_infer_wave (the caller has checked wave_ok)
void infer_fused(rlgpu_ppo* h, int mi, Weights w, const Rows& r, float* out_f, const Draw* d, hipStream_t s, bool wave = false) {
    const int n = (int)r.n;
    infer::InferArgs a = fused_args(h, mi, w, r, out_f, d);
    if (wave) {
        rlgpu::launch_mlp_infer_wave(f16(h), ceil_div(n, infer::WR), s, &a, sizeof(a));
        RLGPU_CHECK_HIP(hipGetLastError());
        return;
    }
    a.trace = g_infer_trace;
    if (a.trace && ceil_div(n, infer::IR) * 16 > g_infer_trace_cap)
        throw rlgpu::Error(RLGPU_ERR_INVALID_ARG, "rlgpu_debug_infer_trace: buffer of " + std::to_string(g_infer_trace_cap) +
                                                      " entries, this launch needs " + std::to_string(ceil_div(n, infer::IR) * 16));
    // the LeakyReLU / ReLU instances are this unit's; SIGMOID / TANH: infer_act.hip
    if (h->cfg.activation != mlp::ACT_LEAKY)
        rlgpu::launch_mlp_infer_act(h->cfg.activation, f16(h), ceil_div(n, infer::IR), s, &a, sizeof(a));
    else
        RLGPU_H16_LAUNCH(f16(h), infer::mlp_infer, dim3(ceil_div(n, infer::IR)), dim3(infer::IT), 0, s, a);
    RLGPU_CHECK_HIP(hipGetLastError());
}

// The inference forward of model mi over a block (n <= max_rows off the fused kernel) into f32 out [n, out]: fp32
// (useHalfPrecision = false) or 16-bit.  half: 16-bit on an fp32 handle too (rlgpu_ppo_forward's precision 1).
void infer_values(rlgpu_ppo* h, int mi, const Rows& r, float* out, hipStream_t s, bool half = false) {
    if (infer_f32(h) && !half) return forward_f32(h, mi, r.X, (int)r.n, out, s);
    if (fused_ok(h, mi)) return infer_fused(h, mi, Weights::Current, r, out, nullptr, s);
    const uint16_t* y = forward_half(h, mi, r.X, (int)r.n, s);
    const int64_t e = r.n * h->M[mi].out;
    RLGPU_H16_LAUNCH(f16(h), ppo::bf16_to_f32, dim3(ceil_div(e, 256)), dim3(256), 0, s, y, out, e);
    RLGPU_CHECK_HIP(hipGetLastError());
}

// one policy forward over a block (n <= max_rows off the fused kernel) and its draw, with the current parameters
// or (ver) the old version's: the fused kernel, or fp32 logits / forward_half and the sampler
void sample_pass(rlgpu_ppo* h, bool ver, const Rows& r, const Draw& d, hipStream_t s) {
    if (fused_ok(h, 0)) return infer_fused(h, 0, version_if(ver), r, nullptr, &d, s);
    const int n = (int)r.n;
    const auto sample = [&](auto kern, const auto* logits) {
        hipLaunchKernelGGL(kern, dim3(ceil_div(n, 4)), dim3(256), 0, s, logits, r.masks, n, h->cfg.num_actions,
                           h->cfg.policy_temperature, d.det, h->cfg.seed, d.step, r.row0, d.act, d.logp, d.row_sel, d.sel);
        RLGPU_CHECK_HIP(hipGetLastError());
    };
    if (infer_f32(h)) {  // useHalfPrecision = false: fp32 logits, the same sampler
        forward_f32(h, 0, r.X, n, h->logits_f, s);
        return sample(ppo::sample_actions<false, float>, h->logits_f);
    }
    const uint16_t* y = forward_half(h, 0, r.X, n, s, ver ? h->half_ver : h->half);
    sample(f16(h) ? ppo::sample_actions<true> : ppo::sample_actions<false>, y);
}

// The action entry points after their argument checks: the block in chunks of `chunk` rows; with old_rows, per chunk
// the current policy's rows and then the old version's, log probs only from the current pass.  Chunking: the layered
// and fp32 paths work in the per-handle row buffers, so a launch of theirs takes at most max_rows rows; the fused
// kernel keeps none and takes any count.  rlgpu_ppo_infer_actions and _mixed chunk by max_rows on every path (the fused
// one too), rlgpu_ppo_infer_actions_rows -- fused only -- never chunks (INT64_MAX), and the critic chunks by max_rows
// off the fused kernel and by 2^30 rows on it.
void infer_policy(rlgpu_ppo* h, const Rows& rows, const Draw& draw, const uint8_t* old_rows, int64_t chunk, hipStream_t s) {
    for (int64_t b = 0; b < rows.n; b += chunk) {
        const Rows r = rows.sub(h->cfg, b, std::min(chunk, rows.n - b));
        Draw d = draw.sub(b);
        d.row_sel = old_rows ? old_rows + b : nullptr;
        for (d.sel = 0; d.sel < (old_rows ? 2 : 1); d.sel++) {
            if (d.sel) d.logp = nullptr;
            sample_pass(h, d.sel != 0, r, d, s);
        }
    }
}

// One side of a split weight -- `rows` B rows of k elements -- appended to m's plane and scale buffers: rows padded
// to whole B tiles of the mode, k to mlp::XKMAX; frag (H3): the fragment-order copy of its mlp::RLN_J rows behind it
Side add_side(Model& m, int rows, int k, bool frag) {
    const bool h3 = m.mode == RLGPU_GEMM_F16X3;
    const int rpad = h3 ? mlp::BNW : mlp::BN;
    Side S;
    S.rows = (int)ceil_div(rows, rpad) * rpad;
    S.ld = (int)ceil_div(k, mlp::XKMAX) * mlp::XKMAX;
    S.planes = m.nsplit;
    m.nsplit += (h3 ? 2 : 3) * S.plane();  // planes per split weight
    S.scale = m.nscale;
    m.nscale += S.rows;
    if (frag) {
        S.frag = m.nsplit;
        m.nsplit += 2 * (int64_t)mlp::RLN_J * S.ld;
    }
    return S;
}

// Model layout in the flat buffers.  out = 0: the shared head (hidden layers only, PPOLearner.cpp:56-64);
// input_grad: the model reads the shared head's output, so its first layer also gets the transposed
// weight planes for the input gradient.
void build_model(rlgpu_ppo* h, Model& m, int in, const int32_t* layers, int nl, int out, float lr, bool input_grad = false) {
    m.head_only = out == 0;
    if (m.head_only) nl--;  // the last hidden layer takes the output layer's slot in the loop below
    m.in = in;
    m.out = m.head_only ? layers[nl] : out;
    m.lr = lr;
    m.mode = h->cfg.train_gemm;
    m.akind = h->cfg.activation;
    m.off = h->nparams;
    int prev = in;
    for (int l = 0; l <= nl; l++) {
        Layer L;
        L.in = prev;
        const bool hidden = l < nl || m.head_only;
        L.out = l < nl ? layers[l] : m.out;
        L.w = h->nparams;
        h->nparams += (int64_t)L.in * L.out;
        L.b = h->nparams;
        h->nparams += L.out;
        L.g = L.be = -1;
        if (hidden && h->cfg.layer_norm) {
            L.g = h->nparams;
            h->nparams += L.out;
            L.be = h->nparams;
            h->nparams += L.out;
        }
        L.in_pad = (L.in + 7) / 8 * 8;
        h->nhalf = (h->nhalf + 7) / 8 * 8;
        L.hw = h->nhalf;
        h->nhalf += (int64_t)L.out * L.in_pad;
        L.hb = h->nhalf;
        h->nhalf += L.out;
        L.hg = L.hbe = -1;
        L.fw = h->nfrag;
        h->nfrag += infer::frag_size(L.out, L.in);
        if (L.g >= 0) {
            L.hg = h->nhalf;
            h->nhalf += L.out;
            L.hbe = h->nhalf;
            h->nhalf += L.out;
        }
        if (L.out > h->hmax) h->hmax = L.out;
        if (L.in > h->hmax && l > 0) h->hmax = L.in;
        if (split_mode(m.mode) && L.out > 1) {  // the rank-1 critic head has no GEMM
            const bool h3 = m.mode == RLGPU_GEMM_F16X3;
            // fragment-order copies: a hidden layer's own full row forward, and backward where a hidden layer below
            // consumes this layer's dA (the first layer's goes to the model input)
            L.fwd = add_side(m, L.out, L.in, h3 && m.akind == mlp::ACT_LEAKY && hidden && L.out == mlp::RLN_J);
            if (l > 0 || input_grad)  // dA of the first layer only behind the shared head
                L.bwd = add_side(m, L.in, L.out, h3 && m.akind == mlp::ACT_LEAKY && l > 0 && L.in == mlp::RLN_J);
        }
        m.L.push_back(L);
        prev = L.out;
    }
    m.count = h->nparams - m.off;
}

// h->scratch: [0, 512) the sum-of-squares partials, 600 + mi the clip coefficients, kScratchNorm + mi a model's gradient
// norm where no metrics buffer takes it
constexpr int kScratchNorm = 608;

// one step of a non-Adam optimizer on a model's span (ppo::optim_step); coef null: unclipped
void launch_optim_step(int kind, float* p, float* g, float* v, int64_t n, const float* coef, const float* norm, float lr,
                       hipStream_t s) {
    auto* fn = kind == RLGPU_OPT_ADAGRAD   ? &ppo::optim_step<ppo::kOptAdagrad>
               : kind == RLGPU_OPT_RMSPROP ? &ppo::optim_step<ppo::kOptRmsprop>
                                           : &ppo::optim_step<ppo::kOptMagSgd>;
    hipLaunchKernelGGL(fn, dim3(ceil_div(n, 256)), dim3(256), 0, s, p, g, v, n, coef, norm, lr);
    RLGPU_CHECK_HIP(hipGetLastError());
}

void sumsq_coef(rlgpu_ppo* h, const float* x, int64_t n, float max_norm, float* coef, float* norm_out, hipStream_t s) {
    const int nb = 512;
    hipLaunchKernelGGL(ppo::sumsq_partial, dim3(nb), dim3(256), 0, s, x, n, h->scratch);
    hipLaunchKernelGGL(ppo::clip_coef, dim3(1), dim3(64), 0, s, h->scratch, nb, max_norm, coef, norm_out);
    RLGPU_CHECK_HIP(hipGetLastError());
}

// bf16 inference copy of model mi from `src` (the model's flat fp32 parameters, torch order) into
// the padded layout at `dst` (h->half or h->half_ver)
void half_from(rlgpu_ppo* h, int mi, const float* src, uint16_t* dst, uint16_t* fdst, hipStream_t s) {
    const Model& m = h->M[mi];
    for (auto& L : m.L) {
        const int64_t nf = infer::frag_size(L.out, L.in);
        RLGPU_H16_LAUNCH(f16(h), infer::weight_to_frag, dim3(ceil_div(nf, 256)), dim3(256), 0, s, src + (L.w - m.off),
                         L.out, L.in, fdst + L.fw);
        int64_t e = (int64_t)L.out * L.in_pad;
        RLGPU_H16_LAUNCH(f16(h), mlp::weight_to_bf16, dim3(ceil_div(e, 256)), dim3(256), 0, s, src + (L.w - m.off), L.out, L.in,
                           dst + L.hw, L.in_pad);
        int nv = L.g >= 0 ? 3 * L.out : L.out;  // bias | LN weight | LN bias, contiguous in both layouts
        RLGPU_H16_LAUNCH(f16(h), ppo::to_half, dim3(ceil_div(nv, 256)), dim3(256), 0, s, src + (L.b - m.off), dst + L.hb,
                           (int64_t)nv);
    }
    RLGPU_CHECK_HIP(hipGetLastError());
}

void refresh_half(rlgpu_ppo* h, hipStream_t s) {
    for (int mi = 0; mi < h->nm; mi++) {
        half_from(h, mi, h->params + h->M[mi].off, h->half, h->frag, s);
        h->split_dirty[mi] = true;
    }
}

static_assert(mlp::ACT_LEAKY == RLGPU_ACT_LEAKY_RELU && mlp::ACT_SIGMOID == RLGPU_ACT_SIGMOID && mlp::ACT_TANH == RLGPU_ACT_TANH,
              "mlp::ACT_* are rlgpu_ppo_config.activation's values");

}  // namespace

extern "C" int32_t rlgpu_ppo_config_size(void) { return (int32_t)sizeof(rlgpu_ppo_config); }

extern "C" int rlgpu_ppo_get_config(rlgpu_ppo* h, rlgpu_ppo_config* out) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && out, "rlgpu_ppo_get_config: null argument");
        *out = h->cfg;
    });
}

extern "C" int rlgpu_ppo_create(const rlgpu_ppo_config* cfg, rlgpu_ppo** out) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(cfg && out, "rlgpu_ppo_create: null argument");
        // one action has no distribution to learn: the entropy is normalised by log(num_actions), which is 0
        RLGPU_REQUIRE(cfg->obs_size > 0 && cfg->num_actions >= 2 && cfg->num_actions <= ppo::kMaxA,
                      "num_actions must be in [2, 128]");
        // policyTemperature: 0 (a zero-initialised config) means 1; the sampler and the loss divide by it
        RLGPU_REQUIRE(std::isfinite(cfg->policy_temperature) && cfg->policy_temperature >= 0.f,
                      "policy_temperature must be finite and > 0 (0 = the default, 1)");
        RLGPU_REQUIRE(cfg->mask_entropy == 0 || cfg->mask_entropy == 1, "mask_entropy must be 0 or 1");
        RLGPU_REQUIRE(cfg->activation >= RLGPU_ACT_LEAKY_RELU && cfg->activation <= RLGPU_ACT_TANH,
                      "activation must be RLGPU_ACT_LEAKY_RELU (0), _RELU (1), _SIGMOID (2) or _TANH (3)");
        RLGPU_REQUIRE(cfg->n_policy_layers >= 1 && cfg->n_policy_layers <= RLGPU_MAX_LAYERS && cfg->n_critic_layers >= 1 &&
                          cfg->n_critic_layers <= RLGPU_MAX_LAYERS,
                      "1..8 hidden layers per model");
        RLGPU_REQUIRE(cfg->max_rows > 0, "max_rows must be > 0");
        for (int i = 0; i < cfg->n_policy_layers; i++)
            RLGPU_REQUIRE(cfg->policy_layers[i] > 0 && cfg->policy_layers[i] <= 2048, "hidden sizes must be in [1, 2048]");
        for (int i = 0; i < cfg->n_critic_layers; i++)
            RLGPU_REQUIRE(cfg->critic_layers[i] > 0 && cfg->critic_layers[i] <= 2048, "hidden sizes must be in [1, 2048]");
        RLGPU_REQUIRE(cfg->n_shared_layers >= 0 && cfg->n_shared_layers <= RLGPU_MAX_LAYERS, "0..8 shared-head layers");
        for (int i = 0; i < cfg->n_shared_layers; i++)
            RLGPU_REQUIRE(cfg->shared_layers[i] > 0 && cfg->shared_layers[i] <= 2048, "hidden sizes must be in [1, 2048]");
        auto* h = new rlgpu_ppo();
        try {
            h->cfg = *cfg;
            if (h->cfg.policy_temperature == 0.f) h->cfg.policy_temperature = 1.f;
            if (h->cfg.activation == RLGPU_ACT_RELU) {  // the kernels' LEAKY kind with slope 0
                h->cfg.activation = RLGPU_ACT_LEAKY_RELU;
                h->cfg.leaky_slope = 0.f;
            }
            const bool sh = cfg->n_shared_layers > 0;
            h->nm = sh ? 3 : 2;
            // PPOLearner::MakeModels (PPOLearner.cpp:42-74): behind a shared head the policy / critic
            // take its last width as input
            const int min = sh ? cfg->shared_layers[cfg->n_shared_layers - 1] : cfg->obs_size;
            build_model(h, h->M[0], min, cfg->policy_layers, cfg->n_policy_layers, cfg->num_actions, cfg->policy_lr, sh);
            h->nparams = (h->nparams + 63) / 64 * 64;  // 256-byte aligned model start: float4 weight rows
            build_model(h, h->M[1], min, cfg->critic_layers, cfg->n_critic_layers, 1, cfg->critic_lr, sh);
            if (sh) {  // shared head LR = min(policy, critic) (PPOLearner::SetLearningRates, :652-663)
                h->nparams = (h->nparams + 63) / 64 * 64;
                build_model(h, h->M[2], cfg->obs_size, cfg->shared_layers, cfg->n_shared_layers, 0,
                            std::min(cfg->policy_lr, cfg->critic_lr));
            }
            int64_t P = h->nparams, R = cfg->max_rows;
            h->params = h->alloc<float>(P);
            h->grads = h->alloc<float>(P);
            h->exp_avg = h->alloc<float>(P);
            h->exp_avg_sq = h->alloc<float>(P);
            h->half = h->alloc<uint16_t>(h->nhalf + 8);
            h->half_ver = h->alloc<uint16_t>(h->nhalf + 8);
            h->frag = h->alloc<uint16_t>(h->nfrag);
            h->frag_ver = h->alloc<uint16_t>(h->nfrag);
            RLGPU_CHECK_HIP(hipMemset(h->params, 0, P * 4));
            RLGPU_CHECK_HIP(hipMemset(h->grads, 0, P * 4));
            RLGPU_CHECK_HIP(hipMemset(h->exp_avg, 0, P * 4));
            RLGPU_CHECK_HIP(hipMemset(h->exp_avg_sq, 0, P * 4));
            for (int mi = 0; mi < h->nm; mi++) {
                Model& m = h->M[mi];
                const int nh = nhid(m);
                for (int l = 0; l < nh; l++) {
                    m.xhat.push_back(h->alloc<float>(R * m.L[l].out));
                    m.act.push_back(h->alloc<float>(R * m.L[l].out));
                    m.rstd.push_back(h->alloc<float>(2 * R));  // (mean, rstd) per row
                }
            }
            int H = h->hmax;
            int omax = cfg->num_actions > 1 ? cfg->num_actions : 1;
            {
                int dev = 0, cus = 256;
                if (hipGetDevice(&dev) == hipSuccess) {
                    hipDeviceProp_t prop;
                    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
                        cus = prop.multiProcessorCount;
                }
                g_cus = cus;
            }
            // most blocks of any kernel that writes per-block partials: the LayerNorm backward variants and the policy
            // loss (a 256-row column-sum pass once shared these buffers; 256 was never the minimum, so nb is what it was)
            int64_t nb = ceil_div(R, std::min(mlp::LNB_ROWS_MIN, ppo::PL_ROWS));
            for (int mi = 0; mi < h->nm; mi++) {
                Model& m = h->M[mi];
                if (!m.head_only) {
                    m.y = h->alloc<float>(R * omax);
                    m.dy = h->alloc<float>(R * ((omax + 3) / 4 * 4));
                }
                if (sh && mi < 2) m.dX = h->alloc<float>(R * (int64_t)m.in);  // input gradient behind the shared head
                m.dA = h->alloc<float>(R * H);
                m.dZ = h->alloc<float>(R * H);
                m.hpart = h->alloc<float>(nb * ((int64_t)H + 1));
                // the deferred reductions' per-layer partials and level-1 rows (Reducer); splits_for is
                // non-decreasing in the row count, and a launch's ceil(n / chunk) partials are at most its splits
                for (auto& L : m.L) {
                    m.wpart_l.push_back(h->alloc<float>((int64_t)splits_for(m.mode, (int)R, L.out, L.in) * L.in * L.out));
                    m.cpart_l.push_back(h->alloc<float>(nb * 3 * (int64_t)L.out));
                }
                m.lpart = h->alloc<float>(nb * (int64_t)omax);
                m.midn = 3 * (int64_t)std::max(std::max(H, omax) + 1, 1024);
                m.mid = h->alloc<float>((int64_t)mlp::kRedJobs * 16 * m.midn);
                if (m.nsplit) m.wsplit = h->alloc<uint16_t>(m.nsplit);
                if (m.mode == RLGPU_GEMM_F16X3 && m.nscale) m.wscale = h->alloc<float>(m.nscale);
            }
            if (sh) h->dshared = h->alloc<float>(R * (int64_t)h->M[2].out);
            if (cfg->train_gemm == RLGPU_GEMM_F16X3) {  // operand-scale shards: every model's slots + the obs
                h->amax_count = (3 * (int64_t)kAmaxSlots + 1) * 64;
                h->amax_all = h->alloc<float>(h->amax_count);
                RLGPU_CHECK_HIP(hipMemset(h->amax_all, 0, h->amax_count * sizeof(float)));
                for (int mi = 0; mi < 3; mi++) h->M[mi].amax = h->amax_all + (int64_t)mi * kAmaxSlots * 64;
                h->x_amax = h->amax_all + 3 * (int64_t)kAmaxSlots * 64;
            }
            RLGPU_CHECK_HIP(hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking));
            RLGPU_CHECK_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
            RLGPU_CHECK_HIP(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
            h->scratch = h->alloc<float>(2048 + 16 * 3 * 1024);
            h->x_ld = (cfg->obs_size + 3) / 4 * 4;
            h->x0 = h->alloc<float>(R * h->x_ld);
            h->xh_ld = (cfg->obs_size + 7) / 8 * 8;
            h->xh = h->alloc<uint16_t>(R * h->xh_ld);
            h->zh = h->alloc<uint16_t>(R * H);
            h->ah[0] = h->alloc<uint16_t>(R * H);
            h->ah[1] = h->alloc<uint16_t>(R * H);
            h->logits_h = h->alloc<uint16_t>(R * omax);
            if (cfg->infer_fp16 == RLGPU_INFER_F32) h->logits_f = h->alloc<float>(R * omax);
            build_chains(h);
            *out = h;
        } catch (...) {
            for (void* p : h->allocs) rlgpu::dev_free(p);
            delete h;
            throw;
        }
    });
}

extern "C" int rlgpu_ppo_destroy(rlgpu_ppo* h) {
    return rlgpu::guarded([&] {
        if (!h) return;
        if (h->aux) (void)hipStreamSynchronize(h->aux);
        if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
        if (h->ev_join) (void)hipEventDestroy(h->ev_join);
        if (h->aux) (void)hipStreamDestroy(h->aux);
        for (void* p : h->allocs) rlgpu::dev_free(p);
        delete h;
    });
}

extern "C" int rlgpu_ppo_buffers(rlgpu_ppo* h, float** d_params, float** d_grads, int64_t* num_params) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h, "null handle");
        if (d_params) *d_params = h->params;
        if (d_grads) *d_grads = h->grads;
        if (num_params) *num_params = h->nparams;
    });
}

extern "C" int rlgpu_ppo_model_range(rlgpu_ppo* h, int32_t model, int64_t* offset, int64_t* count) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && model >= 0 && model <= 2, "model must be 0 (policy), 1 (critic) or 2 (shared head)");
        const bool present = model < h->nm;
        if (offset) *offset = present ? h->M[model].off : h->nparams;
        if (count) *count = present ? h->M[model].count : 0;
    });
}

extern "C" int rlgpu_ppo_init_params(rlgpu_ppo* h, uint64_t seed, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h, "null handle");
        hipStream_t s = rlgpu::as_stream(stream);
        uint32_t sid = 0;  // Philox stream per tensor, in model order (policy, critic, shared head)
        for (int mi = 0; mi < h->nm; mi++)
            for (auto& L : h->M[mi].L) {
                float bound = 1.f / std::sqrt((float)L.in);
                int64_t nw = (int64_t)L.in * L.out;
                hipLaunchKernelGGL(ppo::init_uniform, dim3(ceil_div(nw, 256)), dim3(256), 0, s, h->params + L.w, nw, bound, seed,
                                   sid++);
                hipLaunchKernelGGL(ppo::init_uniform, dim3(ceil_div(L.out, 256)), dim3(256), 0, s, h->params + L.b,
                                   (int64_t)L.out, bound, seed, sid++);
                if (L.g >= 0) {
                    hipLaunchKernelGGL(ppo::fill, dim3(ceil_div(L.out, 256)), dim3(256), 0, s, h->params + L.g, (int64_t)L.out,
                                       1.f);
                    hipLaunchKernelGGL(ppo::fill, dim3(ceil_div(L.out, 256)), dim3(256), 0, s, h->params + L.be, (int64_t)L.out,
                                       0.f);
                }
            }
        RLGPU_CHECK_HIP(hipGetLastError());
        refresh_half(h, s);
    });
}

extern "C" int rlgpu_ppo_refresh_half(rlgpu_ppo* h, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h, "null handle");
        refresh_half(h, rlgpu::as_stream(stream));
    });
}

extern "C" int rlgpu_ppo_forward(rlgpu_ppo* h, int32_t model, int32_t precision, const float* d_in, int32_t n, float* d_out,
                                 void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_in && d_out, "null argument");
        RLGPU_REQUIRE(model >= 0 && model < h->nm, "model must be 0, 1 or (with a shared head) 2");
        RLGPU_REQUIRE(n >= 0 && n <= h->cfg.max_rows, "n must be in [0, max_rows]");
        if (n == 0) return;
        hipStream_t s = rlgpu::as_stream(stream);
        if (precision != 0) return infer_values(h, model, Rows{d_in, n, 0, nullptr}, d_out, s, true);
        if (model != 2) return forward_f32(h, model, d_in, n, d_out, s);
        // the shared head's last activation
        gather_obs(h, d_in, nullptr, 0, n, s);
        forward_train(h, 2, obs_input(h), n, nullptr, s);
        RLGPU_CHECK_HIP(hipMemcpyAsync(d_out, model_input(h, 0).X, (int64_t)n * h->M[2].out * sizeof(float),
                                       hipMemcpyDeviceToDevice, s));
    });
}

extern "C" int rlgpu_ppo_infer_actions(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, int32_t n,
                                       int32_t deterministic, uint64_t rng_step, int32_t* d_actions, float* d_logp,
                                       void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_obs && d_masks && d_actions, "null argument");
        RLGPU_REQUIRE(n >= 0, "n must be >= 0");
        infer_policy(h, Rows{d_obs, n, h->cfg.sample_row_offset, d_masks}, Draw{deterministic, rng_step, d_actions, d_logp},
                     nullptr, h->cfg.max_rows, rlgpu::as_stream(stream));
    });
}

extern "C" int rlgpu_debug_infer_trace(void* d_buf, int64_t capacity) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(!d_buf || capacity >= 16, "rlgpu_debug_infer_trace: capacity below one workgroup's 16 marks");
        g_infer_trace = (unsigned long long*)d_buf;
        g_infer_trace_cap = d_buf ? capacity : 0;
    });
}

extern "C" int rlgpu_ppo_set_version(rlgpu_ppo* h, const float* d_policy_params, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_policy_params, "rlgpu_ppo_set_version: null argument");
        hipStream_t s = rlgpu::as_stream(stream);
        half_from(h, 0, d_policy_params, h->half_ver, h->frag_ver, s);
        // the version's shared head follows its policy (GetPolicyModels, PPOLearner.cpp:665-674)
        if (h->shared()) half_from(h, 2, d_policy_params + h->M[0].count, h->half_ver, h->frag_ver, s);
        h->has_ver = true;
    });
}

static_assert(ppo::kGuidingLossSlot == RLGPU_M_GUIDING_LOSS, "the guided loss kernel's metric slot");

extern "C" int rlgpu_ppo_set_guide(rlgpu_ppo* h, const float* d_policy_params, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_policy_params, "rlgpu_ppo_set_guide: null argument");
        if (infer_f32(h))
            throw rlgpu::Error(RLGPU_ERR_UNSUPPORTED, "rlgpu_ppo_set_guide: fp32 inference (RLGPU_INFER_F32) keeps no 16-bit "
                                                      "copies (a guiding policy needs 16-bit inference)");
        hipStream_t s = rlgpu::as_stream(stream);
        if (!h->half_guide) {  // the first guide: its copies and the fused pass's f32 chunk
            h->half_guide = h->alloc<uint16_t>(h->nhalf + 8);
            h->frag_guide = h->alloc<uint16_t>(h->nfrag);
            h->guide_f = h->alloc<float>((int64_t)h->cfg.max_rows * h->cfg.num_actions);
        }
        half_from(h, 0, d_policy_params, h->half_guide, h->frag_guide, s);
        // the guide's shared head follows its policy, as an old version's does
        if (h->shared()) half_from(h, 2, d_policy_params + h->M[0].count, h->half_guide, h->frag_guide, s);
        h->has_guide = true;
    });
}

extern "C" int rlgpu_ppo_infer_guide_logits(rlgpu_ppo* h, const float* d_obs, int64_t n, uint16_t* d_logits16, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_obs && d_logits16 && n >= 0, "rlgpu_ppo_infer_guide_logits: bad argument");
        RLGPU_REQUIRE(h->has_guide, "rlgpu_ppo_infer_guide_logits: no guide set (rlgpu_ppo_set_guide)");
        hipStream_t s = rlgpu::as_stream(stream);
        const int A = h->cfg.num_actions;
        const Rows rows{d_obs, n, 0, nullptr};
        // chunks of max_rows on both paths: the fused kernel's f32 outputs go through guide_f, the layered kernels
        // work in the per-handle row buffers
        for (int64_t b = 0; b < n; b += h->cfg.max_rows) {
            const Rows r = rows.sub(h->cfg, b, std::min<int64_t>(h->cfg.max_rows, n - b));
            const int64_t e = r.n * A;
            uint16_t* out = d_logits16 + b * A;
            if (fused_ok(h, 0)) {
                infer_fused(h, 0, Weights::Guide, r, h->guide_f, nullptr, s);
                // exact: the kernel's f32 outputs are 16-bit-rounded values
                RLGPU_H16_LAUNCH(f16(h), ppo::to_half, dim3(ceil_div(e, 256)), dim3(256), 0, s, h->guide_f, out, e);
                RLGPU_CHECK_HIP(hipGetLastError());
            } else {
                const uint16_t* y = forward_half(h, 0, r.X, (int)r.n, s, h->half_guide);
                RLGPU_CHECK_HIP(hipMemcpyAsync(out, y, e * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
            }
        }
    });
}

extern "C" int rlgpu_ppo_infer_actions_mixed(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, int32_t n,
                                             int32_t deterministic, uint64_t rng_step, const uint8_t* d_old_rows,
                                             int32_t* d_actions, float* d_logp, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_obs && d_masks && d_actions && d_old_rows, "null argument");
        RLGPU_REQUIRE(h->has_ver, "rlgpu_ppo_infer_actions_mixed: no version set (rlgpu_ppo_set_version)");
        if (infer_f32(h))
            throw rlgpu::Error(RLGPU_ERR_UNSUPPORTED, "rlgpu_ppo_infer_actions_mixed: fp32 inference (RLGPU_INFER_F32) "
                                                      "keeps no old-version copy (self-play needs 16-bit inference)");
        RLGPU_REQUIRE(n >= 0, "n must be >= 0");
        infer_policy(h, Rows{d_obs, n, h->cfg.sample_row_offset, d_masks}, Draw{deterministic, rng_step, d_actions, d_logp},
                     d_old_rows, h->cfg.max_rows, rlgpu::as_stream(stream));
    });
}

extern "C" int rlgpu_ppo_infer_actions_rows(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, int32_t n, int64_t row0,
                                            int32_t deterministic, uint64_t rng_step, const uint8_t* d_old_rows,
                                            int32_t* d_actions, float* d_logp, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_obs && d_masks && d_actions, "null argument");
        RLGPU_REQUIRE(n >= 0 && row0 >= 0, "n and row0 must be >= 0");
        RLGPU_REQUIRE(!d_old_rows || h->has_ver, "rlgpu_ppo_infer_actions_rows: old rows without a version set");
        if (!fused_ok(h, 0))
            throw rlgpu::Error(RLGPU_ERR_UNSUPPORTED, "rlgpu_ppo_infer_actions_rows: the policy is not on the fused kernel "
                                                      "(widths, RLGPU_FUSED_INFER = 0 or fp32 inference)");
        const Rows rows{d_obs, n, row0 + h->cfg.sample_row_offset, d_masks};
        infer_policy(h, rows, Draw{deterministic, rng_step, d_actions, d_logp}, d_old_rows, INT64_MAX, rlgpu::as_stream(stream));
    });
}

bool rlgpu::ppo_wave_policy(rlgpu_ppo* h, int obs_size, int num_actions) {
    return h && wave_ok(h, 0) && h->cfg.obs_size == obs_size && h->cfg.num_actions == num_actions;
}
void rlgpu::ppo_wave_args(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, int64_t n, int deterministic,
                          uint64_t rng_step, int32_t* d_actions, float* d_logp, void* blob, size_t cap, bool* f16_out) {
    RLGPU_REQUIRE(h && wave_ok(h, 0), "ppo_wave_args: the policy is not on the one-wave kernel");
    const Draw d{deterministic, rng_step, d_actions, d_logp};
    const infer::InferArgs a = fused_args(h, 0, Weights::Current, Rows{d_obs, n, h->cfg.sample_row_offset, d_masks}, nullptr, &d);
    RLGPU_REQUIRE(sizeof(a) <= cap, "ppo_wave_args: InferArgs do not fit the blob");
    std::memcpy(blob, &a, sizeof(a));
    *f16_out = f16(h);
}

void rlgpu::ppo_widths(rlgpu_ppo* h, int* obs_size, int* num_actions) {
    RLGPU_REQUIRE(h, "null policy handle");
    *obs_size = h->cfg.obs_size;
    *num_actions = h->cfg.num_actions;
}
// fused_args and sample_pass read the temperature from the handle's config: it holds the call's for the time of the
// enqueue (a handle is used from one thread at a time, as everywhere in this ABI)
void rlgpu::ppo_infer_actions_temp(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, int64_t n, int64_t row0,
                                   int deterministic, float temperature, uint64_t rng_step, int32_t* d_actions, float* d_logp,
                                   hipStream_t s) {
    RLGPU_REQUIRE(h && d_obs && d_masks && d_actions && n >= 0 && row0 >= 0, "ppo_infer_actions_temp: bad argument");
    struct Restore {
        float& slot;
        float old;
        ~Restore() { slot = old; }
    } restore{h->cfg.policy_temperature, h->cfg.policy_temperature};
    h->cfg.policy_temperature = temperature;
    infer_policy(h, Rows{d_obs, n, row0 + h->cfg.sample_row_offset, d_masks}, Draw{deterministic, rng_step, d_actions, d_logp},
                 nullptr, h->cfg.max_rows, s);
}

extern "C" int rlgpu_ppo_wave_infer(rlgpu_ppo* h, int32_t model) { return h && model >= 0 && model < 3 && wave_ok(h, model); }

extern "C" int rlgpu_ppo_infer_actions_wave(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, int32_t n, int64_t row0,
                                            int32_t deterministic, uint64_t rng_step, const uint8_t* d_old_rows,
                                            int32_t* d_actions, float* d_logp, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_obs && d_masks && d_actions, "null argument");
        RLGPU_REQUIRE(n >= 0 && row0 >= 0, "n and row0 must be >= 0");
        RLGPU_REQUIRE(!d_old_rows || h->has_ver, "rlgpu_ppo_infer_actions_wave: old rows without a version set");
        if (!wave_ok(h, 0))
            throw rlgpu::Error(RLGPU_ERR_UNSUPPORTED, "rlgpu_ppo_infer_actions_wave: the policy is not eligible for the one-wave "
                                                      "kernel (the fused kernel's conditions and LeakyReLU / ReLU)");
        if (n == 0) return;
        const Rows rows{d_obs, n, row0 + h->cfg.sample_row_offset, d_masks};
        Draw d{deterministic, rng_step, d_actions, d_logp, d_old_rows, 0};
        for (d.sel = 0; d.sel < (d_old_rows ? 2 : 1); d.sel++) {  // infer_policy's passes, unchunked
            if (d.sel) d.logp = nullptr;
            infer_fused(h, 0, version_if(d.sel != 0), rows, nullptr, &d, rlgpu::as_stream(stream), true);
        }
    });
}

extern "C" int rlgpu_ppo_infer_values_wave(rlgpu_ppo* h, int32_t model, const float* d_obs, int32_t n, float* d_out,
                                           void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_obs && d_out && n >= 0 && model >= 0 && model < 2, "rlgpu_ppo_infer_values_wave: bad argument");
        if (!wave_ok(h, model))
            throw rlgpu::Error(RLGPU_ERR_UNSUPPORTED, "rlgpu_ppo_infer_values_wave: the model is not eligible for the one-wave "
                                                      "kernel (the fused kernel's conditions and LeakyReLU / ReLU)");
        if (n == 0) return;
        infer_fused(h, model, Weights::Current, Rows{d_obs, n, 0, nullptr}, d_out, nullptr, rlgpu::as_stream(stream), true);
    });
}

extern "C" int rlgpu_ppo_fused_infer(rlgpu_ppo* h, int32_t model) { return h && model >= 0 && model < 3 && fused_ok(h, model); }

extern "C" int rlgpu_ppo_infer_critic(rlgpu_ppo* h, const float* d_obs, int64_t n, float* d_values, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_obs && d_values, "null argument");
        hipStream_t s = rlgpu::as_stream(stream);
        const Rows rows{d_obs, n, 0, nullptr};
        const int64_t R = fused_ok(h, 1) ? (int64_t)1 << 30 : h->cfg.max_rows;  // see infer_policy on chunking
        for (int64_t b = 0; b < n; b += R) infer_values(h, 1, rows.sub(h->cfg, b, std::min(R, n - b)), d_values + b, s);
    });
}

extern "C" int rlgpu_mean_std(const float* d_x, int64_t n, float* d_out, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(d_x && d_out && n > 0, "rlgpu_mean_std: bad argument");
        hipStream_t s = rlgpu::as_stream(stream);
        const int nb = 256;
        double* part = nullptr;
        RLGPU_CHECK_HIP(hipMallocAsync((void**)&part, nb * 2 * sizeof(double), s));
        hipLaunchKernelGGL(ppo::moments_partial, dim3(nb), dim3(256), 0, s, d_x, n, part);
        hipLaunchKernelGGL(ppo::moments_final, dim3(1), dim3(64), 0, s, part, nb, n, d_out);
        RLGPU_CHECK_HIP(hipGetLastError());
        RLGPU_CHECK_HIP(hipFreeAsync(part, s));
    });
}

extern "C" int rlgpu_ppo_minibatch(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, const int32_t* d_actions,
                                   const float* d_old_logp, const float* d_adv, const float* d_target, const int32_t* d_index,
                                   int64_t start, int32_t n, int64_t batch_size, const float* d_adv_stats, float* d_metrics,
                                   void* stream) {
    return rlgpu_ppo_minibatch_guided(h, d_obs, d_masks, d_actions, d_old_logp, d_adv, d_target, d_index, start, n, batch_size,
                                      d_adv_stats, nullptr, 0.f, d_metrics, stream);
}

extern "C" int rlgpu_ppo_minibatch_guided(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, const int32_t* d_actions,
                                          const float* d_old_logp, const float* d_adv, const float* d_target,
                                          const int32_t* d_index, int64_t start, int32_t n, int64_t batch_size,
                                          const float* d_adv_stats, const uint16_t* d_guide_logits, float guiding_strength,
                                          float* d_metrics, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_obs && d_masks && d_actions && d_old_logp && d_adv && d_target && d_adv_stats,
                      "rlgpu_ppo_minibatch: null argument");
        RLGPU_REQUIRE(n > 0 && n <= h->cfg.max_rows, "minibatch rows must be in [1, max_rows]");
        RLGPU_REQUIRE(batch_size > 0, "batch_size must be > 0");
        RLGPU_REQUIRE(std::isfinite(guiding_strength) && guiding_strength >= 0.f, "guiding_strength must be finite and >= 0");
        if (d_guide_logits && infer_f32(h))
            throw rlgpu::Error(RLGPU_ERR_UNSUPPORTED, "rlgpu_ppo_minibatch_guided: guide logits on an fp32-inference handle "
                                                      "(RLGPU_INFER_F32 has no 16-bit logit format)");
        hipStream_t s = rlgpu::as_stream(stream);
        float bsr = (float)n / (float)batch_size;  // PPOLearner.cpp:374
        int A = h->cfg.num_actions;
        gather_obs(h, d_obs, d_index, start, n, s);  // one gathered, padded copy serves both models
        // the shared head's forward once per minibatch (PPOLearner.cpp:395-398); policy and critic read it
        const Operand obs_in = obs_input(h), xin = model_input(h, 0);
        if (h->shared()) forward_train(h, 2, obs_in, n, nullptr, s);
        // the critic's pass runs on the auxiliary stream (disjoint parameters, gradients, workspace
        // and metric slots), overlapping the policy's; the caller's stream waits for both
        hipStream_t cs = h->aux;
        RLGPU_CHECK_HIP(hipEventRecord(h->ev_fork, s));
        RLGPU_CHECK_HIP(hipStreamWaitEvent(h->aux, h->ev_fork, 0));
        Model& pm = h->M[0];
        Model& cm = h->M[1];
        forward_train(h, 1, xin, n, cm.y, cs);
        hipLaunchKernelGGL(ppo::critic_loss, dim3(ceil_div(n, 256)), dim3(256), 0, cs, cm.y, d_target, d_index, start, n,
                           bsr, cm.dy, d_metrics);
        RLGPU_CHECK_HIP(hipGetLastError());
        backward(h, 1, xin, n, cm.dy, cs);
        RLGPU_CHECK_HIP(hipEventRecord(h->ev_join, h->aux));
        // policy on the caller's stream
        forward_train(h, 0, xin, n, pm.y, s);
        const int pl_blocks = (int)ceil_div(n, ppo::PL_ROWS);
        // the kernel that knows policy_temperature / mask_entropy only when one of them is set: the defaults run the
        // kernel without them (see policy_loss on why x / 1 alone does not keep the bits)
        const bool pl_opt = h->cfg.policy_temperature != 1.f || h->cfg.mask_entropy != 0;
        // a guide takes the guided instance of its logit format (always with the options' semantics);
        // d loss / d c = strength / (n A) sign
        const int guide = d_guide_logits ? (f16(h) ? 2 : 1) : 0;
        hipLaunchKernelGGL(ppo::policy_loss_any(A, pl_opt, guide), dim3(pl_blocks), dim3(256), 0, s, pm.y, d_masks, d_actions,
                           d_old_logp, d_adv, d_index, start, n, A, d_adv_stats, bsr, h->cfg.clip_range, h->cfg.entropy_scale,
                           1.f / std::log((float)A), h->cfg.policy_temperature, h->cfg.mask_entropy, pm.dy, dout_ld(A),
                           d_metrics, pm.lpart, amax_slot(pm, kAmaxOut), d_guide_logits,
                           d_guide_logits ? guiding_strength / ((float)n * (float)A) : 0.f);
        RLGPU_CHECK_HIP(hipGetLastError());
        backward(h, 0, xin, n, pm.dy, s, pm.lpart, pl_blocks);
        RLGPU_CHECK_HIP(hipStreamWaitEvent(s, h->ev_join, 0));
        if (h->shared()) {  // (ppoLoss + criticLoss).backward() through the shared features (:498)
            const int64_t e = (int64_t)n * h->M[2].out;
            hipLaunchKernelGGL(ppo::add2, dim3(ceil_div(ceil_div(e, 4), 256)), dim3(256), 0, s, pm.dX, cm.dX, h->dshared, e);
            RLGPU_CHECK_HIP(hipGetLastError());
            backward(h, 2, obs_in, n, h->dshared, s);
        }
    });
}

extern "C" int rlgpu_ppo_optimizer_step(rlgpu_ppo* h, float* d_metrics, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h, "null handle");
        hipStream_t s = rlgpu::as_stream(stream);
        const auto& c = h->cfg;
        const int slot[3] = {RLGPU_M_GRAD_NORM_POLICY, RLGPU_M_GRAD_NORM_CRITIC, RLGPU_M_GRAD_NORM_SHARED};
        for (int mi = 0; mi < h->nm; mi++) {
            Model& m = h->M[mi];
            h->step[mi]++;
            double bc1 = 1.0 - std::pow((double)c.beta1, (double)h->step[mi]);
            double bc2 = 1.0 - std::pow((double)c.beta2, (double)h->step[mi]);
            float* coef = h->scratch + 600 + mi;
            float* norm_out = d_metrics ? d_metrics + slot[mi] : nullptr;
            const bool adam = h->opt[mi] == RLGPU_OPT_ADAMW || h->opt[mi] == RLGPU_OPT_ADAM;
            // MagSGD reads the norm back on the device: without a metrics buffer it goes to the scratch
            if (h->opt[mi] == RLGPU_OPT_MAGSGD && !norm_out) norm_out = h->scratch + kScratchNorm + mi;
            sumsq_coef(h, h->grads + m.off, m.count, c.max_grad_norm, coef, norm_out, s);
            h->opt_stepped[mi] = true;
            if (!adam) {
                launch_optim_step(h->opt[mi], h->params + m.off, h->grads + m.off, h->exp_avg_sq + m.off, m.count, coef,
                                  norm_out, (float)m.lr, s);
                continue;
            }
            double lr = m.lr;
            float decay_mul = (float)(1.0 - lr * (double)c.weight_decay);
            float step_size = (float)(lr / bc1);
            float bc2_sqrt = (float)std::sqrt(bc2);
            hipLaunchKernelGGL(ppo::adamw, dim3(ceil_div(m.count, 256)), dim3(256), 0, s, h->params + m.off, h->grads + m.off,
                               h->exp_avg + m.off, h->exp_avg_sq + m.off, m.count, coef, decay_mul, c.beta1,
                               c.beta2, 1.f - c.beta1, 1.f - c.beta2, step_size, bc2_sqrt, c.eps);
            RLGPU_CHECK_HIP(hipGetLastError());
        }
        refresh_half(h, s);  // Model::Forward's lazily refreshed seqHalf (Models.cpp:46-66)
    });
}

extern "C" int rlgpu_ppo_zero_grad(rlgpu_ppo* h, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h, "null handle");
        RLGPU_CHECK_HIP(hipMemsetAsync(h->grads, 0, h->nparams * sizeof(float), rlgpu::as_stream(stream)));
    });
}

extern "C" int rlgpu_ppo_optimizer_state(rlgpu_ppo* h, int64_t* step, float** d_exp_avg, float** d_exp_avg_sq) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h, "null handle");
        if (step) *step = h->step[0];
        if (d_exp_avg) *d_exp_avg = h->exp_avg;
        if (d_exp_avg_sq) *d_exp_avg_sq = h->exp_avg_sq;
    });
}

extern "C" int rlgpu_ppo_set_optimizer(rlgpu_ppo* h, int32_t model, int32_t type) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h, "null handle");
        RLGPU_REQUIRE(model >= -1 && model < h->nm, "rlgpu_ppo_set_optimizer: model must be -1 (every model) or one of the handle's");
        RLGPU_REQUIRE(type >= RLGPU_OPT_ADAMW && type <= RLGPU_OPT_MAGSGD,
                      "rlgpu_ppo_set_optimizer: type must be RLGPU_OPT_ADAMW, ADAM, ADAGRAD, RMSPROP or MAGSGD");
        for (int mi = 0; mi < h->nm; mi++)
            RLGPU_REQUIRE((model >= 0 && model != mi) || !h->opt_stepped[mi],
                          "rlgpu_ppo_set_optimizer: the model's optimizer has already stepped (set the type before the first step)");
        for (int mi = 0; mi < h->nm; mi++)
            if (model < 0 || model == mi) h->opt[mi] = type;
    });
}

extern "C" int rlgpu_ppo_get_optimizer(rlgpu_ppo* h, int32_t model, int32_t* type) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && type && model >= 0 && model < h->nm, "rlgpu_ppo_get_optimizer: bad argument");
        *type = h->opt[model];
    });
}

extern "C" int rlgpu_ppo_set_optimizer_step(rlgpu_ppo* h, int64_t step) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && step >= 0, "rlgpu_ppo_set_optimizer_step: bad argument");
        for (int mi = 0; mi < 3; mi++) h->step[mi] = step;
    });
}

extern "C" int rlgpu_ppo_model_optimizer_step(rlgpu_ppo* h, int32_t model, int64_t* step) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && step && model >= 0 && model < h->nm, "rlgpu_ppo_model_optimizer_step: bad argument");
        *step = h->step[model];
    });
}

extern "C" int rlgpu_ppo_set_model_optimizer_step(rlgpu_ppo* h, int32_t model, int64_t step) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && step >= 0 && model >= 0 && model < h->nm, "rlgpu_ppo_set_model_optimizer_step: bad argument");
        h->step[model] = step;
    });
}

// ---- transfer learning: the kernels are transfer.hip's (transfer_kernels.hpp), launched through common.hpp
static_assert(RLGPU_M_TL_LOSS == 11 && RLGPU_M_TL_ACCURACY == 12 && RLGPU_M_TL_OLD_ENTROPY == 13 && RLGPU_M_ENTROPY == 0,
              "the transfer kernels' metric slots (transfer_kernels.hpp: kTlLossSlot, kTlAccuracySlot, kTlOldEntropySlot)");

namespace {
void check_teacher_shapes(int64_t n, int A_old, const int32_t* map, int A_out) {
    RLGPU_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "teacher_probs: n must be in [0, 2^31)");
    RLGPU_REQUIRE(A_old >= 2 && A_old <= ppo::kMaxA && A_out >= 2 && A_out <= ppo::kMaxA,
                  "teacher_probs: the action counts must be in [2, 128]");
    RLGPU_REQUIRE(map || A_out == A_old, "teacher_probs: without an action map A_out must be the teacher's num_actions");
}
}  // namespace

extern "C" int rlgpu_teacher_probs_from_logits(const float* d_logits, const uint8_t* d_masks, int64_t n, int32_t A_old,
                                               const int32_t* d_action_map, int32_t A_out, float policy_temperature,
                                               int32_t mask_entropy, float* d_probs, int32_t* d_argmax, float* d_metrics,
                                               void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(d_logits && d_masks && d_probs && d_argmax, "rlgpu_teacher_probs_from_logits: null argument");
        check_teacher_shapes(n, A_old, d_action_map, A_out);
        RLGPU_REQUIRE(std::isfinite(policy_temperature) && policy_temperature > 0.f, "policy_temperature must be finite and > 0");
        rlgpu::launch_teacher_probs({d_logits, d_masks, (int)n, A_old, d_action_map, A_out, policy_temperature, mask_entropy != 0, n,
                                     d_probs, d_argmax, d_metrics},
                                    rlgpu::as_stream(stream));
    });
}

extern "C" int rlgpu_ppo_teacher_probs(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, int64_t n,
                                       const int32_t* d_action_map, int32_t A_out, float* d_probs, int32_t* d_argmax,
                                       float* d_metrics, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_obs && d_masks && d_probs && d_argmax, "rlgpu_ppo_teacher_probs: null argument");
        const int A_old = h->cfg.num_actions;
        check_teacher_shapes(n, A_old, d_action_map, A_out);
        hipStream_t s = rlgpu::as_stream(stream);
        if (!h->teach_f) h->teach_f = h->alloc<float>((int64_t)h->cfg.max_rows * A_old);
        const Rows rows{d_obs, n, 0, d_masks};
        for (int64_t b = 0; b < n; b += h->cfg.max_rows) {
            const Rows r = rows.sub(h->cfg, b, std::min<int64_t>(h->cfg.max_rows, n - b));
            infer_values(h, 0, r, h->teach_f, s);  // the handle's inference path: fp32, fused or layered 16-bit
            rlgpu::launch_teacher_probs({h->teach_f, r.masks, (int)r.n, A_old, d_action_map ? d_action_map + b * A_out : nullptr,
                                         A_out, h->cfg.policy_temperature, h->cfg.mask_entropy, n, d_probs + b * A_out,
                                         d_argmax + b, d_metrics},
                                        s);
        }
    });
}

extern "C" int rlgpu_ppo_transfer_chunk(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, const float* d_target_probs,
                                        const int32_t* d_target_argmax, const int32_t* d_index, int64_t start, int32_t n,
                                        int64_t total_rows, int32_t use_kl, float loss_scale, float loss_exponent,
                                        float* d_metrics, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && d_obs && d_masks && d_target_probs && d_target_argmax, "rlgpu_ppo_transfer_chunk: null argument");
        RLGPU_REQUIRE(n > 0 && n <= h->cfg.max_rows, "chunk rows must be in [1, max_rows]");
        RLGPU_REQUIRE(start >= 0 && start + n <= total_rows, "the chunk's rows [start, start + n) must lie inside total_rows");
        RLGPU_REQUIRE(std::isfinite(loss_scale), "loss_scale must be finite");
        RLGPU_REQUIRE(std::isfinite(loss_exponent) && loss_exponent >= 1.f,
                      "loss_exponent must be finite and >= 1: below 1 the loss's backward is inf * 0 = NaN on every masked "
                      "column (|old - new| = 0 there), in the reference too");
        hipStream_t s = rlgpu::as_stream(stream);
        const int A = h->cfg.num_actions;
        Model& pm = h->M[0];
        gather_obs(h, d_obs, d_index, start, n, s);
        const Operand obs_in = obs_input(h), xin = model_input(h, 0);
        if (h->shared()) forward_train(h, 2, obs_in, n, nullptr, s);
        forward_train(h, 0, xin, n, pm.y, s);
        rlgpu::launch_transfer_loss({pm.y, d_masks, d_target_probs, d_target_argmax, d_index, start, n, A,
                                     h->cfg.policy_temperature, h->cfg.mask_entropy, total_rows, use_kl != 0, loss_scale,
                                     loss_exponent, pm.dy, dout_ld(A), d_metrics, pm.lpart, amax_slot(pm, kAmaxOut)},
                                    s);
        backward(h, 0, xin, n, pm.dy, s, pm.lpart, rlgpu::transfer_loss_blocks(n));
        // the shared head's backward from the policy's input gradient alone: the critic has no part in this loss
        if (h->shared()) backward(h, 2, obs_in, n, pm.dX, s);
    });
}

extern "C" int rlgpu_ppo_transfer_step(rlgpu_ppo* h, float lr, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(h && std::isfinite(lr) && lr >= 0.f, "rlgpu_ppo_transfer_step: lr must be finite and >= 0");
        hipStream_t s = rlgpu::as_stream(stream);
        const auto& c = h->cfg;
        for (int mi = 0; mi < h->nm; mi += 2) {  // GetPolicyModels(): the policy and the shared head
            Model& m = h->M[mi];
            h->step[mi]++;
            h->opt_stepped[mi] = true;
            if (h->opt[mi] == RLGPU_OPT_ADAMW || h->opt[mi] == RLGPU_OPT_ADAM) {
                // rlgpu_ppo_optimizer_step's scalars with lr in place of the model's
                const double bc1 = 1.0 - std::pow((double)c.beta1, (double)h->step[mi]);
                const double bc2 = 1.0 - std::pow((double)c.beta2, (double)h->step[mi]);
                const double dlr = lr;
                rlgpu::launch_adam_models(h->params + m.off, h->grads + m.off, h->exp_avg + m.off, h->exp_avg_sq + m.off,
                                          m.count, (float)(1.0 - dlr * (double)c.weight_decay), c.beta1, c.beta2,
                                          (float)(dlr / bc1), (float)std::sqrt(bc2), c.eps, s);
            } else {  // optim_step without a clip coefficient; MagSGD's own reduction goes through the scratch
                rlgpu::launch_optim_models(h->opt[mi], h->params + m.off, h->grads + m.off, h->exp_avg_sq + m.off, m.count, lr,
                                           h->scratch, h->scratch + kScratchNorm + mi, s);
            }
            half_from(h, mi, h->params + m.off, h->half, h->frag, s);
            h->split_dirty[mi] = true;
        }
    });
}

extern "C" int rlgpu_diff_norm(const float* d_a, const float* d_b, int64_t n, float* d_out, float* d_scratch, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(d_a && d_b && d_out && n >= 0, "rlgpu_diff_norm: bad argument");
        hipStream_t s = rlgpu::as_stream(stream);
        float* part = d_scratch;  // the caller's 512 floats, or a stream-ordered temporary
        if (!part) RLGPU_CHECK_HIP(hipMallocAsync((void**)&part, 512 * sizeof(float), s));
        rlgpu::launch_diff_norm(d_a, d_b, n, part, d_out, s);
        if (!d_scratch) RLGPU_CHECK_HIP(hipFreeAsync(part, s));
    });
}

extern "C" int rlgpu_permutation(int64_t n, uint64_t seed, uint64_t counter, int32_t* d_out, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(d_out && n >= 0 && n < (1ll << 31), "rlgpu_permutation: bad argument");
        if (n == 0) return;
        hipStream_t s = rlgpu::as_stream(stream);
        uint32_t *k0 = nullptr, *k1 = nullptr;
        int32_t* v0 = nullptr;
        RLGPU_CHECK_HIP(hipMallocAsync((void**)&k0, n * 4, s));
        RLGPU_CHECK_HIP(hipMallocAsync((void**)&k1, n * 4, s));
        RLGPU_CHECK_HIP(hipMallocAsync((void**)&v0, n * 4, s));
        hipLaunchKernelGGL(ppo::perm_keys, dim3(ceil_div(n, 256)), dim3(256), 0, s, k0, v0, n, seed, (uint32_t)counter);
        RLGPU_CHECK_HIP(hipGetLastError());
        size_t tmp_bytes = 0;
        RLGPU_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k0, k1, v0, d_out, (int)n, 0, 32, s));
        void* tmp = nullptr;
        RLGPU_CHECK_HIP(hipMallocAsync(&tmp, tmp_bytes + 16, s));
        RLGPU_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, k0, k1, v0, d_out, (int)n, 0, 32, s));
        RLGPU_CHECK_HIP(hipFreeAsync(tmp, s));
        RLGPU_CHECK_HIP(hipFreeAsync(k0, s));
        RLGPU_CHECK_HIP(hipFreeAsync(k1, s));
        RLGPU_CHECK_HIP(hipFreeAsync(v0, s));
    });
}

extern "C" int rlgpu_gemm(int32_t mode, int32_t a_layout, int32_t b_layout, const float* d_A, int64_t lda, const float* d_B,
                          int64_t ldb, float* d_C, int64_t ldc, const float* d_bias, int32_t I, int32_t J, int32_t K,
                          int32_t splits, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(d_A && d_B && d_C, "rlgpu_gemm: null argument");
        RLGPU_REQUIRE(mode == RLGPU_GEMM_F32X6 || mode == RLGPU_GEMM_F32 || mode == RLGPU_GEMM_F16X3,
                      "rlgpu_gemm: unknown mode");
        RLGPU_REQUIRE(I > 0 && J > 0 && K > 0 && splits >= 1, "rlgpu_gemm: bad sizes");
        RLGPU_REQUIRE((a_layout == 0 && (b_layout == 0 || b_layout == 1)) || (a_layout == 1 && b_layout == 1),
                      "rlgpu_gemm: unsupported layout pair");
        hipStream_t s = rlgpu::as_stream(stream);
        if (mode == RLGPU_GEMM_F16X3) {
            // operand scales from stand-alone max |x| passes (the training path gets them from the
            // producer kernels); B pre-split into scaled planes when the training path would be
            float* sh = nullptr;
            RLGPU_CHECK_HIP(hipMallocAsync((void**)&sh, 128 * sizeof(float), s));
            RLGPU_CHECK_HIP(hipMemsetAsync(sh, 0, 128 * sizeof(float), s));
            const int64_t ar = a_layout == 0 ? I : K, ac = a_layout == 0 ? K : I;
            hipLaunchKernelGGL(mlp::amax_rows, dim3(256), dim3(256), 0, s, d_A, ar, (int)ac, lda, sh);
            if (a_layout == 0 && splits == 1) {
                const int rows = (int)ceil_div(J, mlp::BNW) * mlp::BNW, ld = (int)ceil_div(K, mlp::XKMAX) * mlp::XKMAX;
                const int64_t plane = (int64_t)rows * ld;
                uint16_t* planes = nullptr;
                float* inv = nullptr;
                RLGPU_CHECK_HIP(hipMallocAsync((void**)&planes, 2 * plane * sizeof(uint16_t), s));
                RLGPU_CHECK_HIP(hipMallocAsync((void**)&inv, rows * sizeof(float), s));
                if (b_layout == 0)  // B [J][ldb]: W = B (out = J, in = K)
                    hipLaunchKernelGGL(mlp::split_weight_h3, dim3(rows), dim3(256), 0, s, d_B, J, K, ldb, 0, ld, planes, plane, inv);
                else  // B [K][ldb]: W^T (out = K, in = J)
                    hipLaunchKernelGGL(mlp::split_weight_h3, dim3(rows), dim3(256), 0, s, d_B, K, J, ldb, 1, ld, planes, plane, inv);
                RLGPU_CHECK_HIP(hipGetLastError());
                gemm_x6_pre(Operand{d_A, lda, sh, false}, planes, ld, plane, inv, d_C, ldc, d_bias, I, J, K, s);
                RLGPU_CHECK_HIP(hipFreeAsync(planes, s));
                RLGPU_CHECK_HIP(hipFreeAsync(inv, s));
            } else {
                const int64_t br = b_layout == 0 ? J : K, bc = b_layout == 0 ? K : J;
                hipLaunchKernelGGL(mlp::amax_rows, dim3(256), dim3(256), 0, s, d_B, br, (int)bc, ldb, sh + 64);
                gemm_f32(mode, a_layout, b_layout, Operand{d_A, lda, sh, false}, Operand{d_B, ldb, sh + 64, false}, d_C, ldc, d_bias,
                         I, J, K, splits, s);
            }
            RLGPU_CHECK_HIP(hipGetLastError());
            RLGPU_CHECK_HIP(hipFreeAsync(sh, s));
            return;
        }
        if (mode == RLGPU_GEMM_F32X6 && a_layout == 0 && splits == 1) {
            // the training path's form: B split once into padded planes, then the pre-split kernel
            const int rows = (int)ceil_div(J, mlp::BN) * mlp::BN, ld = (int)ceil_div(K, mlp::XKMAX) * mlp::XKMAX;
            const int64_t plane = (int64_t)rows * ld;
            uint16_t* planes = nullptr;
            RLGPU_CHECK_HIP(hipMallocAsync((void**)&planes, 3 * plane * sizeof(uint16_t), s));
            if (b_layout == 0)
                hipLaunchKernelGGL(mlp::split_weight, dim3(ceil_div(plane, 256)), dim3(256), 0, s, d_B, J, (int)ldb, 0, rows, ld,
                                   planes);
            else
                hipLaunchKernelGGL(mlp::split_weight, dim3(ceil_div(plane, 256)), dim3(256), 0, s, d_B, K, (int)ldb, 1, rows, ld,
                                   planes);
            RLGPU_CHECK_HIP(hipGetLastError());
            gemm_x6_pre(Operand{d_A, lda, nullptr, false}, planes, ld, plane, nullptr, d_C, ldc, d_bias, I, J, K, s);
            RLGPU_CHECK_HIP(hipFreeAsync(planes, s));
            return;
        }
        gemm_f32(mode, a_layout, b_layout, Operand{d_A, lda, nullptr, false}, Operand{d_B, ldb, nullptr, false}, d_C, ldc, d_bias, I,
                 J, K, splits, s);
    });
}

extern "C" int rlgpu_gemm_f32(int32_t a_layout, int32_t b_layout, const float* d_A, int64_t lda, const float* d_B, int64_t ldb,
                              float* d_C, int64_t ldc, const float* d_bias, int32_t I, int32_t J, int32_t K, int32_t splits,
                              void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(d_A && d_B && d_C, "rlgpu_gemm_f32: null argument");
        RLGPU_REQUIRE(I > 0 && J > 0 && K > 0 && splits >= 1, "rlgpu_gemm_f32: bad sizes");
        RLGPU_REQUIRE((a_layout == 0 && (b_layout == 0 || b_layout == 1)) || (a_layout == 1 && b_layout == 1),
                      "rlgpu_gemm_f32: unsupported layout pair");
        gemm_f32(RLGPU_GEMM_F32, a_layout, b_layout, Operand{d_A, lda, nullptr, false}, Operand{d_B, ldb, nullptr, false}, d_C, ldc,
                 d_bias, I, J, K, splits, rlgpu::as_stream(stream));
    });
}

extern "C" int rlgpu_kernel_timing(int32_t enable) {
    return rlgpu::guarded([&] {
        ktime::clear();
        ktime::g.on = enable != 0;
    });
}

extern "C" int rlgpu_kernel_timing_read(double* ms, double* work, int64_t* count, int32_t nslots) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(ms && work && count && nslots >= 0, "rlgpu_kernel_timing_read: null argument");
        for (int i = 0; i < nslots; i++) {
            ms[i] = work[i] = 0.0;
            count[i] = 0;
        }
        for (auto& r : ktime::g.recs) {
            if (r.slot >= nslots) continue;
            RLGPU_CHECK_HIP(hipEventSynchronize(r.b));
            float t = 0.f;
            RLGPU_CHECK_HIP(hipEventElapsedTime(&t, r.a, r.b));
            ms[r.slot] += t;
            work[r.slot] += r.work;
            count[r.slot]++;
        }
    });
}

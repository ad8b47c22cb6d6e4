// ppo_kernels.hpp -- policy head, PPO losses and optimizer kernels (gfx950, one wave per row).
// Semantics follow GigaLearnCPP PPOLearner.cpp (InferPolicyProbsFromModels :78-112,
// InferActionsFromModels :114-184, Learn :278-581) with the libtorch op semantics spelled out
// where they matter (clamp / min tie gradients, softmax backward, AdamW, clip_grad_norm_).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/rlgpu_detmath.h"
#include "mlp_kernels.hpp"

namespace ppo {

using mlp::bf2f;
using mlp::wave_max;
using mlp::wave_sum;

constexpr float kMinProb = 1e-11f;        // ACTION_MIN_PROB
constexpr float kDisabledLogit = -1e10f;  // ACTION_DISABLED_LOGIT
constexpr int kMaxA = 128;                // actions per row: 2 per lane
constexpr int kGuidingLossSlot = 10;      // RLGPU_M_GUIDING_LOSS (include/rlgpu_ppo.h; ppo.hip asserts the match)

// The sampler's Philox key for a draw step: the seed, with the step's high 32 bits folded in (the counter carries its
// low 32), so streams on separate step ranges -- the skill matches' 2^40 + k (rlgpu/skill.py) against the rollout's
// k -- never share uniforms; steps below 2^32 keep key = seed.
__host__ __device__ __forceinline__ uint64_t sample_key(uint64_t seed, uint64_t step) {
    return seed ^ ((step >> 32) * 0x9E3779B97F4A7C15ull);
}

__device__ __forceinline__ uint32_t philox(uint64_t key, uint32_t c0, uint32_t c1) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    uint32_t x0 = c0, x1 = c1, x2 = 0x2545F491u, x3 = 0x4F6CDD1Du;
    for (int r = 0; r < 10; r++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * x0, p1 = (uint64_t)0xCD9E8D57u * x2;
        uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y1 = (uint32_t)p1, y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1,
                 y3 = (uint32_t)p0;
        x0 = y0;
        x1 = y1;
        x2 = y2;
        x3 = y3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return x0;
}

// InferActions: logits [n, A] -> action (int32), log prob (PPOLearner.cpp:78-184).  The probs are the
// softmax of logit / temp + (-1e10) * !mask (temp = policyTemperature, wave-uniform; an IEEE fp32 division of
// the fp32-converted logit, the mask term added after it, :97-102; skipped by a uniform branch at temp = 1, where
// x / 1 = x) clamped to [1e-11, 1]; deterministic: argmax (lowest index on ties); otherwise the
// reference's CPU sampler (PPOLearner.cpp:157-178): r uniform in [0, 1), the first action whose running sum
// of the clamped probs, accumulated in column order, reaches r (r <= running), the last column when none
// does, and log(max(1e-12, p)) of the pick.  The uniform is a Philox draw of (seed, row0 + row, step) --
// global row numbers, so chunked launches draw the same uniforms as one launch -- where the reference uses
// an unseeded thread-local mt19937.
// Bit-exact against the CPU oracle (oracle/sampler_ref.c): IEEE + - * / only, exp / log by the shared
// rs_expf / rs_logf (include/rlgpu_detmath.h), no FMA contraction, max / sum by xor butterflies (= pairwise
// trees), and the running sum sequential: one lane per row walks the row's probs staged in LDS.
// One text, sample_rows_looped (below), serves every caller -- sample_actions with one row per wave, the fused
// inference kernel with 8, the one-wave kernel and the collection loop with 16 (infer_kernels.hpp) -- so all
// draw the same actions from the same logits.

// a logit as the sampler reads it: 16-bit storage (bf16 / fp16), or fp32 (useHalfPrecision = false)
template <bool F16>
__device__ __forceinline__ float logit_f(uint16_t u) { return mlp::h2f<F16>(u); }
template <bool F16>
__device__ __forceinline__ float logit_f(float x) { return x; }

// The sampler for the RG rows of one wave: lane l holds actions 2l and 2l + 1 of the row at hand.  The softmax and
// the writes loop over the rows (not unrolled: unrolled over 8 rows it was ~1,900 instructions that each call
// executes once, and instruction fetch, not arithmetic, set its time -- 17 us from the staged logits to the probs in
// the fused kernel's phase trace); the probs go to LDS in both modes and the pick's prob is read back from there;
// the running-sum walk keeps one lane per row, all RG rows at once.  rowfn(g, lg, mk, pr, row, ok) gives row g's A
// logits (global or LDS; LT: 16-bit in the format F16 names, or float), its masks, A floats of LDS scratch for its
// probs, its row and write flag: act[row], logp[row] are written where ok.  row_sel is the caller's business.
// mark(k) optional phase timestamps (the fused kernel's trace): 0 = probs in LDS, 1 = picks known.
struct NoMark {
    __device__ void operator()(int) const {}
};
template <int RG, bool F16, typename LT = uint16_t, typename RowFn, typename Mark = NoMark>
__device__ __forceinline__ void sample_rows_looped(RowFn rowfn, int A, float temp, int deterministic, uint64_t seed,
                                                   uint64_t step, int64_t row0, int lane, int32_t* act, float* logp,
                                                   Mark mark = Mark{}) {
#pragma clang fp contract(off)
    const int a0 = 2 * lane, a1 = 2 * lane + 1;
    const bool in0 = a0 < A, in1 = a1 < A;
    const int c0 = min(a0, A - 1), c1 = min(a1, A - 1);  // loads stay unconditional (no branches between them)
    int mine = A - 1;  // lane g < RG: row g's pick (deterministic: its argmax); cols - 1 when no running sum reaches r
#pragma unroll 1
    for (int g = 0; g < RG; g++) {
        const LT* lg;
        const uint8_t* mk;
        float* pr;
        int rw;
        bool ok;
        rowfn(g, lg, mk, pr, rw, ok);
        float l0 = logit_f<F16>(lg[c0]), l1 = logit_f<F16>(lg[c1]);
        const uint8_t m0 = mk[c0], m1 = mk[c1];
        if (temp != 1.f) {  // wave-uniform; x / 1 = x exactly, the branch only spares T = 1 the division's time
            l0 = l0 / temp;
            l1 = l1 / temp;
        }
        // softmax over all A columns (masked ones carry -1e10, exactly as the reference)
        float z0 = in0 ? l0 + (m0 ? 0.f : kDisabledLogit) : 0.f;
        float z1 = in1 ? l1 + (m1 ? 0.f : kDisabledLogit) : 0.f;
        const float m = mlp::wave_max_x(fmaxf(in0 ? z0 : -INFINITY, in1 ? z1 : -INFINITY));
        z0 = in0 ? rs_expf(z0 - m) : 0.f;
        z1 = in1 ? rs_expf(z1 - m) : 0.f;
        const float s = mlp::wave_sum_x(z0 + z1);
        const float p0 = in0 ? fminf(fmaxf(z0 / s, kMinProb), 1.f) : 0.f;
        const float p1 = in1 ? fminf(fmaxf(z1 / s, kMinProb), 1.f) : 0.f;
        if (deterministic) {
            float best = fmaxf(p0, p1);
            int bi = p0 >= p1 ? a0 : a1;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                const bool take = ob > best || (ob == best && oi < bi);
                best = take ? ob : best;
                bi = take ? oi : bi;
            }
            mine = lane == g ? bi : mine;
        }
        if (in0) pr[a0] = p0;
        if (in1) pr[a1] = p1;
    }
    mark(0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (!deterministic && lane < RG) {
        const LT* lg;
        const uint8_t* mk;
        float* p;
        int rw;
        bool ok;
        rowfn(lane, lg, mk, p, rw, ok);
        const float r = (float)(philox(sample_key(seed, step), (uint32_t)(row0 + rw), (uint32_t)step) >> 8) *
                        (1.f / 16777216.f);
        // the sequential running sum, 8 probs' LDS loads issued ahead of their adds (the loads do not depend
        // on the sum; one LDS round trip per 8 columns instead of per column)
        float running = 0.f;
        bool found = false;
        int j = 0;
        for (; j + 8 <= A; j += 8) {
            float q[8];
#pragma unroll
            for (int k = 0; k < 8; k++) q[k] = p[j + k];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                running += q[k];
                const bool hit = !found && r <= running;
                mine = hit ? j + k : mine;
                found = found || hit;
            }
        }
        for (; j < A; j++) {
            running += p[j];
            const bool hit = !found && r <= running;
            mine = hit ? j : mine;
            found = found || hit;
        }
    }
    mark(1);
#pragma unroll 1
    for (int g = 0; g < RG; g++) {
        const int pk = __shfl(mine, g, 64);
        const LT* lg;
        const uint8_t* mk;
        float* pr;
        int rw;
        bool ok;
        rowfn(g, lg, mk, pr, rw, ok);
        if (lane == 0 && ok) {
            act[rw] = pk;
            const float pp = pr[pk];
            if (logp) logp[rw] = rs_logf(1e-12f < pp ? pp : 1e-12f);  // log(std::max(1e-12f, p))
        }
    }
}

// the sampler alone (the layered inference path): one wave per row, 4 rows per block.
// row_sel (optional): only rows with (row_sel[row] != 0) == sel are written (mixed-policy inference).
template <bool F16, typename LT = uint16_t>
__global__ void __launch_bounds__(256) sample_actions(const LT* logits, const uint8_t* masks, int n, int A, float temp,
                                                     int deterministic, uint64_t seed, uint64_t step, int64_t row0,
                                                     int32_t* act, float* logp, const uint8_t* row_sel = nullptr,
                                                     int sel = 0) {
    __shared__ float probs[4][kMaxA];  // one row of probs per wave (the sampler's running sum)
    int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    if (row_sel && ((row_sel[row] != 0) != (sel != 0))) return;
    const auto rowfn = [&](int, const LT*& lg, const uint8_t*& mk, float*& pr, int& rw, bool& ok) {
        lg = logits + (int64_t)row * A;
        mk = masks + (int64_t)row * A;
        pr = probs[threadIdx.x >> 6];
        rw = row;
        ok = true;
    };
    sample_rows_looped<1, F16, LT>(rowfn, A, temp, deterministic, seed, step, row0, lane, act, logp);
}

// PPO policy loss + entropy and its gradient w.r.t. the fp32 training logits.
// Rows are minibatch-ordered; sample s = idx ? idx[start + r] : start + r addresses the
// batch buffers.  Metrics are reduced per block (one atomic each).
// temp (PPOLearnerConfig::policyTemperature, :411-415): the softmax runs on logit / temp + (-1e10) * !mask, an
// fp32 division, and the logit gradient is the softmax's times 1 / temp -- that scaled value is what dlogits,
// the bias partials and the H3 amax see.
// mask_entropy (maskEntropy, :426-428): each row's entropy, in the gradient and in the metric, is divided by
// log(the row's legal actions) instead of the launch constant log A.  No guard: a row with one legal action
// divides by log 1 = 0, as the reference does (the Rocket League masks never produce one).
// OPT: the instantiation that knows the two options; the launch takes it only when temp != 1 or mask_entropy is
// set.  OPT = false is the kernel without them, statement for statement: x / 1 and x * 1 are exact, but under
// this file's FMA contraction an extra factor regroups what fuses with what (the column sum's p (d - dot) + col
// becomes one FMA or a rounded product and an add), and the defaults must keep their bits.
// 16 lanes per row, 4 rows in parallel per wave (lane group q = lane / 16 owns row q of the pass),
// each lane holding the PL_K actions i, i + 16, .., i + 16 (PL_K - 1) of its row: the row's
// reductions take 4 shuffle steps and one instruction stream serves 4 rows.
constexpr int PL_K = (kMaxA + 15) / 16;  // actions per lane (A <= 128)
constexpr int PL_PASSES = 2;             // passes of 4 rows per wave
constexpr int PL_ROWS = 4 * 4 * PL_PASSES;  // rows per 256-thread block
__device__ __forceinline__ float grp_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float grp_max(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// GUIDE (PPOLearnerConfig::useGuidingPolicy, PPOLearner.cpp:458-468,551-552): 0 = none; 1 / 2 = the loss adds
// g_guide n A mean |gp - c| with gp the guide's clamped probabilities, softmax(guide logit / temp + (-1e10) * !mask)
// of the frozen policy's 16-bit logits (1: bf16, 2: fp16; rows [*, A] addressed by the sample index like the masks),
// and g_guide = guidingStrength / (n A) -- the term is added after the batch-size-ratio scaling, so bsr is not in it.
// Its gradient g_guide sign(c - gp) (sign(0) = 0, torch's abs backward) joins d[k] before the clamp gate, so the
// softmax backward, the 1 / temp factor, dlogits, the bias partials and the H3 amax all see it; the metric
// (RLGPU_M_GUIDING_LOSS) is the block's sum of |gp - c| over n A.  Masked columns hold 1e-11 on both sides: exactly 0.
// GUIDE != 0 always has the OPT = true semantics.  Every guided statement is behind if constexpr (GUIDE != 0), which
// emits nothing for GUIDE = 0: the unguided instances take guide = nullptr, g_guide = 0 and never read them.  The body
// stays one flat text: with its statements moved into __forceinline__ helpers the instances' register allocation and
// operand order moved ("Guiding policy").
template <int K, bool OPT, int GUIDE = 0>
__global__ void __launch_bounds__(256) policy_loss(const float* logits, const uint8_t* masks, const int32_t* actions,
                                                  const float* old_logp, const float* adv, const int32_t* idx, int64_t start,
                                                  int n, int A, const float* adv_stats, float bsr, float clip_range,
                                                  float ent_scale, float inv_log_a, float temp, int mask_entropy,
                                                  float* dlogits, int ldd, float* metrics, float* bias_part,
                                                  float* amax, const uint16_t* guide, float g_guide) {
    static_assert(GUIDE == 0 || OPT, "a guided instance has the options' semantics");
    __shared__ float red[16][GUIDE ? 6 : 5];
    __shared__ float colred[16][16 * K];  // per (wave, lane group) column sums of dlogits
    uint32_t vmax = 0;  // max |dlogits| (H3 operand scale, when amax is given)
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane >> 4, i = lane & 15;
    const float mean = adv_stats[0], sd = adv_stats[1];
    float m_ent = 0.f, m_kl = 0.f, m_pl = 0.f, m_ratio = 0.f, m_clip = 0.f;
    [[maybe_unused]] float m_guide = 0.f;  // this lane's sum of |gp - c| over its columns of the valid rows (GUIDE)
    float col[K];
#pragma unroll
    for (int k = 0; k < K; k++) col[k] = 0.f;
    const float g_pl = -bsr / (float)n;
    const float g_ent_a = -ent_scale * bsr * inv_log_a / (float)n;  // d loss / d H_i (H_i unnormalised)
    const float inv_temp = 1.f / temp;  // d z / d logit (OPT)
#pragma unroll
    for (int pass = 0; pass < PL_PASSES; pass++) {
        const int row = blockIdx.x * PL_ROWS + (w * PL_PASSES + pass) * 4 + grp;
        const bool valid = row < n;
        const int rowc = valid ? row : n - 1;
        const int64_t sidx = idx ? (int64_t)idx[start + rowc] : start + rowc;
        const float* lg = logits + (int64_t)rowc * A;
        const uint8_t* mk = masks + sidx * A;
        float z[K], legal_l = 0.f;
        bool in[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int a = i + 16 * k;
            in[k] = a < A;
            if constexpr (OPT) {
                const bool on = in[k] && mk[a] != 0;
                z[k] = in[k] ? lg[a] / temp + (on ? 0.f : kDisabledLogit) : -INFINITY;
                legal_l += on ? 1.f : 0.f;
            } else {
                z[k] = in[k] ? lg[a] + (mk[a] ? 0.f : kDisabledLogit) : -INFINITY;
            }
        }
        // maskEntropy: the row's entropy over log(its legal actions) (PPOLearner.cpp:426-428), one legal action
        // dividing by log 1 = 0 as the reference does; otherwise the launch constant 1 / log A
        float inv_log = inv_log_a, g_ent = g_ent_a;
        if constexpr (OPT)
            if (mask_entropy) {
                inv_log = 1.f / logf(grp_sum(legal_l));
                g_ent = -ent_scale * bsr * inv_log / (float)n;
            }
        const int a_raw = actions[sidx];
        const float old = old_logp[sidx], advr = adv[sidx];
        float m = z[0];
#pragma unroll
        for (int k = 1; k < K; k++) m = fmaxf(m, z[k]);
        m = grp_max(m);
        float e[K], esum = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++) {
            e[k] = in[k] ? expf(z[k] - m) : 0.f;
            esum += e[k];
        }
        const float sum = grp_sum(esum);
        float p[K], c[K], lgc[K], ent_l = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++) {
            p[k] = e[k] / sum;
            c[k] = fminf(fmaxf(p[k], kMinProb), 1.f);
            lgc[k] = in[k] ? logf(c[k]) : 0.f;
            ent_l += in[k] ? lgc[k] * c[k] : 0.f;
        }
        const float ent = -grp_sum(ent_l);
        // the guide's clamped probabilities of the row, kept only as sign(c - gp) and the lane's sum of |gp - c|
        [[maybe_unused]] float sg[K];
        if constexpr (GUIDE != 0) {
            const uint16_t* gl = guide + sidx * A;
            float zg[K];
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int a = i + 16 * k;
                const bool on = in[k] && mk[a] != 0;
                zg[k] = in[k] ? mlp::h2f<GUIDE == 2>(gl[a]) / temp + (on ? 0.f : kDisabledLogit) : -INFINITY;
            }
            float mg = zg[0];
#pragma unroll
            for (int k = 1; k < K; k++) mg = fmaxf(mg, zg[k]);
            mg = grp_max(mg);
            float gsum_l = 0.f;
#pragma unroll
            for (int k = 0; k < K; k++) {
                zg[k] = in[k] ? expf(zg[k] - mg) : 0.f;
                gsum_l += zg[k];
            }
            const float gsum = grp_sum(gsum_l);
            float gabs_l = 0.f;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const float gp = fminf(fmaxf(zg[k] / gsum, kMinProb), 1.f);
                sg[k] = c[k] > gp ? 1.f : (c[k] < gp ? -1.f : 0.f);
                gabs_l += in[k] ? fabsf(gp - c[k]) : 0.f;
            }
            if (valid) m_guide += gabs_l;
        }
        const int a = a_raw < 0 ? 0 : (a_raw > A - 1 ? A - 1 : a_raw);
        // the action's clamped probability: lane a % 16 of the group holds it in slot a / 16
        float mine = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++)
            if (a == i + 16 * k) mine = c[k];
        const float pa = __shfl(mine, (lane & ~15) | (a & 15), 64);
        const float lp = logf(pa);
        const float ratio = expf(lp - old);
        const float advn = (advr - mean) / (sd + 1e-8f);
        const float clipped = fminf(fmaxf(ratio, 1.f - clip_range), 1.f + clip_range);
        const float s1 = ratio * advn, s2 = clipped * advn;
        const float pl = fminf(s1, s2);
        // ---- backward (torch semantics: min() ties split the gradient, clamp passes inside [lo, hi])
        const float g_s1 = s1 < s2 ? g_pl : (s1 == s2 ? g_pl * 0.5f : 0.f);
        const float g_s2 = s2 < s1 ? g_pl : (s1 == s2 ? g_pl * 0.5f : 0.f);
        const float in_rng = (ratio >= 1.f - clip_range && ratio <= 1.f + clip_range) ? 1.f : 0.f;
        const float g_ratio = g_s1 * advn + g_s2 * advn * in_rng;
        const float g_lp = g_ratio * ratio;
        float d[K], dot_l = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++) {
            d[k] = in[k] ? -g_ent * (lgc[k] + 1.f) : 0.f;
            if (a == i + 16 * k) d[k] += g_lp / c[k];
            if constexpr (GUIDE != 0) d[k] += in[k] ? g_guide * sg[k] : 0.f;
            d[k] = (p[k] >= kMinProb && p[k] <= 1.f) ? d[k] : 0.f;
            dot_l += in[k] ? d[k] * p[k] : 0.f;
        }
        const float dot = grp_sum(dot_l);
        if (valid) {
            // dlogits rows of ldd >= A floats: the columns [A, ldd) are written as zeros, so the
            // output layer's GEMMs read 16-byte vectors across the row end
            float* dl = dlogits + (int64_t)row * ldd;
#pragma unroll
            for (int k = 0; k < K; k++) {
                if (!in[k]) {
                    if (i + 16 * k < ldd) dl[i + 16 * k] = 0.f;
                    continue;
                }
                const float gk = OPT ? p[k] * (d[k] - dot) * inv_temp : p[k] * (d[k] - dot);
                dl[i + 16 * k] = gk;
                col[k] += gk;
                const uint32_t b = mlp::abs_bits(gk);
                vmax = b > vmax ? b : vmax;
            }
            const float lr = lp - old;
            m_ent += ent * inv_log;
            m_kl += expf(lr) - 1.f - lr;
            m_pl += -pl;
            m_ratio += ratio;
            m_clip += fabsf(ratio - 1.f) > clip_range ? 1.f : 0.f;
        }
    }
    const int slot = w * 4 + grp;
#pragma unroll
    for (int k = 0; k < K; k++) colred[slot][i + 16 * k] = col[k];
    if constexpr (GUIDE != 0) m_guide = grp_sum(m_guide);
    if (i == 0) {
        if constexpr (GUIDE != 0) red[slot][5] = m_guide;
        red[slot][0] = m_ent;
        red[slot][1] = m_kl;
        red[slot][2] = m_pl;
        red[slot][3] = m_ratio;
        red[slot][4] = m_clip;
    }
    __syncthreads();
    if (bias_part)  // output-bias gradient partials of this block's rows: part[blk][A]
        for (int c2 = threadIdx.x; c2 < A; c2 += 256) {
            float t = 0.f;
            for (int q = 0; q < 16; q++) t += colred[q][c2];
            bias_part[(int64_t)blockIdx.x * A + c2] = t;
        }
    if (threadIdx.x < 5 && metrics) {
        const int mslot[5] = {0, 1, 2, 4, 5};  // entropy, KL, policy loss, ratio, clip fraction
        float v = 0.f;
        for (int q = 0; q < 16; q++) v += red[q][threadIdx.x];
        atomicAdd(&metrics[mslot[threadIdx.x]], v / (float)n);
    }
    if constexpr (GUIDE != 0)
        if (threadIdx.x == 5 && metrics) {  // mean over all n A elements
            float v = 0.f;
            for (int q = 0; q < 16; q++) v += red[q][5];
            atomicAdd(&metrics[kGuidingLossSlot], v / ((float)n * (float)A));
        }
    if (amax) mlp::h3_amax_commit(amax, vmax);
}

// f(std::integral_constant<int, K>) with K = ceil(A / 16) actions per lane (A = 90: 6 of the 8 slots PL_K allows):
// a run-time action count as the template argument of one launch expression
template <class F>
inline void with_actions_per_lane(int A, F&& f) {
    switch ((A + 15) / 16) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        default: return f(std::integral_constant<int, PL_K>{});
    }
}
// the policy-loss instance for A actions: without the policy options, with them (opt), or with a guide (guide = 1:
// bf16 guide logits, 2: fp16; implies opt)
using policy_loss_fn = decltype(&policy_loss<PL_K, false, 0>);
inline policy_loss_fn policy_loss_any(int A, bool opt, int guide) {
    policy_loss_fn fn = nullptr;
    with_actions_per_lane(A, [&](auto K) {
        fn = guide == 2   ? &policy_loss<K(), true, 2>
             : guide == 1 ? &policy_loss<K(), true, 1>
             : opt        ? &policy_loss<K(), true, 0>
                          : &policy_loss<K(), false, 0>;
    });
    return fn;
}

// Critic MSE: loss = mean((v - t)^2) * bsr ; dv = 2 (v - t) / n * bsr.
__global__ void critic_loss(const float* vals, const float* target, const int32_t* idx, int64_t start, int n, float bsr,
                            float* dvals, float* metrics) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    float contrib = 0.f;
    if (r < n) {
        int64_t s = idx ? (int64_t)idx[start + r] : start + r;
        float d = vals[r] - target[s];
        dvals[r] = 2.f * d / (float)n * bsr;
        contrib = d * d / (float)n * bsr;
    }
    contrib = wave_sum(contrib);
    if ((threadIdx.x & 63) == 0 && metrics) atomicAdd(&metrics[3], contrib);
}

// out = a + b over n floats (the shared head's output gradient: policy + critic input gradients),
// 4 per thread where the three spans are 16-byte aligned
__global__ void add2(const float* a, const float* b, float* out, int64_t n) {
    const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e >= n) return;
    const bool vec = e + 4 <= n && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
                                     reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    if (vec) {
        const float4 x = *reinterpret_cast<const float4*>(a + e), y = *reinterpret_cast<const float4*>(b + e);
        *reinterpret_cast<float4*>(out + e) = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
        return;
    }
    for (int64_t k = e; k < e + 4 && k < n; k++) out[k] = a[k] + b[k];
}

// sum of squares partials (fixed grid -> deterministic)
__global__ void __launch_bounds__(256) sumsq_partial(const float* x, int64_t n, float* part) {
    __shared__ float red[4];
    float s = 0.f;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) s += x[e] * x[e];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// clip_grad_norm_: coef = min(max_norm / (||g|| + 1e-6), 1) (torch/csrc/api/src/nn/utils/clip_grad.h)
__global__ void clip_coef(const float* part, int nblk, float max_norm, float* coef, float* norm_out) {
    if (threadIdx.x != 0) return;
    float s = 0.f;
    for (int b = 0; b < nblk; b++) s += part[b];
    float norm = sqrtf(s);
    float c = max_norm / (norm + 1e-6f);
    *coef = c < 1.f ? c : 1.f;
    if (norm_out) *norm_out = norm;
}

// AdamW step, libtorch semantics (torch/csrc/api/src/optim/adamw.cpp): grads pre-scaled by the
// clip coefficient; grads zeroed after use (the bf16 copy is refreshed afterwards).
__global__ void adamw(float* p, float* g, float* m, float* v, int64_t n, const float* coef, float decay_mul,
                      float beta1, float beta2, float one_m_b1, float one_m_b2, float step_size, float bc2_sqrt, float eps) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float gr = g[e] * *coef;
    float pv = p[e] * decay_mul;
    float mv = m[e] * beta1 + gr * one_m_b1;
    float vv = v[e] * beta2 + one_m_b2 * gr * gr;
    float denom = sqrtf(vv) / bc2_sqrt + eps;
    pv = pv + (-step_size) * (mv / denom);
    p[e] = pv;
    m[e] = mv;
    v[e] = vv;
    g[e] = 0.f;
}

// The other optimizers of MakeOptimizer (Util/Models.h), libtorch defaults with nothing but lr set; KIND is the
// RLGPU_OPT_* value.  coef: the clip coefficient, or null for an unclipped step (the transfer step).  The operations
// are rounded one by one, as adamw's are; grads zeroed after use.
//   ADAGRAD (adagrad.cpp: lr_decay 0, initial_accumulator_value 0, eps 1e-10): v = sum
//   RMSPROP (rmsprop.cpp: alpha 0.99, eps 1e-8, momentum 0, not centered):     v = square_avg
//   MAGSGD  (Util/MagSGD.h, then SGD at momentum 0): p -= lr * gr / ||gr||, with ||gr|| = *norm * coef (norm: the
//           model's unclipped gradient norm); v is not touched.  An all-zero gradient gives 0 / 0 = NaN, as there.
constexpr int kOptAdagrad = 2, kOptRmsprop = 3, kOptMagSgd = 4;
template <int KIND>
__global__ void optim_step(float* p, float* g, float* v, int64_t n, const float* coef, const float* norm, float lr) {
#pragma clang fp contract(off)
    static_assert(KIND == kOptAdagrad || KIND == kOptRmsprop || KIND == kOptMagSgd, "optim_step: unknown optimizer");
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float c = coef ? *coef : 1.f;
    const float gr = coef ? g[e] * c : g[e];
    float denom;
    if constexpr (KIND == kOptAdagrad) {
        const float sum = v[e] + gr * gr;
        v[e] = sum;
        denom = sqrtf(sum) + 1e-10f;
    } else if constexpr (KIND == kOptRmsprop) {
        constexpr float alpha = 0.99f, one_m_alpha = (float)(1.0 - 0.99);  // libtorch forms 1 - alpha in double
        const float sq = v[e] * alpha + one_m_alpha * gr * gr;
        v[e] = sq;
        denom = sqrtf(sq) + 1e-8f;
    } else {
        denom = coef ? *norm * c : *norm;
    }
    p[e] = p[e] + (-lr) * (gr / denom);
    g[e] = 0.f;
}

template <bool F16>
__global__ void to_half(const float* p, uint16_t* h, int64_t n) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) h[e] = mlp::f2h<F16>(p[e]);
}

template <bool F16>
__global__ void bf16_to_f32(const uint16_t* h, float* f, int64_t n) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) f[e] = mlp::h2f<F16>(h[e]);
}

// torch-default Linear init U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (kaiming_uniform a=sqrt(5) for
// weights, the same bound for biases); LayerNorm weight 1, bias 0.
__global__ void init_uniform(float* p, int64_t n, float bound, uint64_t seed, uint32_t stream_id) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float u = (float)(philox(seed, (uint32_t)e, stream_id) >> 8) * (1.f / 16777216.f);
    p[e] = (2.f * u - 1.f) * bound;
}
__global__ void fill(float* p, int64_t n, float v) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) p[e] = v;
}

// mean / unbiased std (fp64 accumulation): part[blk] = (sum, sumsq)
__global__ void __launch_bounds__(256) moments_partial(const float* x, int64_t n, double* part) {
    __shared__ double red[2][256];
    double s = 0, s2 = 0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        double v = x[e];
        s += v;
        s2 += v * v;
    }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = red[0][0];
        part[2 * blockIdx.x + 1] = red[1][0];
    }
}
__global__ void moments_final(const double* part, int nblk, int64_t n, float* out) {
    if (threadIdx.x != 0) return;
    double s = 0, s2 = 0;
    for (int b = 0; b < nblk; b++) {
        s += part[2 * b];
        s2 += part[2 * b + 1];
    }
    double mean = s / (double)n;
    double var = n > 1 ? (s2 - s * mean) / (double)(n - 1) : 0.0;
    out[0] = (float)mean;
    out[1] = (float)sqrt(var > 0 ? var : 0.0);
}

__global__ void perm_keys(uint32_t* keys, int32_t* vals, int64_t n, uint64_t seed, uint32_t counter) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    keys[e] = philox(seed, (uint32_t)e, counter);
    vals[e] = (int32_t)e;
}

}  // namespace ppo

// transfer_kernels.hpp -- transfer learning (Learner::StartTransferLearn, Learner.cpp:299-480; PPOLearner::TransferLearn,
// PPOLearner.cpp:583-637): the teacher's target probabilities, the distillation loss with its logit gradient, and the
// policy-only optimiser step.  Compiled in transfer.hip, a translation unit of its own: ppo.hip's kernels are not
// recompiled next to these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlp_kernels.hpp"
#include "ppo_kernels.hpp"

namespace ppo {

constexpr int kTlLossSlot = 11, kTlAccuracySlot = 12, kTlOldEntropySlot = 13;  // RLGPU_M_TL_* (ppo.hip asserts the match)

// (value, index) argmax step: the larger value, the lower index on ties
__device__ __forceinline__ void argmax_take(float& best, int& bi, float ob, int oi) {
    const bool take = ob > best || (ob == best && oi < bi);
    best = take ? ob : best;
    bi = take ? oi : bi;
}

// The teacher's side of TransferLearn (PPOLearner.cpp:592-600): oldProbs = clamp(softmax(logit / temp + (-1e10) * !mask),
// 1e-11, 1) of f32 logits [n][A_old] (InferPolicyProbsFromModels after its forward), its entropy (ComputeEntropy: the
// row's -(p log p).sum over log A_old, or with mask_entropy over log(the row's legal actions); summed over the rows as
// value / n_total into metrics[kTlOldEntropySlot]), then -- map given -- the gather along the action axis
// out[i][k] = old[i][map[i][k]] into probs [n][A], and the argmax of the gathered row (first index on ties).  Without a
// map A = A_old and the row is copied.  One wave per row, lane l holding actions 2l and 2l + 1; the clamped row goes
// through LDS for the gather.  A map entry outside [0, A_old) is the caller's error: it is clamped into the row here, so
// the read stays inside the wave's LDS row, and the value it picks is unspecified.
__global__ void __launch_bounds__(256) teacher_probs(const float* logits, const uint8_t* masks, int n, int A_old,
                                                    const int32_t* map, int A, float temp, int mask_entropy,
                                                    float inv_log_a, float inv_total, float* probs, int32_t* argmax,
                                                    float* metrics) {
#pragma clang fp contract(off)
    __shared__ float row_p[4][kMaxA];
    __shared__ float red[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + w;
    const bool valid = row < n;
    const int rowc = valid ? row : n - 1;
    const float* lg = logits + (int64_t)rowc * A_old;
    const uint8_t* mk = masks + (int64_t)rowc * A_old;
    const int a0 = 2 * lane, a1 = 2 * lane + 1;
    const bool in0 = a0 < A_old, in1 = a1 < A_old;
    const int c0 = min(a0, A_old - 1), c1 = min(a1, A_old - 1);
    const bool on0 = in0 && mk[c0] != 0, on1 = in1 && mk[c1] != 0;
    const float z0 = in0 ? lg[c0] / temp + (on0 ? 0.f : kDisabledLogit) : -INFINITY;
    const float z1 = in1 ? lg[c1] / temp + (on1 ? 0.f : kDisabledLogit) : -INFINITY;
    const float m = wave_max(fmaxf(z0, z1));
    const float e0 = in0 ? expf(z0 - m) : 0.f, e1 = in1 ? expf(z1 - m) : 0.f;
    const float s = wave_sum(e0 + e1);
    const float p0 = fminf(fmaxf(e0 / s, kMinProb), 1.f), p1 = fminf(fmaxf(e1 / s, kMinProb), 1.f);
    float ent = (in0 ? logf(p0) * p0 : 0.f) + (in1 ? logf(p1) * p1 : 0.f);
    ent = -wave_sum(ent);
    float inv_log = inv_log_a;
    if (mask_entropy) inv_log = 1.f / logf(wave_sum((on0 ? 1.f : 0.f) + (on1 ? 1.f : 0.f)));
    if (in0) row_p[w][a0] = p0;
    if (in1) row_p[w][a1] = p1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the gathered row: lane l holds columns l and l + 64
    float best = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int k = lane + 64 * q;
        if (k >= A) continue;
        int src = map ? map[(int64_t)rowc * A + k] : k;
        src = src < 0 ? 0 : (src > A_old - 1 ? A_old - 1 : src);
        const float v = row_p[w][src];
        if (valid) probs[(int64_t)row * A + k] = v;
        argmax_take(best, bi, v, k);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        argmax_take(best, bi, ob, oi);
    }
    if (lane == 0) {
        if (valid) argmax[row] = bi;
        red[w] = valid ? ent * inv_log : 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0 && metrics) atomicAdd(&metrics[kTlOldEntropySlot], (red[0] + red[1] + red[2] + red[3]) * inv_total);
}

// The student's side (PPOLearner.cpp:607-630): with c the clamped masked softmax of the fp32 training logits / temp and o
// the teacher's target probabilities (rows addressed by the sample index, like the masks),
//   loss = loss_scale * mean over all N_total A elements of t^e,   t = |o - c|   or (KL)   t = |o log(o / c)|
// and its gradient w.r.t. the logits of the chunk's n rows.  With g = loss_scale / (N_total A):
//   d loss / d c = g e t^(e-1) sign(c - o)            (L1)
//                = g e t^(e-1) sign(c - o) o / c      (KL: d |o log(o / c)| / d c = sign(log(o / c)) (-o / c))
// sign(0) = 0 (torch's abs backward), e = 1 skips the power; then the clamp gate (zero where the raw probability is
// outside [1e-11, 1]), the masked softmax's backward and the 1 / temp factor, as policy_loss's guided term.  Masked
// columns hold 1e-11 on both sides: t = 0 and sign = 0 exactly.  e >= 1 (the host refuses e < 1: 0^(e-1) = inf on
// those columns).
// policy_loss's layout: 16 lanes per row, 4 rows per wave in parallel, K actions per lane (i, i + 16, ..), PL_ROWS rows per
// 256-thread block.  Writes what backward() takes from a loss kernel: dlogits rows of ldd floats (columns [A, ldd)
// zero), the output-bias partials bias_part[blk][A], max |dlogits| into the H3 slot amax (when given); and the metric
// sums, each already divided by the whole batch's count so that the chunks of one epoch add up to the batch's value:
// the loss into kTlLossSlot, the rows with argmax c == target_argmax (first index on ties) / N_total into
// kTlAccuracySlot, and the engine's entropy (policy_loss's, mask_entropy included) / N_total into slot 0.
// Uncontracted: every sign and clamp comparison sees the rounded IEEE results the reference's operators produce.
template <int K>
__global__ void __launch_bounds__(256) transfer_loss(const float* logits, const uint8_t* masks, const float* target,
                                                    const int32_t* target_argmax, const int32_t* idx, int64_t start, int n,
                                                    int A, float temp, int mask_entropy, float inv_log_a, float g,
                                                    float exponent, int use_kl, float loss_scale, float inv_total,
                                                    float* dlogits, int ldd, float* metrics, float* bias_part, float* amax) {
#pragma clang fp contract(off)
    __shared__ float red[16][3];
    __shared__ float colred[16][16 * K];  // per (wave, lane group) column sums of dlogits
    uint32_t vmax = 0;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane >> 4, i = lane & 15;
    float m_ent = 0.f, m_loss = 0.f, m_acc = 0.f;
    float col[K];
#pragma unroll
    for (int k = 0; k < K; k++) col[k] = 0.f;
    const float inv_temp = 1.f / temp;
    const float ge = g * exponent;
    const bool pw = exponent != 1.f;
    const float em1 = exponent - 1.f;
#pragma unroll
    for (int pass = 0; pass < PL_PASSES; pass++) {
        const int row = blockIdx.x * PL_ROWS + (w * PL_PASSES + pass) * 4 + grp;
        const bool valid = row < n;
        const int rowc = valid ? row : n - 1;
        const int64_t sidx = idx ? (int64_t)idx[start + rowc] : start + rowc;
        const float* lg = logits + (int64_t)rowc * A;
        const uint8_t* mk = masks + sidx * A;
        const float* tg = target + sidx * A;
        float z[K], o[K], legal_l = 0.f;
        bool in[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int a = i + 16 * k;
            in[k] = a < A;
            const int ac = in[k] ? a : A - 1;
            const bool on = in[k] && mk[ac] != 0;
            z[k] = in[k] ? lg[ac] / temp + (on ? 0.f : kDisabledLogit) : -INFINITY;
            o[k] = tg[ac];
            legal_l += on ? 1.f : 0.f;
        }
        float inv_log = inv_log_a;
        if (mask_entropy) inv_log = 1.f / logf(grp_sum(legal_l));
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
        float p[K], c[K], ent_l = 0.f, best = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < K; k++) {
            p[k] = e[k] / sum;
            c[k] = fminf(fmaxf(p[k], kMinProb), 1.f);
            ent_l += in[k] ? logf(c[k]) * c[k] : 0.f;
            if (in[k]) argmax_take(best, bi, c[k], i + 16 * k);
        }
        const float ent = -grp_sum(ent_l);
#pragma unroll
        for (int s = 8; s > 0; s >>= 1) {
            const float ob = __shfl_xor(best, s, 64);
            const int oi = __shfl_xor(bi, s, 64);
            argmax_take(best, bi, ob, oi);
        }
        // d[k] = d loss / d c_k through the clamp gate; the lane's sum of t^e
        float d[K], dot_l = 0.f, loss_l = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++) {
            float t, dk;
            const float sg = c[k] > o[k] ? 1.f : (c[k] < o[k] ? -1.f : 0.f);
            if (use_kl) {
                t = fabsf(o[k] * logf(o[k] / c[k]));
                dk = sg * (o[k] / c[k]);
            } else {
                t = fabsf(o[k] - c[k]);
                dk = sg;
            }
            float te = t;
            if (pw) {
                const float tp = powf(t, em1);  // t = 0: 0 (e > 1)
                te = tp * t;
                dk = dk * tp;
            }
            dk = ge * dk;
            loss_l += in[k] ? te : 0.f;
            d[k] = (in[k] && p[k] >= kMinProb && p[k] <= 1.f) ? dk : 0.f;
            dot_l += in[k] ? d[k] * p[k] : 0.f;
        }
        const float dot = grp_sum(dot_l);
        loss_l = grp_sum(loss_l);
        if (valid) {
            float* dl = dlogits + (int64_t)row * ldd;
#pragma unroll
            for (int k = 0; k < K; k++) {
                if (!in[k]) {
                    if (i + 16 * k < ldd) dl[i + 16 * k] = 0.f;
                    continue;
                }
                const float gk = p[k] * (d[k] - dot) * inv_temp;
                dl[i + 16 * k] = gk;
                col[k] += gk;
                const uint32_t b = mlp::abs_bits(gk);
                vmax = b > vmax ? b : vmax;
            }
            m_ent += ent * inv_log;
            m_loss += loss_l;
            m_acc += bi == target_argmax[sidx] ? 1.f : 0.f;
        }
    }
    const int slot = w * 4 + grp;
#pragma unroll
    for (int k = 0; k < K; k++) colred[slot][i + 16 * k] = col[k];
    if (i == 0) {
        red[slot][0] = m_ent;
        red[slot][1] = m_loss;
        red[slot][2] = m_acc;
    }
    __syncthreads();
    if (bias_part)
        for (int c2 = threadIdx.x; c2 < A; c2 += 256) {
            float t = 0.f;
            for (int q = 0; q < 16; q++) t += colred[q][c2];
            bias_part[(int64_t)blockIdx.x * A + c2] = t;
        }
    if (threadIdx.x < 3 && metrics) {
        const int mslot[3] = {0, kTlLossSlot, kTlAccuracySlot};
        float v = 0.f;
        for (int q = 0; q < 16; q++) v += red[q][threadIdx.x];
        // the loss: sum t^e over the chunk times loss_scale / (N_total A)
        const float scale = threadIdx.x == 1 ? loss_scale * (inv_total / (float)A) : inv_total;
        atomicAdd(&metrics[mslot[threadIdx.x]], v * scale);
    }
    if (amax) mlp::h3_amax_commit(amax, vmax);
}

using transfer_loss_fn = decltype(&transfer_loss<PL_K>);
inline transfer_loss_fn transfer_loss_any(int A) {
    transfer_loss_fn fn = nullptr;
    with_actions_per_lane(A, [&](auto K) { fn = &transfer_loss<K()>; });
    return fn;
}

// The policy-only optimiser step (ModelSet::StepOptims after SetOptimLR(tlConfig.lr), with no clip_grad_norm_ before it,
// PPOLearner.cpp:602-603,632): adamw's arithmetic on one model's span without the clip coefficient; the gradient is
// zeroed after use.
__global__ void adam_models(float* p, float* g, float* m, float* v, int64_t n, float decay_mul, float beta1, float beta2,
                            float one_m_b1, float one_m_b2, float step_size, float bc2_sqrt, float eps) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float gr = g[e];
    float pv = p[e] * decay_mul;
    const float mv = m[e] * beta1 + gr * one_m_b1;
    const float vv = v[e] * beta2 + one_m_b2 * gr * gr;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pv = pv + (-step_size) * (mv / denom);
    p[e] = pv;
    m[e] = mv;
    v[e] = vv;
    g[e] = 0.f;
}

// sum of squares of a - b (fixed grid -> deterministic): "Policy Update Magnitude" = ||before - after||
__global__ void __launch_bounds__(256) diff_sumsq_partial(const float* a, const float* b, int64_t n, float* part) {
    __shared__ float red[4];
    float s = 0.f;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const float d = a[e] - b[e];
        s += d * d;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void diff_norm_final(const float* part, int nblk, float* out) {
    if (threadIdx.x != 0) return;
    float s = 0.f;
    for (int b = 0; b < nblk; b++) s += part[b];
    *out = sqrtf(s);
}

}  // namespace ppo

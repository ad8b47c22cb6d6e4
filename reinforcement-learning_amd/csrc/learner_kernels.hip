// learner_kernels.hip -- small device helpers of the C++ host Learner (host/learner.cpp):
// truncated-row compaction, index gathers / scatters, self-play row lists, fp64 moments, obs standardisation.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "common.hpp"
#include "learner_kernels.hpp"

namespace lk {
namespace {

using rlgpu::ceil_div;

__global__ void k_gather_f32(const float* src, const int32_t* idx, int64_t n, float* dst) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

__global__ void k_scatter_f32(const float* src, const int32_t* idx, int64_t n, float* dst) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[idx[i]] = src[i];
}

__global__ void k_gather_rows(const float* src, int C, const int32_t* idx, int64_t n, float* dst) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * C) return;
    int64_t r = e / C;
    int c = (int)(e % C);
    dst[e] = src[(int64_t)idx[r] * C + c];
}

__global__ void k_compose(const int32_t* rows, const int32_t* perm, int64_t n, int32_t* out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rows[perm[i]];
}

__global__ void k_train_rows(int T, int P, int team, int32_t* out) {
    const int half = P / 2;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)T * half) return;
    int t = (int)(i / half), q = (int)(i % half);
    out[i] = t * P + 2 * q + team;  // team of player p is p % 2 (cars 0, 2 blue; 1, 3 orange)
}

// one lane per player column: the last step t whose trajectory code is nonzero, -1 if none
__global__ void k_last_ends(const int8_t* terms, int T, int P, int32_t* out) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    int last = -1;
    for (int t = T - 1; t >= 0; --t)
        if (terms[(int64_t)t * P + p] != 0) {
            last = t;
            break;
        }
    out[p] = last;
}

__global__ void k_gather_samples(const float* src, const int64_t* idx, int n, float* dst) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

// fp64 (sum, sum of squares) partials over a grid-stride range, then a fixed-order final sum:
// deterministic run to run
constexpr int kMomBlocks = 256;
__global__ void __launch_bounds__(256) k_moments_partial(const float* x, const int32_t* idx, int64_t n, double* part) {
    __shared__ double s1[256], s2[256];
    double a = 0, b = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double v = idx ? x[idx[i]] : x[i];
        a += v;
        b += v * v;
    }
    s1[threadIdx.x] = a;
    s2[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            s1[threadIdx.x] += s1[threadIdx.x + o];
            s2[threadIdx.x] += s2[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = s1[0];
        part[2 * blockIdx.x + 1] = s2[0];
    }
}
__global__ void k_moments_final(const double* part, int nb, int64_t n, double* out) {
    if (threadIdx.x != 0) return;
    double a = 0, b = 0;
    for (int k = 0; k < nb; k++) {
        a += part[2 * k];
        b += part[2 * k + 1];
    }
    out[0] = a;
    out[1] = b;
    out[2] = (double)n;
}

__global__ void k_stack_frames(const float* cur, const float* trunc, const int8_t* codes, float* hist, int K, int P,
                               int obs, float* out, float* out_trunc) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)P * obs) return;
    const int p = (int)(e / obs), c = (int)(e % obs);
    const float x = cur[e];
    const int code = codes ? codes[p] : 1;
    const int64_t W = (int64_t)K * obs, plane = (int64_t)P * obs;
    float* o = out + p * W + c;
    if (code == 2 && out_trunc && trunc) {  // the ended trajectory's last stacked row
        float* ot = out_trunc + p * W + c;
        ot[0] = trunc[e];
        for (int k = 1; k < K; k++) ot[(int64_t)k * obs] = hist[(int64_t)(k - 1) * plane + e];
    }
    if (code != 0) {
        for (int k = 0; k < K; k++) o[(int64_t)k * obs] = x;
        for (int k = 0; k < K - 1; k++) hist[(int64_t)k * plane + e] = x;
        return;
    }
    float prev = x;
    o[0] = x;
    for (int k = 0; k < K - 1; k++) {  // read the old frame before overwriting it with the newer one
        const float h = hist[(int64_t)k * plane + e];
        o[(int64_t)(k + 1) * obs] = h;
        hist[(int64_t)k * plane + e] = prev;
        prev = h;
    }
}

// After a step hook (host plugins, Learner.cpp:780-861): one thread per (player, obs column).  The
// player's code becomes the arena's merged terminal (the hook's NORMAL-over-TRUNCATED merge of device and
// host conditions) or, where that is 0, the device's own code (the max-episode-length truncation); column 0
// also takes the step's (host-rebuilt) reward.  A code-2 row's pre-reset obs goes to the truncation rows.
__global__ void k_host_step_finish(const uint8_t* arena_terms, int8_t* codes, const float* rewards, float* rew_out,
                                   const float* obs, float* trunc_env, float* trunc_out, int P, int obs_w) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)P * obs_w) return;
    const int p = (int)(e / obs_w), c = (int)(e % obs_w);
    const int m = arena_terms[p / 4];
    const int code = m ? m : codes[p];
    if (code == 2) {
        trunc_env[e] = obs[e];
        if (trunc_out) trunc_out[e] = obs[e];
    }
    if (c == 0) {  // idempotent: a thread of the row that reads codes[p] after this write computes the same code
        codes[p] = (int8_t)code;
        if (rew_out) rew_out[p] = rewards[p];
    }
}

// one workgroup walks the players in chunks of 1024: block-wide exclusive scans of the end /
// truncation flags give each ending trajectory its record slot, truncation slot and combined offset in
// (player) order after the records of earlier steps
constexpr int kTrajThreads = 1024;
__global__ void __launch_bounds__(kTrajThreads) k_traj_step(const int8_t* codes, int row, int Tmax, const uint8_t* track,
                                                            int P, int32_t* start, int32_t* len, TrajRecs R,
                                                            int64_t* cnt, int32_t* trnew) {
    typedef hipcub::BlockScan<int, kTrajThreads> Scan;
    typedef hipcub::BlockScan<int64_t, kTrajThreads> Scan64;
    __shared__ typename Scan::TempStorage ts;
    __shared__ typename Scan64::TempStorage ts64;
    __shared__ int64_t base[3];
    __shared__ int newtr;
    const int t = threadIdx.x;
    if (t == 0) {
        base[0] = cnt[kTcRecs];
        base[1] = cnt[kTcTruncs];
        base[2] = cnt[kTcSteps];
        newtr = 0;
    }
    __syncthreads();
    const int next = (row + 1) % Tmax;
    for (int c0 = 0; c0 < P; c0 += kTrajThreads) {
        const int p = c0 + t;
        const bool on = p < P && (!track || track[p]);
        const int code = on ? codes[p] : 0;
        const int l = on ? len[p] + 1 : 0;
        const int e = code != 0, tr = code == 2;
        int eo, to, etot, ttot;
        int64_t lo, ltot;
        Scan(ts).ExclusiveSum(e, eo, etot);
        __syncthreads();
        Scan(ts).ExclusiveSum(tr, to, ttot);
        __syncthreads();
        Scan64(ts64).ExclusiveSum(e ? (int64_t)l : (int64_t)0, lo, ltot);
        __syncthreads();
        if (e) {
            const int64_t k = base[0] + eo;
            R.p[k] = p;
            R.start[k] = start[p];
            R.len[k] = l;
            R.code[k] = code;
            R.tidx[k] = tr ? (int32_t)(base[1] + to) : -1;
            R.off[k] = base[2] + lo;
            if (tr) trnew[newtr + to] = p;
            start[p] = next;
            len[p] = 0;
        } else if (on) {
            len[p] = l;
        }
        __syncthreads();
        if (t == 0) {
            base[0] += etot;
            base[1] += ttot;
            base[2] += ltot;
            newtr += ttot;
        }
        __syncthreads();
    }
    if (t == 0) {
        cnt[kTcRecs] = base[0];
        cnt[kTcTruncs] = base[1];
        cnt[kTcSteps] = base[2];
        cnt[kTcNewTruncs] = newtr;
    }
}

__global__ void k_traj_trunc_copy(const float* src, int W, const int64_t* cnt, const int32_t* trnew, float* dst) {
    const int64_t nnew = cnt[kTcNewTruncs], first = cnt[kTcTruncs] - nnew;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnew * W; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = e / W;
        const int c = (int)(e - j * W);
        dst[(first + j) * W + c] = src[(int64_t)trnew[j] * W + c];
    }
}

__global__ void k_traj_restart(const uint8_t* mask, int P, int row, int32_t* start, int32_t* len) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P && mask[p]) {
        start[p] = row;
        len[p] = 0;
    }
}

// one workgroup per record: its steps' rows, 16-byte vectors where the obs rows allow
__global__ void __launch_bounds__(256) k_traj_gather(TrajRecs R, int Tmax, int P, int W, int A, const float* obs,
                                                     const uint8_t* masks, const int32_t* acts, const float* logp,
                                                     const float* rews, const int8_t* terms, float* c_obs,
                                                     uint8_t* c_masks, int32_t* c_acts, float* c_logp, float* c_rews,
                                                     int8_t* c_terms) {
    const int64_t k = blockIdx.x;
    const int p = R.p[k], st = R.start[k], L = R.len[k];
    const int64_t off = R.off[k];
    for (int j = threadIdx.x; j < L; j += blockDim.x) {
        const int64_t src = (int64_t)((st + j) % Tmax) * P + p, dst = off + j;
        c_acts[dst] = acts[src];
        c_logp[dst] = logp[src];
        c_rews[dst] = rews[src];
        c_terms[dst] = terms[src];
    }
    for (int j = 0; j < L; j++) {
        const int64_t src = (int64_t)((st + j) % Tmax) * P + p, dst = off + j;
        const float* so = obs + src * W;
        float* d = c_obs + dst * W;
        for (int c = threadIdx.x; c < W; c += blockDim.x) d[c] = so[c];
        const uint8_t* sm = masks + src * A;
        uint8_t* dm = c_masks + dst * A;
        for (int c = threadIdx.x; c < A; c += blockDim.x) dm[c] = sm[c];
    }
}

struct IsTrunc {
    const int8_t* t;
    __device__ bool operator()(const int32_t& i) const { return t[i] == 2; }
};

// ---- obs standardisation (LearnerConfig::standardizeObs; Learner.cpp:679-693, Util/WelfordStat.h:69-243)
// Philox4x32-10 of a 64-bit counter, first output word; the same function on the host (obs_sample_row)
__host__ __device__ inline uint32_t obs_philox(uint64_t key, uint64_t ctr) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    uint32_t x0 = (uint32_t)ctr, x1 = (uint32_t)(ctr >> 32), x2 = 0, x3 = 0;
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * x0, p1 = (uint64_t)0xCD9E8D57u * x2;
        const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y1 = (uint32_t)p1, y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1,
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
__host__ __device__ inline int32_t obs_draw(uint64_t key, uint64_t ctr, int32_t rows) {
    return (int32_t)(((uint64_t)obs_philox(key, ctr) * (uint64_t)(uint32_t)rows) >> 32);
}

// the state block's parts (obs_stat_bytes): int64 count | double mean[W] | double m2[W] | float coef[2][W] | int32 active
__host__ __device__ inline double* obs_mean(void* st) { return (double*)((char*)st + 8); }
__host__ __device__ inline float* obs_coef(void* st, int W) { return (float*)((char*)st + 8 + 16 * (size_t)W); }
__host__ __device__ inline int32_t* obs_active(void* st, int W) { return (int32_t*)((char*)st + 8 + 24 * (size_t)W); }

// BatchedWelfordStat::IncrementRow over S drawn rows, then the coefficients NormalizeInPlace derives from the new
// state.  One workgroup, lane j = column j: the columns are independent, so each lane's sequential walk over the
// rows in draw order is the reference's order.  The draws are made once per chunk of kObsChunk (all lanes, into
// LDS); a lane has the next kObsAhead rows' elements in flight while it runs the dependent fp64 chain of the
// kObsAhead before them.  No contraction: every fp64 / fp32 operation rounds on its own, as the reference's
// /fp:precise build does.
constexpr int kObsLanes = 192, kObsChunk = 768, kObsAhead = 16;
__global__ void __launch_bounds__(kObsLanes) k_obs_stat_update(void* st, const float* obs, int P, int W, int S, uint64_t key,
                                                               float max_mean, float min_std) {
#pragma clang fp contract(off)
    __shared__ int32_t rows[kObsChunk];
    int64_t* pcount = (int64_t*)st;
    const int64_t c0 = *pcount;
    double* means = obs_mean(st);
    double* m2s = means + W;
    for (int j0 = 0; j0 < W; j0 += kObsLanes) {  // W <= kObsLanes in practice: one pass
        const int j = j0 + threadIdx.x;
        const bool on = j < W;
        double mean = on ? means[j] : 0.0, m2 = on ? m2s[j] : 0.0;
        for (int i0 = 0; i0 < S; i0 += kObsChunk) {
            const int n = min(kObsChunk, S - i0);
            __syncthreads();  // the chunk before is consumed
            for (int i = threadIdx.x; i < n; i += kObsLanes) rows[i] = obs_draw(key, (uint64_t)(c0 + i0 + i), P);
            __syncthreads();
            if (!on) continue;
            float x[kObsAhead], nx[kObsAhead];
#pragma unroll
            for (int u = 0; u < kObsAhead; u++) nx[u] = u < n ? obs[(int64_t)rows[u] * W + j] : 0.f;
            for (int i = 0; i < n; i += kObsAhead) {
#pragma unroll
                for (int u = 0; u < kObsAhead; u++) x[u] = nx[u];
#pragma unroll
                for (int u = 0; u < kObsAhead; u++) {  // the group after this one, loaded under this one's chain
                    const int k = i + kObsAhead + u;
                    nx[u] = k < n ? obs[(int64_t)rows[k] * W + j] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < kObsAhead; u++) {
                    if (i + u < n) {  // wave-uniform
                        const int64_t cnt = c0 + i0 + i + u;
                        const double delta = (double)x[u] - mean;
                        const double deltaN = delta / (double)(cnt + 1);
                        mean += deltaN;
                        m2 += (delta * deltaN) * (double)cnt;
                    }
                }
            }
        }
        if (!on) continue;
        means[j] = mean;
        m2s[j] = m2;
        const int64_t cn = c0 + S;
        float inv = 1.f, shift = 0.f;
        if (cn >= 2) {
            const double var = m2 / (double)(cn - 1);
            const double sd = var > 0 ? sqrt(var) : 1.0;
            const double mn = (double)min_std, mr = (double)max_mean;
            const double csd = sd > mn ? sd : mn;                  // RS_MAX
            const double lo = mean > -mr ? mean : -mr;            // RS_CLAMP = RS_MIN(RS_MAX(v, lo), hi)
            const double cmean = lo < mr ? lo : mr;
            inv = 1.0f / (float)csd;
            shift = -(float)cmean * inv;
        }
        float* coef = obs_coef(st, W);
        coef[j] = inv;
        coef[W + j] = shift;
    }
    __syncthreads();  // every lane has read the old count
    if (threadIdx.x == 0) {
        *pcount = c0 + S;
        *obs_active(st, W) = c0 + S >= 2 ? 1 : 0;
    }
}

// x <- x * inv[col] + shift[col] over the flat [n] array, col = index % W: 16-byte vectors from the first aligned
// element on, the elements before it and the last n % 4 by the first lanes of workgroup 0.  A workgroup takes
// kStdVecs * 256 consecutive vectors, every lane its kStdVecs loads before the first store.  Returns at once while the
// statistic is inactive (count < 2).
constexpr int kStdVecs = 4;
__global__ void __launch_bounds__(256) k_obs_standardize_rows(float* x, int64_t n, int W, const void* st) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float coef[];  // [2][W]
    if (*obs_active(const_cast<void*>(st), W) == 0) return;
    const float* g = obs_coef(const_cast<void*>(st), W);
    for (int k = threadIdx.x; k < 2 * W; k += blockDim.x) coef[k] = g[k];
    __syncthreads();
    const int64_t lead = (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) / 4);
    const int64_t head = lead < n ? lead : n;
    const int64_t nvec = (n - head) / 4;
    const int64_t tail0 = head + 4 * nvec;
    if (blockIdx.x == 0) {
        const int64_t edge = head + (n - tail0);  // < 8 elements
        if ((int64_t)threadIdx.x < edge) {
            const int64_t e = (int64_t)threadIdx.x < head ? (int64_t)threadIdx.x : tail0 + (threadIdx.x - head);
            const int c = (int)(e % W);
            x[e] = x[e] * coef[c] + coef[W + c];
        }
    }
    float4* xv = reinterpret_cast<float4*>(x + head);
    const int64_t v0 = (int64_t)blockIdx.x * (kStdVecs * 256) + threadIdx.x;
    float4 q[kStdVecs];
#pragma unroll
    for (int k = 0; k < kStdVecs; k++)
        if (v0 + k * 256 < nvec) q[k] = xv[v0 + k * 256];
    int c0 = (int)((head + 4 * v0) % W);
    const int hop = (4 * 256) % W;  // columns between a lane's consecutive vectors
#pragma unroll
    for (int k = 0; k < kStdVecs; k++) {
        if (v0 + k * 256 < nvec) {
            float* f = reinterpret_cast<float*>(&q[k]);
            int c = c0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                f[u] = f[u] * coef[c] + coef[W + c];
                c = c + 1 == W ? 0 : c + 1;
            }
            xv[v0 + k * 256] = q[k];
        }
        c0 = c0 + hop >= W ? c0 + hop - W : c0 + hop;
    }
}

}  // namespace

size_t obs_stat_bytes(int W) { return 8 + 24 * (size_t)W + 8; }
uint64_t obs_stat_key(uint64_t seed) {
    auto mix = [](uint64_t x) {  // splitmix64
        x += 0x9E3779B97F4A7C15ull;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        return x ^ (x >> 31);
    };
    return mix(seed ^ mix(kObsStatStream << 48));
}
int32_t obs_sample_row(uint64_t key, int64_t counter, int32_t rows) { return obs_draw(key, (uint64_t)counter, rows); }
void obs_stat_update(void* state, const float* obs, int P, int W, int S, uint64_t key, float max_mean, float min_std,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_obs_stat_update, dim3(1), dim3(kObsLanes), 0, s, state, obs, P, W, S, key, max_mean, min_std);
    RLGPU_CHECK_HIP(hipGetLastError());
}
void obs_standardize_rows(float* obs, int64_t n, int W, const void* state, hipStream_t s) {
    if (n <= 0) return;
    RLGPU_REQUIRE(n / 4 / (kStdVecs * 256) < (int64_t)1 << 31, "obs_standardize_rows: too many elements for one launch");
    const unsigned blocks = std::max(1u, ceil_div(n / 4, kStdVecs * 256));  // n / 4 >= the vectors of any alignment
    hipLaunchKernelGGL(k_obs_standardize_rows, dim3(blocks), dim3(256), 2 * (size_t)W * sizeof(float), s, obs, n, W, state);
    RLGPU_CHECK_HIP(hipGetLastError());
}

void gather_f32(const float* src, const int32_t* idx, int64_t n, float* dst, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_gather_f32, dim3(ceil_div(n, 256)), dim3(256), 0, s, src, idx, n, dst);
    RLGPU_CHECK_HIP(hipGetLastError());
}
void scatter_f32(const float* src, const int32_t* idx, int64_t n, float* dst, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_scatter_f32, dim3(ceil_div(n, 256)), dim3(256), 0, s, src, idx, n, dst);
    RLGPU_CHECK_HIP(hipGetLastError());
}
void gather_rows(const float* src, int C, const int32_t* idx, int64_t n, float* dst, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_gather_rows, dim3(ceil_div(n * C, 256)), dim3(256), 0, s, src, C, idx, n, dst);
    RLGPU_CHECK_HIP(hipGetLastError());
}
void compose(const int32_t* rows, const int32_t* perm, int64_t n, int32_t* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_compose, dim3(ceil_div(n, 256)), dim3(256), 0, s, rows, perm, n, out);
    RLGPU_CHECK_HIP(hipGetLastError());
}
void train_rows(int T, int P, int team, int32_t* out, hipStream_t s) {
    int64_t n = (int64_t)T * (P / 2);
    hipLaunchKernelGGL(k_train_rows, dim3(ceil_div(n, 256)), dim3(256), 0, s, T, P, team, out);
    RLGPU_CHECK_HIP(hipGetLastError());
}
void last_ends(const int8_t* terms, int T, int P, int32_t* out, hipStream_t s) {
    if (P <= 0) return;
    hipLaunchKernelGGL(k_last_ends, dim3(ceil_div(P, 256)), dim3(256), 0, s, terms, T, P, out);
    RLGPU_CHECK_HIP(hipGetLastError());
}
void gather_samples(const float* src, const int64_t* idx, int n, float* dst, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_gather_samples, dim3(ceil_div(n, 256)), dim3(256), 0, s, src, idx, n, dst);
    RLGPU_CHECK_HIP(hipGetLastError());
}
size_t moments_scratch_bytes() { return 2 * kMomBlocks * sizeof(double); }
void moments_f64(const float* x, const int32_t* idx, int64_t n, double* scratch, double* out3, hipStream_t s) {
    hipLaunchKernelGGL(k_moments_partial, dim3(kMomBlocks), dim3(256), 0, s, x, idx, n, scratch);
    hipLaunchKernelGGL(k_moments_final, dim3(1), dim3(64), 0, s, scratch, kMomBlocks, n, out3);
    RLGPU_CHECK_HIP(hipGetLastError());
}

void stack_frames(const float* cur, const float* trunc, const int8_t* codes, float* hist, int K, int P, int obs,
                  float* out, float* out_trunc, hipStream_t s) {
    const int64_t n = (int64_t)P * obs;
    hipLaunchKernelGGL(k_stack_frames, dim3(ceil_div(n, 256)), dim3(256), 0, s, cur, trunc, codes, hist, K, P, obs, out,
                       out_trunc);
    RLGPU_CHECK_HIP(hipGetLastError());
}

void host_step_finish(const uint8_t* arena_terms, int8_t* codes, const float* rewards, float* rew_out, const float* obs,
                      float* trunc_env, float* trunc_out, int P, int obs_w, hipStream_t s) {
    const int64_t n = (int64_t)P * obs_w;
    hipLaunchKernelGGL(k_host_step_finish, dim3(ceil_div(n, 256)), dim3(256), 0, s, arena_terms, codes, rewards, rew_out,
                       obs, trunc_env, trunc_out, P, obs_w);
    RLGPU_CHECK_HIP(hipGetLastError());
}

void traj_step(const int8_t* codes, int row, int Tmax, const uint8_t* track, int P, int32_t* start, int32_t* len,
               TrajRecs recs, int64_t* counters, int32_t* trnew, hipStream_t s) {
    hipLaunchKernelGGL(k_traj_step, dim3(1), dim3(kTrajThreads), 0, s, codes, row, Tmax, track, P, start, len, recs, counters,
                       trnew);
    RLGPU_CHECK_HIP(hipGetLastError());
}
void traj_trunc_copy(const float* src, int W, const int64_t* counters, const int32_t* trnew, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(k_traj_trunc_copy, dim3(256), dim3(256), 0, s, src, W, counters, trnew, dst);
    RLGPU_CHECK_HIP(hipGetLastError());
}
void traj_restart(const uint8_t* mask, int P, int row, int32_t* start, int32_t* len, hipStream_t s) {
    hipLaunchKernelGGL(k_traj_restart, dim3(ceil_div(P, 256)), dim3(256), 0, s, mask, P, row, start, len);
    RLGPU_CHECK_HIP(hipGetLastError());
}
void traj_gather(TrajRecs recs, int64_t K, int Tmax, int P, int W, int A, const float* obs, const uint8_t* masks,
                 const int32_t* acts, const float* logp, const float* rews, const int8_t* terms, float* c_obs,
                 uint8_t* c_masks, int32_t* c_acts, float* c_logp, float* c_rews, int8_t* c_terms, hipStream_t s) {
    if (K <= 0) return;
    hipLaunchKernelGGL(k_traj_gather, dim3((unsigned)K), dim3(256), 0, s, recs, Tmax, P, W, A, obs, masks, acts, logp, rews,
                       terms, c_obs, c_masks, c_acts, c_logp, c_rews, c_terms);
    RLGPU_CHECK_HIP(hipGetLastError());
}

size_t select_trunc_scratch_bytes(int64_t n) {
    size_t bytes = 0;
    hipcub::CountingInputIterator<int32_t> it(0);
    RLGPU_CHECK_HIP(hipcub::DeviceSelect::If(nullptr, bytes, it, (int32_t*)nullptr, (int32_t*)nullptr, (int)n,
                                             IsTrunc{nullptr}, (hipStream_t)0));
    return bytes;
}
void select_trunc(const int8_t* terms, int64_t n, void* scratch, size_t scratch_bytes, int32_t* rows, int32_t* count,
                  hipStream_t s) {
    hipcub::CountingInputIterator<int32_t> it(0);
    RLGPU_CHECK_HIP(hipcub::DeviceSelect::If(scratch, scratch_bytes, it, rows, count, (int)n, IsTrunc{terms}, s));
}

}  // namespace lk

// policy_loss_body.inc -- the statements of ppo::policy_loss and ppo::policy_loss_guided (ppo_kernels.hpp), included into
// both kernels' bodies: one text, two kernels, and no call in between -- as an inlined function the shared body moved
// the unguided instances' register allocation and operand order.  The including kernel provides K, OPT, GUIDE (0 = no
// guide, 1 = bf16 guide logits, 2 = fp16), the arguments of policy_loss and, when GUIDE != 0, guide and g_guide; every
// guided statement is behind if constexpr (GUIDE != 0), which emits nothing for GUIDE = 0.
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

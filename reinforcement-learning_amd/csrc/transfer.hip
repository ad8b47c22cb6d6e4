// transfer.hip -- the launches of transfer_kernels.hpp (declared in common.hpp, called by ppo.hip's
// rlgpu_ppo_teacher_probs / rlgpu_ppo_transfer_chunk / rlgpu_ppo_transfer_step): a translation unit of its own, so the
// transfer-learning kernels are built beside ppo.hip's, not among them.
//
// The kernel headers define non-template kernels too, so this unit takes its copy of them in an unnamed namespace
// (internal linkage; what it does not launch is not emitted), as infer_act.hip does.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/rlgpu_detmath.h"
#include "../../include/rlgpu_ppo.h"
#include "common.hpp"

namespace {
#include "transfer_kernels.hpp"
}

namespace rlgpu {

void launch_teacher_probs(const TeacherProbsArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(ppo::teacher_probs, dim3(ceil_div(a.n, 4)), dim3(256), 0, s, a.logits, a.masks, a.n, a.A_old, a.map, a.A,
                       a.temp, a.mask_entropy, 1.f / std::log((float)a.A_old), 1.f / (float)a.total_rows, a.probs, a.argmax,
                       a.metrics);
    RLGPU_CHECK_HIP(hipGetLastError());
}

int transfer_loss_blocks(int n) { return (int)ceil_div(n, ppo::PL_ROWS); }

void launch_transfer_loss(const TransferLossArgs& a, hipStream_t s) {
    const float g = a.loss_scale / ((float)a.total_rows * (float)a.A);
    hipLaunchKernelGGL(ppo::transfer_loss_any(a.A), dim3(transfer_loss_blocks(a.n)), dim3(256), 0, s, a.logits, a.masks, a.target,
                       a.target_argmax, a.idx, a.start, a.n, a.A, a.temp, a.mask_entropy, 1.f / std::log((float)a.A), g,
                       a.exponent, a.use_kl, a.loss_scale, 1.f / (float)a.total_rows, a.dlogits, a.ldd, a.metrics, a.bias_part,
                       a.amax);
    RLGPU_CHECK_HIP(hipGetLastError());
}

void launch_adam_models(float* p, float* g, float* m, float* v, int64_t n, float decay_mul, float beta1, float beta2,
                        float step_size, float bc2_sqrt, float eps, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ppo::adam_models, dim3(ceil_div(n, 256)), dim3(256), 0, s, p, g, m, v, n, decay_mul, beta1, beta2,
                       1.f - beta1, 1.f - beta2, step_size, bc2_sqrt, eps);
    RLGPU_CHECK_HIP(hipGetLastError());
}

void launch_optim_models(int kind, float* p, float* g, float* v, int64_t n, float lr, float* part512, float* norm,
                         hipStream_t s) {
    if (n <= 0) return;
    const dim3 grid(ceil_div(n, 256)), block(256);
    const float* no_coef = nullptr;
    if (kind == RLGPU_OPT_ADAGRAD) {
        hipLaunchKernelGGL(ppo::optim_step<ppo::kOptAdagrad>, grid, block, 0, s, p, g, v, n, no_coef, no_coef, lr);
    } else if (kind == RLGPU_OPT_RMSPROP) {
        hipLaunchKernelGGL(ppo::optim_step<ppo::kOptRmsprop>, grid, block, 0, s, p, g, v, n, no_coef, no_coef, lr);
    } else {
        RLGPU_REQUIRE(kind == RLGPU_OPT_MAGSGD, "launch_optim_models: unknown optimizer");
        const int nb = 512;  // MagSGD::step's grad.norm() over the model: the clip's reduction, its result the norm alone
        hipLaunchKernelGGL(ppo::sumsq_partial, dim3(nb), dim3(256), 0, s, (const float*)g, n, part512);
        hipLaunchKernelGGL(ppo::diff_norm_final, dim3(1), dim3(64), 0, s, (const float*)part512, nb, norm);
        hipLaunchKernelGGL(ppo::optim_step<ppo::kOptMagSgd>, grid, block, 0, s, p, g, v, n, no_coef, (const float*)norm, lr);
    }
    RLGPU_CHECK_HIP(hipGetLastError());
}

void launch_diff_norm(const float* a, const float* b, int64_t n, float* part512, float* out, hipStream_t s) {
    const int nb = 512;
    hipLaunchKernelGGL(ppo::diff_sumsq_partial, dim3(nb), dim3(256), 0, s, a, b, n, part512);
    hipLaunchKernelGGL(ppo::diff_norm_final, dim3(1), dim3(64), 0, s, part512, nb, out);
    RLGPU_CHECK_HIP(hipGetLastError());
}

}  // namespace rlgpu

// env_collect_k0.hip -- the collection loop kernel (env_step.hpp: every env workgroup loops over the rollout's T
// steps, the policy forward of its 16 players inside it) for RLGPU_ARITH_MSVC_X64, with its constant uploads and its
// launch.  A unit of its own: the per-step kernel of env_k0.hip and the device functions it calls keep their code
// (functions shared by two kernels of one unit are compiled for both).
#define RLGPU_ENV_ARITH 0
#define RLGPU_ENV_COLLECT_KERNEL env_collect_a0
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cstdlib>

#include "../../include/rlgpu_detmath.h"
#include "common.hpp"
// The policy forward is compiled as in ppo.hip, with FMA contraction on (this unit's command line turns it off for
// the physics), so that it rounds as the fused inference kernel does.  An unnamed namespace for infer_act.hip's reason.
#pragma clang fp contract(fast)
namespace {
#include "infer_kernels.hpp"
}
#pragma clang fp contract(off)
#include "env_step.hpp"

namespace rl {
void env_collect_k0_upload(const EnvConst& k, const RsqrtLut* lut) {
    RLGPU_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(C), &k, sizeof k));
    if (lut) RLGPU_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(kRsqrtLut), lut, sizeof *lut));
}
void env_collect_k0_launch(const CollectArgs& c, bool f16, int blocks, hipStream_t s) {
    // c.split selects the profiled instantiation (env_step.hpp SplitClock)
    if (c.split) {
        if (f16) hipLaunchKernelGGL((env_collect_a0<true, true>), dim3(blocks), dim3(kWG), 0, s, c);
        else hipLaunchKernelGGL((env_collect_a0<false, true>), dim3(blocks), dim3(kWG), 0, s, c);
    } else {
        if (f16) hipLaunchKernelGGL((env_collect_a0<true, false>), dim3(blocks), dim3(kWG), 0, s, c);
        else hipLaunchKernelGGL((env_collect_a0<false, false>), dim3(blocks), dim3(kWG), 0, s, c);
    }
    RLGPU_CHECK_HIP(hipGetLastError());
}
}  // namespace rl

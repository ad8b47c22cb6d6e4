// infer_wave.hip -- the stand-alone instances of the one-wave inference forward (infer::mlp_infer_wave: 16 rows per
// 64-thread workgroup, infer_kernels.hpp) and their launch.  Compiled apart from ppo.hip for infer_act.hip's reason:
// the default mlp_infer instances there stay the only kernels of that header in their translation unit and keep
// their code.  The launch arguments cross the unit boundary as bytes, as in infer_act.hip.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cstdlib>
#include <cstring>

#include "../../include/rlgpu_detmath.h"
#include "common.hpp"

namespace {
#include "infer_kernels.hpp"
}

namespace rlgpu {

// One launch of mlp_infer_wave<f16> (LeakyReLU / ReLU) over `blocks` workgroups with the infer::InferArgs at `args`.
void launch_mlp_infer_wave(bool f16, unsigned blocks, hipStream_t s, const void* args, size_t bytes) {
    infer::InferArgs a;
    if (bytes != sizeof(a)) throw Error(RLGPU_ERR_STATE, "launch_mlp_infer_wave: InferArgs size mismatch");
    std::memcpy(&a, args, sizeof(a));
    if (f16) hipLaunchKernelGGL((infer::mlp_infer_wave<true, mlp::ACT_LEAKY>), dim3(blocks), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((infer::mlp_infer_wave<false, mlp::ACT_LEAKY>), dim3(blocks), dim3(64), 0, s, a);
}

}  // namespace rlgpu

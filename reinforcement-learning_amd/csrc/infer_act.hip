// infer_act.hip -- the SIGMOID / TANH instances of the fused inference kernel (infer::mlp_infer<F16, ACT>) and their
// launch.  They are compiled apart from ppo.hip so that the LeakyReLU instances there are the only ones in their
// translation unit: with further instances beside them the optimizer orders the default kernel's address
// arithmetic differently (177 -> 179 VGPRs, same occupancy), and the default path is to keep its code.
//
// The kernel headers define non-template kernels too, so this unit takes its copy of them in an unnamed namespace
// (internal linkage; what it does not launch is not emitted).  The launch arguments cross the unit boundary as
// bytes: both units build infer::InferArgs from the same header, and the size is checked.
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

// One launch of mlp_infer<f16, act> (act: mlp::ACT_SIGMOID or mlp::ACT_TANH) over `blocks` workgroups with the
// infer::InferArgs at `args`.
void launch_mlp_infer_act(int act, bool f16, unsigned blocks, hipStream_t s, const void* args, size_t bytes) {
    infer::InferArgs a;
    if (bytes != sizeof(a)) throw Error(RLGPU_ERR_STATE, "launch_mlp_infer_act: InferArgs size mismatch");
    std::memcpy(&a, args, sizeof(a));
    const auto launch = [&](auto k16, auto k) { hipLaunchKernelGGL(f16 ? k16 : k, dim3(blocks), dim3(infer::IT), 0, s, a); };
    if (act == mlp::ACT_SIGMOID) launch(infer::mlp_infer<true, mlp::ACT_SIGMOID>, infer::mlp_infer<false, mlp::ACT_SIGMOID>);
    else if (act == mlp::ACT_TANH) launch(infer::mlp_infer<true, mlp::ACT_TANH>, infer::mlp_infer<false, mlp::ACT_TANH>);
    else throw Error(RLGPU_ERR_INVALID_ARG, "launch_mlp_infer_act: activation kind " + std::to_string(act));
}

}  // namespace rlgpu

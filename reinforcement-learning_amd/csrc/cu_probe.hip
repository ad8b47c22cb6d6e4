// cu_probe.hip -- rlgpu_debug_cu_probe (include/rlgpu_core.h): where the workgroups of a launch land.
//
// One wave per workgroup holding the whole register file of its SIMD (512 registers per lane, as the env kernel
// does), so a launch of one workgroup per SIMD that holds its waves long enough for all of them to be resident puts
// exactly one on every SIMD the stream may use.  Each workgroup reports the XCD, shader engine and CU it ran on.
#include "common.hpp"

namespace {

constexpr int kHwRegHwId = 4, kHwRegXccId = 20;  // s_getreg_b32 register ids (gfx9 / gfx940+)
constexpr int getreg(int id, int offset, int size) { return id | (offset << 6) | ((size - 1) << 11); }
constexpr unsigned kMaxHoldUs = 2000;

__global__ void __launch_bounds__(64) cu_probe_kernel(uint32_t* out, int n, unsigned hold_ticks) {
    // the last architectural and the last accumulation register: 256 + 256 per lane
    asm volatile("" ::: "v255", "a255");
    const uint32_t hw = __builtin_amdgcn_s_getreg(getreg(kHwRegHwId, 0, 32));
    const uint32_t xcc = __builtin_amdgcn_s_getreg(getreg(kHwRegXccId, 0, 4));
    const unsigned long long t0 = wall_clock64();  // 100 MHz
    // bounded both by the clock and by a trip count
    for (int i = 0; i < (1 << 20) && wall_clock64() - t0 < hold_ticks; i++) __builtin_amdgcn_s_sleep(8);
    const int w = (int)blockIdx.x;
    if (w < n && threadIdx.x < 4) {
        const uint32_t v = threadIdx.x == 0 ? xcc : threadIdx.x == 1 ? (hw >> 13) & 7u : threadIdx.x == 2 ? (hw >> 8) & 15u : hw;
        out[(size_t)w * 4 + threadIdx.x] = v;  // one lane per word: vector stores
    }
}

}  // namespace

extern "C" int rlgpu_debug_cu_probe(void* stream, uint32_t* d_out, int32_t n_workgroups, int32_t hold_us) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(d_out && n_workgroups > 0 && n_workgroups <= 65536, "rlgpu_debug_cu_probe: 1 .. 65536 workgroups");
        RLGPU_REQUIRE(hold_us >= 0 && (unsigned)hold_us <= kMaxHoldUs, "rlgpu_debug_cu_probe: hold of 0 .. 2000 us");
        hipLaunchKernelGGL(cu_probe_kernel, dim3((unsigned)n_workgroups), dim3(64), 0, rlgpu::as_stream(stream), d_out,
                           (int)n_workgroups, (unsigned)hold_us * 100u);
        RLGPU_CHECK_HIP(hipGetLastError());
    });
}

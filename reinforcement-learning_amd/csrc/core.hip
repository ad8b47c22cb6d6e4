// core.hip -- error channel and version of the rlgpu C ABI (include/rlgpu_core.h).
#include "common.hpp"

#include <atomic>

namespace rlgpu {
static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }

static std::atomic<int64_t> g_live_allocations{0};
void* dev_alloc(size_t bytes) {
    void* p = nullptr;
    RLGPU_CHECK_HIP(hipMalloc(&p, bytes));
    if (p) g_live_allocations++;  // hipMalloc(0) hands out null, which dev_free does not count either
    return p;
}
void dev_free(void* p) {
    if (!p) return;
    (void)hipFree(p);
    g_live_allocations--;
}
}  // namespace rlgpu

extern "C" int64_t rlgpu_live_device_allocations(void) { return rlgpu::g_live_allocations.load(); }

extern "C" const char* rlgpu_last_error(void) { return rlgpu::g_last_error.c_str(); }

extern "C" int rlgpu_abi_version(void) { return 101; }

extern "C" int rlgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

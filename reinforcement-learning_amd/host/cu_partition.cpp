// cu_partition.cpp -- the CU partition of host/cu_partition.hpp and its C entries (include/rlgpu_core.h).
//
// How the bits of a HIP CU mask map to the 8 x 32 CUs of an MI355X is not documented; two mappings are plausible.
// Write bit k of the mask as b7 .. b0:
//   interleaved   XCD = k % 8  = (b2 b1 b0), CU within the XCD = k / 8  = (b7 .. b3)
//   blocked       XCD = k / 32 = (b7 b6 b5), CU within the XCD = k % 32 = (b4 .. b0)
// A queue whose mask leaves an XCD without CUs must never exist (workgroups are dealt over the XCDs in hardware), so
// every group takes the same number of CUs in every XCD under BOTH mappings.  The group of bit k is the low
// log2(groups) bits of
//   g0 = b3, g1 = b4, g2 = b2 ^ b5, g3 = b1 ^ b6.
// Fix an XCD.  Interleaved fixes b0 b1 b2 and leaves b3 .. b7 free: b3, b4 are free themselves, and b5, b6 are free
// inside g2, g3, so (g0 .. g3) takes each of its 16 values equally often (twice, by the free b7).  Blocked fixes b5 b6 b7
// and leaves b0 .. b4 free: b3, b4 again, and b2, b1 inside g2, g3 (b0 spare).  Hence 32 / groups CUs per XCD and group for
// groups = 2, 4, 8, 16 under both, the groups pairwise disjoint and covering every bit because each bit has one group.
// (For 4 groups this is (k >> 3) % 4.)  Other group counts, and devices of another CU count, are refused.
#include "cu_partition.hpp"

#include <cstring>

#include "../../include/rlgpu_core.h"
#include "../csrc/common.hpp"

namespace rlgpu {

int cu_partition_group(int k, int groups) {
    if (groups != 2 && groups != 4 && groups != 8 && groups != 16) return -1;
    if (k < 0 || k >= kPartitionCUs) return -1;
    const int b = k;
    const int g = ((b >> 3) & 1) | (((b >> 4) & 1) << 1) | ((((b >> 2) ^ (b >> 5)) & 1) << 2) |
                  ((((b >> 1) ^ (b >> 6)) & 1) << 3);
    return g & (groups - 1);
}

bool cu_partition_masks(int cu_count, int groups, std::vector<uint32_t>& masks) {
    if (cu_count != kPartitionCUs || cu_partition_group(0, groups) < 0) return false;
    std::vector<uint32_t> m((size_t)groups * kPartitionWords, 0u);
    for (int k = 0; k < kPartitionCUs; k++)
        m[(size_t)cu_partition_group(k, groups) * kPartitionWords + k / 32] |= 1u << (k % 32);
    // the balance the construction promises, checked under both mappings before any mask is handed out
    const int want = kPartitionCUs / kPartitionXCDs / groups;
    for (int g = 0; g < groups; g++) {
        int inter[kPartitionXCDs] = {}, block[kPartitionXCDs] = {};
        for (int k = 0; k < kPartitionCUs; k++)
            if (m[(size_t)g * kPartitionWords + k / 32] >> (k % 32) & 1u) {
                inter[k % kPartitionXCDs]++;
                block[k / (kPartitionCUs / kPartitionXCDs)]++;
            }
        for (int x = 0; x < kPartitionXCDs; x++)
            if (inter[x] != want || block[x] != want) return false;
    }
    masks.swap(m);
    return true;
}

hipError_t cu_partition_stream(int groups, int group, hipStream_t* out) {
    *out = nullptr;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return e;
    std::vector<uint32_t> masks;
    if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0 || group < 0 || group >= groups ||
        !cu_partition_masks(p.multiProcessorCount, groups, masks))
        return hipErrorNotSupported;
    return hipExtStreamCreateWithCUMask(out, kPartitionWords, masks.data() + (size_t)group * kPartitionWords);
}

}  // namespace rlgpu

extern "C" int rlgpu_cu_partition(int32_t cu_count, int32_t groups, uint32_t* masks, int32_t words) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(masks && words == rlgpu::kPartitionWords, "rlgpu_cu_partition: masks of 8 words each");
        std::vector<uint32_t> m;
        if (!rlgpu::cu_partition_masks(cu_count, groups, m))
            throw rlgpu::Error(RLGPU_ERR_UNSUPPORTED, "rlgpu_cu_partition: no balanced partition of " +
                                                          std::to_string(cu_count) + " CUs into " +
                                                          std::to_string(groups) + " groups");
        std::memcpy(masks, m.data(), m.size() * sizeof(uint32_t));
    });
}

extern "C" int rlgpu_debug_cu_stream_create(int32_t groups, int32_t group, void** stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(stream, "rlgpu_debug_cu_stream_create: stream is null");
        hipStream_t s = nullptr;
        const hipError_t e = rlgpu::cu_partition_stream(groups, group, &s);
        if (e == hipErrorNotSupported)
            throw rlgpu::Error(RLGPU_ERR_UNSUPPORTED, "rlgpu_debug_cu_stream_create: no balanced partition of this device into " +
                                                          std::to_string(groups) + " groups");
        RLGPU_CHECK_HIP(e);
        *stream = s;
    });
}

extern "C" int rlgpu_debug_cu_stream_mask(void* stream, uint32_t* mask, int32_t words) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(mask && words > 0, "rlgpu_debug_cu_stream_mask: mask of at least one word");
        RLGPU_CHECK_HIP(hipExtStreamGetCUMask(rlgpu::as_stream(stream), (uint32_t)words, mask));
    });
}

extern "C" int rlgpu_debug_cu_stream_destroy(void* stream) {
    return rlgpu::guarded([&] {
        if (stream) RLGPU_CHECK_HIP(hipStreamDestroy(rlgpu::as_stream(stream)));
    });
}

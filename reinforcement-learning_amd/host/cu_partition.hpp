// cu_partition.hpp -- disjoint compute-unit partitions of one MI355X for streams that must not share CUs
// (the rollout collection's arena groups, host/learner.cpp; include/rlgpu_core.h exports them for tests / tools).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

namespace rlgpu {

// The device this build partitions: 8 XCDs of 32 CUs (MI355X).  A CU mask has one bit per CU.
constexpr int kPartitionCUs = 256;
constexpr int kPartitionXCDs = 8;
constexpr int kPartitionWords = kPartitionCUs / 32;

// Group (0 .. groups - 1) of mask bit k, or -1 when `groups` cannot be shown balanced (cu_partition.cpp).
int cu_partition_group(int k, int groups);

// groups masks of kPartitionWords words each, pairwise disjoint, covering every CU, each with
// kPartitionCUs / kPartitionXCDs / groups CUs in every XCD under either bit-to-CU mapping (cu_partition.cpp).
// False (masks untouched) for a cu_count other than kPartitionCUs or a `groups` outside {2, 4, 8, 16}.
bool cu_partition_masks(int cu_count, int groups, std::vector<uint32_t>& masks);

// A stream of the current device restricted to partition `group` of `groups`.  hipExtStreamCreateWithCUMask takes
// no flags: the stream is a default (blocking) stream, i.e. it synchronises with the legacy null stream, and it
// owns a hardware queue of its own.  Returns hipErrorNotSupported where the device is not the one partitioned
// here or `groups` is refused; no stream is created then.
hipError_t cu_partition_stream(int groups, int group, hipStream_t* out);

}  // namespace rlgpu

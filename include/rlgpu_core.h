/*
 * rlgpu_core.h -- error convention and version of the rlgpu C ABI.
 *
 * The reference reports errors by logging and throwing std::runtime_error
 * (RG_ERR_CLOSE, GigaLearnCPP/RLGymCPP/src/RLGymCPP/Framework.h:16-21;
 * RS_ERR_CLOSE, GigaLearnCPP/RLGymCPP/RocketSim/src/Framework.h:67-72).
 * Across this C boundary every entry point instead returns an int status and
 * keeps a thread-local message; the C++ facade (rlgpu.hpp) turns a non-zero
 * status back into std::runtime_error so the Learner's try/catch behaves the
 * same (GigaLearnCPP/src/public/GigaLearnCPP/Learner.cpp:466-474,
 * PPO/PPOLearner.cpp:504-518,571-580).
 */
#ifndef RLGPU_CORE_H
#define RLGPU_CORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum rlgpu_status {
    RLGPU_OK = 0,
    RLGPU_ERR_INVALID_ARG = -1,   /* bad size / null pointer / out-of-range config */
    RLGPU_ERR_HIP = -2,           /* a HIP runtime call failed */
    RLGPU_ERR_OOM = -3,           /* device allocation failed */
    RLGPU_ERR_STATE = -4,         /* call not valid in the handle's current state */
    RLGPU_ERR_UNSUPPORTED = -5    /* plugin / reward / condition type not built */
};

/* Message of the last failing call on this thread ("" if none). */
const char* rlgpu_last_error(void);

/* ABI version: major*10000 + minor*100 + patch. */
int rlgpu_abi_version(void);

/* Number of visible HIP devices (0 if no GPU); never fails. */
int rlgpu_device_count(void);

/* Diagnostics: the persistent device allocations this process holds through the library right now -- the buffers
 * of its env sets, PPO handles and host Learners (not the stream-ordered temporaries of a single call, nor the
 * per-device scratch created once and kept).  Exact per process, which free device memory on a shared card is
 * not: a handle that is created and destroyed, or whose creation fails, leaves the count where it was. */
int64_t rlgpu_live_device_allocations(void);

/* Compute-unit partitions (host/cu_partition.cpp): `groups` CU masks of `words` = 8 uint32 each (bit k of a mask
 * is bit k % 32 of word k / 32), pairwise disjoint, covering every CU, each with the same number of CUs in every
 * XCD under either plausible bit-to-CU mapping.  Host only.  RLGPU_ERR_UNSUPPORTED for a cu_count other than 256
 * (8 XCDs of 32 CUs, MI355X) or a group count outside 2, 4, 8, 16: no balance can be shown for those. */
int rlgpu_cu_partition(int32_t cu_count, int32_t groups, uint32_t* masks, int32_t words);

/* Diagnostics: a stream of the current device restricted to partition `group` of `groups` (what the Learner's
 * collection groups run on), the mask the runtime reports for a stream (hipExtStreamGetCUMask), and the
 * stream's end. */
int rlgpu_debug_cu_stream_create(int32_t groups, int32_t group, void** stream);
int rlgpu_debug_cu_stream_mask(void* stream, uint32_t* mask, int32_t words);
int rlgpu_debug_cu_stream_destroy(void* stream);
/* Diagnostics: one launch of n_workgroups single-wave workgroups on `stream`, each holding all 512 registers per
 * lane of its SIMD (as an env workgroup does) for hold_us microseconds (0 .. 2000), then writing
 * d_out[4 w .. 4 w + 3] = its XCD id, shader-engine id, CU id within the engine, and the raw HW_ID register. */
int rlgpu_debug_cu_probe(void* stream, uint32_t* d_out, int32_t n_workgroups, int32_t hold_us);

#ifdef __cplusplus
}
#endif
#endif

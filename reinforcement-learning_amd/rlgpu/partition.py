"""Compute-unit partitions of one MI355X (host/cu_partition.cpp over include/rlgpu_core.h): the masks, streams
restricted to one partition (what the C++ Learner's collection groups run on), and the placement probe."""
import ctypes

import numpy as np

from . import _lib

WORDS = 8  # uint32 words of a CU mask (256 CUs)


def masks(cu_count, groups):
    """[groups, 8] uint32 CU masks, pairwise disjoint and balanced over the XCDs; raises RLGPUError when no
    balance can be shown for (cu_count, groups).  Host only."""
    out = np.zeros((max(groups, 1), WORDS), np.uint32)
    L = _lib.lib()
    L.rlgpu_cu_partition.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]
    _lib.check(L.rlgpu_cu_partition(cu_count, groups, out.ctypes.data, WORDS), "rlgpu_cu_partition")
    return out


def mask_bits(mask):
    """The set bit indices of one mask (uint32 words, bit k = bit k % 32 of word k // 32)."""
    return [32 * w + b for w, x in enumerate(np.asarray(mask, np.uint32).tolist()) for b in range(32) if x >> b & 1]


class PartitionStream:
    """A HIP stream on partition `group` of `groups` of the current device, usable as a torch stream (.stream)."""

    def __init__(self, groups, group):
        import torch
        L = _lib.lib()
        L.rlgpu_debug_cu_stream_create.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
        h = ctypes.c_void_p()
        _lib.check(L.rlgpu_debug_cu_stream_create(groups, group, ctypes.byref(h)), "rlgpu_debug_cu_stream_create")
        self._h = h
        self.stream = torch.cuda.ExternalStream(h.value)

    def mask(self):
        """The CU mask the runtime reports for the stream (hipExtStreamGetCUMask), [8] uint32."""
        out = np.zeros(WORDS, np.uint32)
        L = _lib.lib()
        L.rlgpu_debug_cu_stream_mask.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
        _lib.check(L.rlgpu_debug_cu_stream_mask(self._h, out.ctypes.data, WORDS), "rlgpu_debug_cu_stream_mask")
        return out

    def close(self):
        if self._h:
            L = _lib.lib()
            L.rlgpu_debug_cu_stream_destroy.argtypes = [ctypes.c_void_p]
            self.stream.synchronize()
            _lib.check(L.rlgpu_debug_cu_stream_destroy(self._h), "rlgpu_debug_cu_stream_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def probe(stream, n_workgroups, hold_us=200):
    """One probe launch of n_workgroups whole-SIMD workgroups on a torch stream (None: the current one); returns
    int64 [n, 4]: XCD id, shader engine, CU within the engine, raw HW_ID -- after synchronising the stream."""
    import torch
    out = torch.full((n_workgroups, 4), -1, dtype=torch.int32, device="cuda")  # unwritten rows read 0xFFFFFFFF
    torch.cuda.current_stream().synchronize()
    L = _lib.lib()
    L.rlgpu_debug_cu_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    _lib.check(L.rlgpu_debug_cu_probe(_lib.stream_ptr(stream), _lib.ptr(out), n_workgroups, hold_us), "rlgpu_debug_cu_probe")
    (stream if stream is not None else torch.cuda.current_stream()).synchronize()
    return out.cpu().numpy().view(np.uint32).astype(np.int64)

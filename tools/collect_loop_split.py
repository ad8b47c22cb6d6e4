"""Where a workgroup of the collection loop (env_collect_a0, csrc/env_step.hpp) spends its steps: the profiled
instantiation's per-workgroup sums (rlgpu_envset_set_collect_split) of one rollout of the bench workload.

A C++ Learner with bench.py's configuration runs `warm` whole iterations on the default instantiation; the next
iteration's collection runs the profiled one.  Lane 0 of every workgroup adds the 100 MHz wall-clock ticks of each
part of each step to its slots; printed per part: mean / p50 / p99 / max over the workgroups of the T-step sum in ms,
the mean per step in us, and the part's share of the mean workgroup's total.  The launch lasts as long as its slowest
workgroup: `total` max is the launch, `total` mean what the average workgroup needs.  The profiled launch itself is
also timed with device events, next to an unprofiled one of the iteration before.

usage: python tools/collect_loop_split.py [arenas=4096] [T=128] [warm=5] [mesh=procedural]
"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "reinforcement-learning_amd")]
from rlgpu import _lib  # noqa: E402
from rlgpu.learner import Learner, LearnerConfig  # noqa: E402
from rlgpu.ppo import GEMM_F16X3  # noqa: E402

SLOTS = 8  # include/rlgpu_env.h RLGPU_COLLECT_SPLIT_SLOTS
PARTS = ("stage", "forward", "sync_a", "load", "body", "store", "sync_b")  # csrc/env_step.hpp kSplit*
TICK_MS = 1e-5  # one tick of the 100 MHz wall clock


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    mesh_name = sys.argv[4] if len(sys.argv) > 4 else "procedural"
    dev = torch.device("cuda:0")
    mesh = None
    if mesh_name == "procedural":
        from rlgpu.mesh import procedural_soccar
        mesh = procedural_soccar()
    L = Learner(LearnerConfig(num_arenas=n, rollout_len=T, train_against_old_versions=False, train_gemm=GEMM_F16X3,
                              mesh=mesh, collect_groups=-1), device=dev)
    L.set_env_timing(True)
    plain_ms = 0.0
    for _ in range(warm):
        plain_ms = L.iterate()["env_kernel_ms"] * T
    torch.cuda.synchronize()
    wg = (n + 3) // 4
    slots = torch.zeros(wg * SLOTS, dtype=torch.int64, device=dev)
    lib = _lib.lib()
    lib.rlgpu_envset_set_collect_split.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    _lib.check(lib.rlgpu_envset_set_collect_split(L.env._h, ctypes.c_void_p(slots.data_ptr()), slots.numel()), "set_collect_split")
    prof_ms = L.iterate()["env_kernel_ms"] * T
    torch.cuda.synchronize()
    _lib.check(lib.rlgpu_envset_set_collect_split(L.env._h, None, 0), "set_collect_split off")
    s = slots.view(wg, SLOTS)[:, :len(PARTS)].double().cpu() * TICK_MS  # ms per workgroup and part, summed over T
    total = s.sum(1)
    print(f"{n} arenas ({wg} workgroups), T = {T}, {mesh_name} mesh, after {warm} iterations; the launch by device events: "
          f"{prof_ms:.2f} ms profiled, {plain_ms:.2f} ms unprofiled (the iteration before)")
    print(f"  {'part':8s} {'mean ms':>9s} {'p50 ms':>9s} {'p99 ms':>9s} {'max ms':>9s} {'us/step':>9s} {'share':>7s}")
    q = torch.tensor([0.5, 0.99], dtype=torch.float64)

    def row(name, v):
        p50, p99 = torch.quantile(v, q).tolist()
        print(f"  {name:8s} {v.mean().item():9.3f} {p50:9.3f} {p99:9.3f} {v.max().item():9.3f} "
              f"{v.mean().item() / T * 1e3:9.2f} {v.mean().item() / total.mean().item() * 100:6.2f}%")

    for i, name in enumerate(PARTS):
        row(name, s[:, i])
    row("fwd_all", s[:, 0] + s[:, 1])
    row("total", total)
    L.close()


if __name__ == "__main__":
    main()

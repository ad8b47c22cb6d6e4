"""What a per-workgroup collection loop could save: the env kernel's per-workgroup cycles (profiled build,
rlgpu_envset_set_profile) of every step of one rollout of the bench workload, summed three ways.

  sum_t max_wg          one launch per step (the launch ends with its slowest workgroup)
  sum_t max per group   today's default: 2 arena groups, each a chain of launches of its own 512 workgroups
  max_wg sum_t          no join between steps: every workgroup runs its own T steps

A C++ Learner with bench.py's configuration runs `warm` whole iterations; the next rollout is then collected
from here, step by step on the Learner's own buffers (same policy, Philox counters and rollout rows as
Learner::Collect), with the per-workgroup counters read and cleared after every step.

usage: python tools/collect_loop_bound.py [arenas=4096] [T=128] [warm=5] [mesh=procedural] [arith=0]
"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "reinforcement-learning_amd")]
from rlgpu import _lib  # noqa: E402
from rlgpu.env import StepOutputs  # noqa: E402
from rlgpu.learner import Learner, LearnerConfig  # noqa: E402
from rlgpu.ppo import GEMM_F16X3  # noqa: E402

PH = list(range(23)) + [30, 31, 33, 34]  # the phase slots (env_kernel.hpp kProfPhases; slot 23 counts solver calls)
KP, KW, APW = 35, 64, 4                  # env_kernel.hpp kProfPhases, kProfWG, kArenas
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
T = int(sys.argv[2]) if len(sys.argv) > 2 else 128
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
mesh_name = sys.argv[4] if len(sys.argv) > 4 else "procedural"
arith = int(sys.argv[5]) if len(sys.argv) > 5 else 0
GROUPS = 2
dev = torch.device("cuda:0")
mesh = None
if mesh_name == "procedural":
    from rlgpu.mesh import procedural_soccar
    mesh = procedural_soccar()
L = Learner(LearnerConfig(num_arenas=n, rollout_len=T, train_against_old_versions=False, train_gemm=GEMM_F16X3,
                          mesh=mesh, arith=arith), device=dev)
for _ in range(warm):
    L.iterate()
torch.cuda.synchronize()
wg = (n + APW - 1) // APW
prof = torch.zeros(KW + wg * KP + n, dtype=torch.int64, device=dev)
lib = _lib.lib()
lib.rlgpu_envset_set_profile.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
_lib.check(lib.rlgpu_envset_set_profile(L.env._h, ctypes.c_void_p(prof.data_ptr()), prof.numel()), "set_profile")
step0 = int(L._stats().rng_step)
cyc = torch.zeros(T, wg, dtype=torch.float64)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
ms = 0.0
for t in range(T):
    L.ppo.infer_actions(L.obs[t], L.masks[t], step=step0 + t, actions=L.actions[t], logp=L.logp[t])
    out = StepOutputs.of(L.obs[t + 1], L.masks[t + 1], L.rewards[t], L.terms[t], L.trunc_obs[t])
    e0.record()
    L.env.step(L.actions[t], True, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms += e0.elapsed_time(e1)
    cyc[t] = prof[KW:KW + wg * KP].view(wg, KP)[:, PH].double().sum(1).cpu()
    prof[KW:].zero_()
_lib.check(lib.rlgpu_envset_set_profile(L.env._h, None, 0), "set_profile off")

per_step_max = cyc.max(1).values
s_launch = per_step_max.sum().item()
half = wg // GROUPS
s_group = [cyc[:, g * half:(g + 1) * half].max(1).values.sum().item() for g in range(GROUPS)]
per_wg = cyc.sum(0)
s_loop = per_wg.max().item()
s_mean = cyc.mean(1).sum().item()
terms = L.terms[:T]
print(f"{n} arenas ({wg} workgroups), T = {T}, {mesh_name} mesh, arith {arith}, after {warm} iterations; "
      f"profiled env launches {ms / T:.3f} ms/step")
print(f"  episode ends in this rollout: {(terms == 1).sum().item()} terminal, {(terms == 2).sum().item()} truncated rows")
print(f"  mean workgroup            {s_mean / T:12.0f} cycles/step   sum_t {s_mean:14.0f}")
print(f"  sum_t max_wg (1 launch)   {s_launch / T:12.0f} cycles/step   sum_t {s_launch:14.0f}   x{s_launch / s_mean:.3f} of the mean")
for g in range(GROUPS):
    print(f"  sum_t max, group {g} of {GROUPS}     {s_group[g] / T:12.0f} cycles/step   sum_t {s_group[g]:14.0f}")
sg = max(s_group)
print(f"  slower group's chain      {sg / T:12.0f} cycles/step   sum_t {sg:14.0f}   x{sg / s_mean:.3f} of the mean")
print(f"  max_wg sum_t (loop)       {s_loop / T:12.0f} cycles/step   sum_t {s_loop:14.0f}   x{s_loop / s_mean:.3f} of the mean")
print(f"  loop / slower group = {s_loop / sg:.4f} ({(1 - s_loop / sg) * 100:.1f} % below); loop / one launch = {s_loop / s_launch:.4f}")
q = torch.quantile(per_wg, torch.tensor([0.0, 0.5, 0.9, 0.99, 1.0], dtype=torch.float64))
print("  per-workgroup sum_t, min / median / p90 / p99 / max: " + " / ".join(f"{x:.0f}" for x in q.tolist()))
qs = torch.quantile(per_step_max, torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64))
print("  per-step max_wg, min / median / max: " + " / ".join(f"{x:.0f}" for x in qs.tolist()))
L.close()

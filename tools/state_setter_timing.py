"""Env-kernel time per fused step with a state setter: per-launch min / median / max (device events) for the
kickoff and for RandomState(true, true, false), at the default terminal list (a reset every 120 steps at the
earliest) and with NoTouchCondition(0.5 s), where every arena is reset every 8th step.

    python tools/state_setter_timing.py [arenas] [steps]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "reinforcement-learning_amd")]
from rlgpu import plugins  # noqa: E402
from rlgpu.env import KICKOFF_STATE, EnvSet, RandomState  # noqa: E402

dev = torch.device("cuda:0")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 64
warm = 8
for tname, terminals in (("default terminals", None), ("NoTouch 0.5 s", [plugins.terminal("NoTouchCondition", 0.5)])):
    for sname, setter in (("kickoff", KICKOFF_STATE), ("RandomState(1,1,0)", RandomState(True, True, False))):
        env = EnvSet(n, seed=1234, device=dev, terminals=terminals, state_setter=setter)
        gen = torch.Generator(device=dev).manual_seed(7)
        acts = torch.empty(4 * n, dtype=torch.int32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms, resets = [], 0
        for i in range(warm + steps):
            acts.copy_(torch.argmax(torch.rand((4 * n, 90), device=dev, generator=gen) * env.action_masks, 1))
            e0.record()
            env.step(acts, True)
            e1.record()
            torch.cuda.synchronize()
            if i >= warm:
                ms.append(e0.elapsed_time(e1))
                resets += int((env.terminals != 0).sum())
        print(f"{n} arenas, {tname}, {sname}: env kernel ms/launch min {min(ms):.3f} median {statistics.median(ms):.3f} "
              f"max {max(ms):.3f} over {steps} launches, {resets} arena resets", flush=True)
        env.close()

"""Env-kernel time per fused step with each obs builder: per-launch min / median / max (device events) for
AdvancedObs, DefaultObs and DefaultObsPadded(3) at the default terminal list.  The sets share seed and actions, and a
builder touches neither the physics nor the streams, so the launches differ in the builder and the row width alone
(167 / 127 / 165 floats per player).

    python tools/obs_builder_timing.py [arenas] [steps]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "reinforcement-learning_amd")]
from rlgpu.env import ADVANCED_OBS, DefaultObs, DefaultObsPadded, EnvSet  # noqa: E402

dev = torch.device("cuda:0")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 64
warm = 8
for name, builder in (("AdvancedObs", ADVANCED_OBS), ("DefaultObs", DefaultObs()), ("DefaultObsPadded(3)", DefaultObsPadded(3))):
    env = EnvSet(n, seed=1234, device=dev, obs_builder=builder)
    gen = torch.Generator(device=dev).manual_seed(7)
    acts = torch.empty(4 * n, dtype=torch.int32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(warm + steps):
        acts.copy_(torch.argmax(torch.rand((4 * n, 90), device=dev, generator=gen) * env.action_masks, 1))
        e0.record()
        env.step(acts, True)
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    print(f"{n} arenas, {name} ({env.obs_size} floats): env kernel ms/launch min {min(ms):.3f} median "
          f"{statistics.median(ms):.3f} max {max(ms):.3f} over {steps} launches", flush=True)
    env.close()

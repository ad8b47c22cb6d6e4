"""Obs standardisation timings (LearnerConfig::standardizeObs): the two kernels at one shape, and the feature's cost
per Learner iteration.

  python tools/obs_stat_bench.py [--rows 16384] [--samples 100] [--steps 128] [--arenas 4096] [--rollout 128]
                                 [--iterations 3] [--no-learner] [--out FILE]

Kernels (HIP events around `--steps` consecutive rlgpu_obs_stat_step calls on one stream, best of 5 repeats):
  step     the update (S = min(rows, samples) dependent fp64 Welford steps per column, one workgroup) + the row rewrite
  rewrite  rows x 167 with max_samples = 1: the rewrite with a one-row update in front of it
  update   `samples` rows only: the update with a rewrite of samples x 167 floats behind it
  copy     a device-to-device hipMemcpyAsync of rows x 167 x 4 bytes on the same device: the same HBM traffic as the
           rewrite (each byte read once, written once), the yardstick the rewrite is held against
Learner (wall time of the collect phase, rlgpu_learner_report, mean of `--iterations` after one warm-up):
  off          standardize_obs off, collect_groups automatic (the collection loop from 4096 arenas on)
  off_per_step standardize_obs off, collect_groups = 1: the per-step path the feature takes, without its kernels
  on           standardize_obs on
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reinforcement-learning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

W = 167


def timed(fn, steps, repeats=5):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / steps)
    return best * 1e3  # us per call


def kernels(args, dev):
    import torch
    from rlgpu.learner import obs_stat_bytes, obs_stat_step
    out = {}
    x = torch.randn((args.rows, W), device=dev)
    y = torch.empty_like(x)
    small = torch.randn((args.samples, W), device=dev)
    for name, buf, ms in (("step", x, args.samples), ("rewrite", x, 1), ("update", small, args.samples)):
        st = torch.zeros(obs_stat_bytes(W), dtype=torch.uint8, device=dev)
        obs_stat_step(st, buf, 1, ms)
        obs_stat_step(st, buf, 1, ms)  # count >= 2: the rewrite is active from here on
        out[name + "_us"] = timed(lambda: obs_stat_step(st, buf, 1, ms), args.steps)
    out["copy_us"] = timed(lambda: y.copy_(x), args.steps)
    traffic = 2 * args.rows * W * 4
    out["traffic_bytes"] = traffic
    out["copy_GBps"] = traffic / out["copy_us"] * 1e-3
    out["rewrite_GBps"] = traffic / out["rewrite_us"] * 1e-3
    out["rewrite_vs_copy"] = out["rewrite_us"] / out["copy_us"]
    out["update_us_per_sample"] = out["update_us"] / args.samples
    return out


def learner(args, dev):
    import torch
    from rlgpu.learner import Learner, LearnerConfig
    out = {}
    for name, kw in (("off", {}), ("off_per_step", dict(collect_groups=1)), ("on", dict(standardize_obs=True))):
        L = Learner(LearnerConfig(num_arenas=args.arenas, rollout_len=args.rollout, train_against_old_versions=False, **kw),
                    device=dev)
        L.iterate()
        reps = [L.iterate() for _ in range(args.iterations)]
        torch.cuda.synchronize()
        out[name] = {k: sum(r[k] for r in reps) / len(reps) * 1e3 for k in ("collect_s", "consume_s", "learn_s", "iteration_s")}
        out[name]["env_launch_arenas"] = reps[-1]["env_launch_arenas"]
        L.close()
    out["on_minus_off_per_step_collect_ms"] = out["on"]["collect_s"] - out["off_per_step"]["collect_s"]
    out["on_minus_off_collect_ms"] = out["on"]["collect_s"] - out["off"]["collect_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--arenas", type=int, default=4096)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--no-learner", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    res = {"shape": [args.rows, W], "samples": args.samples, "steps": args.steps, "device": torch.cuda.get_device_name(0),
           "kernels": kernels(args, dev)}
    if not args.no_learner:
        res["learner_ms"] = learner(args, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

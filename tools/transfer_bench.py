"""Times the host Learner's transfer-learning iteration (rlgpu_learner_transfer_iterate) on an MI355X: the report's
collect_s / learn_s (host clocks around work that ends in a stream synchronise) over `--iters` iterations after
`--warmup` untimed ones, one JSON line.  Defaults: 4096 arenas, T = 4 (65,536 rows), 5 epochs, [512, 512] student and
teacher.  Run it several times and compare: python tools/transfer_bench.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reinforcement-learning_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=4096)
    ap.add_argument("--rollout", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--layers", default="512,512")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    import torch
    from rlgpu.learner import Learner, LearnerConfig, TransferLearnConfig
    from rlgpu.ppo import PPO
    assert torch.cuda.is_available(), "transfer_bench needs a GPU"
    layers = tuple(int(x) for x in a.layers.split(","))
    L = Learner(LearnerConfig(num_arenas=a.arenas, rollout_len=a.rollout, policy_layers=layers, critic_layers=layers,
                              train_against_old_versions=False))
    T = PPO(policy_layers=layers, critic_layers=(8,), max_rows=min(a.rollout * 4 * a.arenas, 65536), seed=77)
    L.set_teacher(T)
    cfg = TransferLearnConfig(epochs=a.epochs)
    for _ in range(a.warmup):
        L.transfer_iterate(cfg)
    reps = [L.transfer_iterate(cfg) for _ in range(a.iters)]
    out = {"arenas": a.arenas, "rollout": a.rollout, "rows": a.rollout * 4 * a.arenas, "epochs": a.epochs, "layers": layers,
           "iters": a.iters, "max_rows": L.ppo.max_rows}
    for k in ("collect_s", "learn_s"):
        xs = [r[k] for r in reps]
        out[k] = {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}
    out["last_report"] = reps[-1]["report"]
    print(json.dumps(out))
    L.close()
    T.close()


if __name__ == "__main__":
    main()

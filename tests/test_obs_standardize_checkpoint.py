"""The obs statistic in checkpoints: RUNNING_STATS.json "obs_stat" = {"means": [167], "vars": [167] (the running m2),
"count": n}, BatchedWelfordStat::ToJSON's keys (Learner.cpp:184-185, 214-215), through rlgpu/checkpoint.py and the C++
trainer facade (rlgpu_train --standardize-obs).

A checkpoint holds no env state, so a learner resumed from one collects other raw rows than the learner that wrote it
went on to collect: their rollouts cannot be compared with each other.  What "resumes exactly" means is checked
instead against the restatement (tests/test_obs_standardize.py) continued from the saved state over the raw rows the
resumed learner records: its row 0 is standardised with the loaded statistic, its draws continue at the loaded count,
and its state after the iteration is the continued restatement's, bit for bit.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from test_obs_standardize import BASE, RefStat, S, W, _learner, _record, _same_rows, _stat_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "reinforcement-learning_amd", "rlgpu", "rlgpu_train")


def _stats_file(folder):
    dirs = sorted(int(d) for d in os.listdir(folder) if d.isdigit())
    assert dirs, os.listdir(folder)
    return os.path.join(folder, str(dirs[-1]), "RUNNING_STATS.json")


def test_python_checkpoint_resumes_the_statistic(gpu, tmp_path):
    import torch
    kw = dict(standardize_obs=True, deterministic=True, checkpoint_folder=str(tmp_path))
    A = _learner(gpu, **kw)
    A.iterate()
    A.save()
    T = A.T
    saved = _stat_bits(A)
    j = json.load(open(_stats_file(tmp_path)))["obs_stat"]
    assert sorted(j) == ["count", "means", "vars"] and len(j["means"]) == W and len(j["vars"]) == W
    assert isinstance(j["count"], int) and j["count"] == S * (T + 1) == saved[0]
    B = _learner(gpu, **kw)  # loads it at construction
    assert B.last_checkpoint is not None and _stat_bits(B) == saved
    ref = RefStat()
    ref.count, ref.mean, ref.m2 = j["count"], np.array(j["means"], np.float64), np.array(j["vars"], np.float64)
    raw, _ = _record(B)
    B.collect()
    torch.cuda.synchronize()
    obs = B.obs.cpu().numpy()
    for k in range(T + 1):  # row 0 included: it met the loaded statistic, not a fresh one
        _same_rows(obs[k], ref.step(raw[k], BASE["seed"])[0], ("resumed row", k))
    assert _stat_bits(B) == (saved[0] + S * (T + 1), ref.mean.view(np.uint64).tolist(), ref.m2.view(np.uint64).tolist())
    # the uninterrupted learner's statistic has advanced by the same number of rows (T: its row 0 was carried over)
    A.iterate()
    assert A.obs_stat.n == saved[0] + S * T
    A.close()
    B.close()


def test_checkpoint_without_obs_stat_loads_fresh(gpu, tmp_path):
    A = _learner(gpu, checkpoint_folder=str(tmp_path))
    A.iterate()
    A.save()
    assert "obs_stat" not in json.load(open(_stats_file(tmp_path)))
    params = A.ppo.params.clone()
    A.close()
    B = _learner(gpu, standardize_obs=True, checkpoint_folder=str(tmp_path))
    import torch
    assert B.last_checkpoint is not None and torch.equal(B.ppo.params, params)
    n, mean, m2 = B.obs_stat.get()
    assert n == 0 and not mean.any() and not m2.any()
    B.close()


def test_hand_written_obs_stat_round_trips(gpu, tmp_path):
    """An obs_stat written by hand in the reference's JSON shape (made here, from a formula) is what a loading learner
    reports and what it saves again."""
    a, b = tmp_path / "a", tmp_path / "b"
    A = _learner(gpu, standardize_obs=True, checkpoint_folder=str(a))
    A.iterate()
    A.save()
    A.close()
    f = _stats_file(str(a))
    j = json.load(open(f))
    k = np.arange(W, dtype=np.float64)
    hand = {"means": (np.sin(k) * 3.3 + 1e-17).tolist(), "vars": (k * k * 1234.5678 + 0.1).tolist(), "count": 123457}
    hand["vars"][0] = 0.0
    j["obs_stat"] = hand
    json.dump(j, open(f, "w"), indent=4)
    B = _learner(gpu, standardize_obs=True, checkpoint_folder=str(a))
    n, mean, m2 = B.obs_stat.get()
    assert n == 123457 and mean.tolist() == hand["means"] and m2.tolist() == hand["vars"]
    B.cfg.checkpoint_folder = str(b)
    B.save()
    assert json.load(open(_stats_file(str(b))))["obs_stat"] == hand
    B.close()


def test_facade_standardize_obs(gpu, tmp_path):
    """GGL::Learner with LearnerConfig::standardizeObs = true (rlgpu_train --standardize-obs): constructs, runs one
    iteration, Save writes obs_stat, Load restores it (a Load + Save round trip writes the same JSON), the Python
    loader reads it; minObsSTD = 0 is refused by name."""
    a, b = tmp_path / "a", tmp_path / "b"
    args = ["--arenas", "8", "--rollout", "8", "--seed", "11", "--c2-model", "--standardize-obs"]
    env = dict(os.environ, RLGPU_MAX_ITERATIONS="1")
    r = subprocess.run([TRAIN, *args, "--iterations", "1", "--checkpoint-folder", str(a)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    ja = json.load(open(_stats_file(str(a))))
    o = ja["obs_stat"]
    assert len(o["means"]) == W and len(o["vars"]) == W and o["count"] == 32 * (8 + 1)
    assert any(v > 0 for v in o["vars"])
    r = subprocess.run([TRAIN, *args, "--checkpoint-folder", str(a), "--resave-to", str(b)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.load(open(_stats_file(str(b)))) == ja
    from rlgpu.learner import Learner, LearnerConfig
    L = Learner(LearnerConfig(num_arenas=8, rollout_len=8, seed=11, mini_batch_size=256, standardize_obs=True,
                              checkpoint_folder=str(a), train_against_old_versions=False), device=gpu)
    n, mean, m2 = L.obs_stat.get()
    assert n == o["count"] and mean.tolist() == o["means"] and m2.tolist() == o["vars"]
    L.close()
    r = subprocess.run([TRAIN, *args, "--iterations", "1", "--min-obs-std", "0"], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode != 0 and "minObsSTD" in r.stdout + r.stderr, r.stdout + r.stderr

"""Transfer learning through the C++ Learner and its Python mirror (rlgpu_learner_set_teacher,
rlgpu_learner_transfer_iterate, Learner.start_transfer_learn).

8 arenas (P = 32), rollout_len = 2 (64 rows, one chunk), student [32, 32], teacher [48] from another seed, 3 epochs:
  * after transfer_iterate the student's parameters equal, bit for bit, a replay of the C-ABI building blocks on a twin
    handle over the rollout's own rows (teacher_probs, then per epoch transfer_chunk over the same chunks and
    transfer_step); the critic, its moments and its step count are untouched; the per-model step counts are 3 / 0;
  * the reported metrics are the replay's: accuracy and update magnitude's inputs exactly, the sums whose atomic order
    is free (loss: 2 blocks, exact; the entropies) to 1e-6 relative;
  * the second iteration starts from the last obs;
  * every unsupported combination returns its documented status (-5, the reason in the message; -4 without a teacher;
    -1 for loss_exponent < 1 or a non-finite loss_scale, before anything is collected): frame stacking, the trajectory
    mode, obs standardisation, deterministic, an old team set (through the C ABI: the Python method clears it), and
    world > 1 (a world = 2 learner whose collective is a single-process stand-in: rank 0's sums are its own values);
  * the trainer facade (rlgpu_train --transfer-learn, GGL::Learner::StartTransferLearn with the native AdvancedObs /
    DefaultAction): two iterations from a [48] teacher's POLICY.lt run, report and save; the checkpoint carries per-model step
    counts (the critic's stays 0), which Load + Save reproduce; a mapActsFn throws the message naming the gap; a
    folder without POLICY.lt is an error naming the file.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPOCHS, LR = 3, 3e-4


def _learner(gpu, **kw):
    from rlgpu.learner import Learner, LearnerConfig
    base = dict(num_arenas=8, rollout_len=2, policy_layers=(32, 32), critic_layers=(32, 32), seed=5,
                train_against_old_versions=False)
    return Learner(LearnerConfig(**{**base, **kw}), device=gpu)


def _teacher(gpu, max_rows=64):
    from rlgpu.ppo import PPO
    return PPO(policy_layers=(48,), critic_layers=(8,), max_rows=max_rows, seed=77, device=gpu)


def _cfg(**kw):
    from rlgpu.learner import TransferLearnConfig
    return TransferLearnConfig(**{**dict(lr=LR, epochs=EPOCHS, use_kl_div=True, loss_scale=500.0, loss_exponent=2.0), **kw})


def test_transfer_iterate_equals_replay(gpu):
    import torch
    from rlgpu.ppo import PPO, diff_norm
    L, T_ = _learner(gpu), _teacher(gpu)
    T, P, W = L.T, L.P, L.W
    cfg = _cfg()
    L.set_teacher(T_)
    pre = {m: L.ppo.model_slice(m).clone() for m in L.ppo.models}
    step0, m0, v0 = L.ppo.optimizer_state()
    o1, c1 = L.ppo.model_range(1)
    obs0, masks0 = L.obs[0].clone(), L.masks[0].clone()
    steps0 = L.total_steps
    r = L.transfer_iterate(cfg)
    torch.cuda.synchronize()
    rep = r["report"]
    assert r["collect_s"] > 0 and r["learn_s"] > 0
    assert L.total_steps == steps0 + T * P and L.iteration == 1
    # the rollout's own rows: row 0 as it was before the iteration (finish moved the last obs there), rows 1 .. T - 1
    obs = torch.cat([obs0[None], L.obs[1:T]]).reshape(T * P, W)
    masks = torch.cat([masks0[None], L.masks[1:T]]).reshape(T * P, 90)
    assert torch.equal(L.obs[0], L.obs[T]) and torch.equal(L.masks[0], L.masks[T])  # the next rollout's start
    twin = PPO(policy_layers=L.cfg.policy_layers, critic_layers=L.cfg.critic_layers, max_rows=L.ppo.max_rows, seed=1,
               init=False, device=gpu)
    for m in twin.models:
        twin.model_slice(m).copy_(pre[m])
    twin.refresh_half()
    tm = torch.zeros(16, device=gpu)
    probs, arg = T_.teacher_probs(obs, masks, metrics=tm)
    twin.zero_grad()
    first = None
    N = T * P
    for e in range(EPOCHS):
        twin.metrics.zero_()
        for s0 in range(0, N, twin.max_rows):
            twin.transfer_chunk(obs, masks, probs, arg, None, s0, min(twin.max_rows, N - s0), N, cfg.use_kl_div,
                                cfg.loss_scale, cfg.loss_exponent)
        first = twin.metrics.clone() if first is None else first
        twin.transfer_step(LR)
    torch.cuda.synchronize()
    for m in (0, 1):
        assert torch.equal(L.ppo.model_slice(m).view(torch.int32), twin.model_slice(m).view(torch.int32)), f"model {m}"
    assert not torch.equal(L.ppo.model_slice(0), pre[0])
    # the critic: parameters, moments, step count
    assert torch.equal(L.ppo.model_slice(1).view(torch.int32), pre[1].view(torch.int32))
    _, m1, v1 = L.ppo.optimizer_state()
    assert not bool(m1[o1:o1 + c1].any()) and not bool(v1[o1:o1 + c1].any())
    assert [L.ppo.model_optimizer_step(m) for m in (0, 1)] == [EPOCHS, 0]
    # metrics
    want = {"Old Policy Entropy": float(tm[13]), "Transfer Learn Accuracy": float(first[12]),
            "Transfer Learn Loss": float(first[11]), "Policy Entropy": float(first[0]),
            "Policy Update Magnitude": diff_norm(pre[0], twin.model_slice(0))}
    print(rep, want)
    assert set(rep) == set(want)
    assert rep["Transfer Learn Accuracy"] == want["Transfer Learn Accuracy"]
    assert rep["Policy Update Magnitude"] == want["Policy Update Magnitude"] > 0
    for k, w in want.items():
        assert np.isfinite(rep[k]) and abs(rep[k] - w) <= 1e-6 * abs(w), k
    assert rep["Transfer Learn Loss"] > 0 and 0 < rep["Old Policy Entropy"] <= 1
    # a second iteration starts from the last obs and runs
    start = L.obs[0].clone()
    L.transfer_iterate(cfg)
    torch.cuda.synchronize()
    assert L.iteration == 2 and [L.ppo.model_optimizer_step(m) for m in (0, 1)] == [2 * EPOCHS, 0]
    assert not torch.equal(L.obs[0], start)
    # an ordinary iteration still runs afterwards and advances every count
    L.iterate()
    assert L.ppo.model_optimizer_step(1) > 0
    twin.close()
    L.close()
    T_.close()


@pytest.mark.parametrize("kw,why", [(dict(frame_stack=2), "frame stacking"),
                                    (dict(experience_mode=1, max_episode_duration=1.0), "trajectory mode"),
                                    (dict(standardize_obs=True), "obs standardisation"),
                                    (dict(deterministic=True), "deterministic")])
def test_unsupported_combinations(gpu, kw, why):
    from rlgpu import _lib
    L = _learner(gpu, **kw)
    T_ = _teacher(gpu)
    L.set_teacher(T_)
    before = L.ppo.model_slice(0).clone()
    with pytest.raises(_lib.RLGPUError, match=rf"\(-5\).*{why}"):
        L.transfer_iterate(_cfg())
    import torch
    assert torch.equal(L.ppo.model_slice(0), before) and L.iteration == 0
    L.close()
    T_.close()


def _raw_transfer_iterate(L, **kw):
    """rlgpu_learner_transfer_iterate through ctypes, without the Python method's own preparation; the status."""
    from rlgpu import _lib
    from rlgpu.learner import _CTransfer
    c = _cfg(**kw)
    tc = _CTransfer(c.lr, c.epochs, int(c.use_kl_div), c.loss_scale, c.loss_exponent)
    return _lib.lib().rlgpu_learner_transfer_iterate(L._h, ctypes.byref(tc), None)


def test_old_team_is_refused(gpu):
    import torch
    from rlgpu import _lib
    L, T_ = _learner(gpu), _teacher(gpu)
    L.set_teacher(T_)
    L.ppo.set_version(L.ppo.policy_version().clone())
    _lib.check(_lib.lib().rlgpu_learner_set_old_team(L._h, 1), "set_old_team")
    before = L.ppo.model_slice(0).clone()
    assert _raw_transfer_iterate(L) == -5 and "old version playing" in _lib.last_error()
    assert torch.equal(L.ppo.model_slice(0), before) and L.iteration == 0
    _lib.check(_lib.lib().rlgpu_learner_set_old_team(L._h, -1), "set_old_team")
    assert _raw_transfer_iterate(L) == 0 and L.iteration == 1
    L.close()
    T_.close()


def test_world_2_is_refused(gpu, monkeypatch):
    """A world = 2 learner (rank 0) over a stand-in collective whose sums and gathers leave rank 0's values in place."""
    import rlgpu.dist as rdist
    from rlgpu import _lib
    from rlgpu.learner import Learner, LearnerConfig

    class Alone:
        def __init__(self, group=None, device="cuda:0"):
            def gather(_u, src, n, dst):
                ctypes.memmove(dst, src, 4 * n)
                ctypes.memmove(dst + 4 * n, src, 4 * n)
                return 0
            self._c = rdist.CCollective(None, rdist._ALLREDUCE_F32(lambda _u, _b, _n: 0),
                                        rdist._ALLREDUCE_F64(lambda _u, _b, _n: 0), rdist._ALLGATHER_F32(gather))

        def c_struct(self):
            return self._c

        def close(self):
            pass

    monkeypatch.setattr(rdist, "TorchCollective", Alone)
    L = Learner(LearnerConfig(num_arenas=8, rollout_len=2, policy_layers=(32, 32), critic_layers=(32, 32), seed=5,
                              train_against_old_versions=False), device=gpu, rank=0, world=2)
    T_ = _teacher(gpu)
    L.set_teacher(T_)
    with pytest.raises(_lib.RLGPUError, match=r"\(-5\).*world > 1"):
        L.transfer_iterate(_cfg())
    assert L.iteration == 0
    L.close()
    T_.close()


def test_teacher_and_exponent_are_required(gpu):
    from rlgpu import _lib
    L = _learner(gpu)
    with pytest.raises(_lib.RLGPUError, match=r"\(-4\).*no teacher"):
        L.transfer_iterate(_cfg())
    T_ = _teacher(gpu)
    L.set_teacher(T_)
    with pytest.raises(_lib.RLGPUError, match=r"\(-1\).*loss_exponent.*NaN"):
        L.transfer_iterate(_cfg(loss_exponent=0.5))
    start = L.obs[0].clone()
    with pytest.raises(_lib.RLGPUError, match=r"\(-1\).*loss_scale"):  # refused before the rollout is collected
        L.transfer_iterate(_cfg(loss_scale=float("inf")))
    import torch
    assert L.iteration == 0 and L.total_steps == 0 and torch.equal(L.obs[0], start)
    L.close()
    T_.close()


def test_start_transfer_learn_loads_teacher_and_saves(gpu, tmp_path):
    """Learner.start_transfer_learn with a teacher read from a checkpoint folder (POLICY.lt of other widths): two
    iterations, a checkpoint whose per-model step counts differ and read back; a folder without POLICY.lt raises, naming
    the file; a map_acts_fn is refused with the remaining gap in the message."""
    import os
    import torch
    from rlgpu import _lib, checkpoint
    from rlgpu.learner import Learner, LearnerConfig
    T_ = _teacher(gpu)
    old = tmp_path / "old"
    old.mkdir()
    checkpoint.write_model(T_.torch_module(0), checkpoint.model_path(str(old), "policy"))
    L = _learner(gpu, checkpoint_folder=str(tmp_path / "ckpt"), ts_per_save=0)
    cfg = _cfg(old_policy_layers=(48,), old_models_path=str(old), epochs=2)
    made = L.make_teacher(cfg)  # the loaded teacher is T_, tensor for tensor; its critic is never read
    assert torch.equal(made.model_slice(0), T_.model_slice(0)) and float(T_.model_slice(0).abs().max()) > 0
    made.close()
    # a teacher with a shared head and its own LayerNorm / activation setting: POLICY.lt and SHARED_HEAD.lt both land
    from rlgpu.ppo import PPO
    T2 = PPO(policy_layers=(24,), critic_layers=(8,), shared_layers=(40,), layer_norm=False, activation="tanh", max_rows=64,
             seed=3, device=gpu)
    old2 = tmp_path / "old2"
    old2.mkdir()
    for mi, name in ((0, "policy"), (2, "shared_head")):
        checkpoint.write_model(T2.torch_module(mi), checkpoint.model_path(str(old2), name))
    cfg2 = _cfg(old_policy_layers=(24,), old_shared_layers=(40,), old_layer_norm=False, old_activation="tanh",
                old_models_path=str(old2))
    made = L.make_teacher(cfg2)
    for mi in (0, 2):
        assert torch.equal(made.model_slice(mi), T2.model_slice(mi)) and float(T2.model_slice(mi).abs().max()) > 0
    obs = L.obs[0]
    assert torch.equal(made.forward(0, obs, half=True), T2.forward(0, obs, half=True))
    made.close()
    os.remove(checkpoint.model_path(str(old2), "shared_head"))
    with pytest.raises(FileNotFoundError, match="SHARED_HEAD.lt"):
        L.make_teacher(cfg2)
    with pytest.raises(ValueError, match="old_models_path"):
        L.make_teacher(_cfg(old_policy_layers=(48,)))
    T2.close()
    reps = L.start_transfer_learn(cfg, 2)
    assert len(reps) == 2 and all("checkpoint" in r for r in reps)
    assert all(np.isfinite(list(r["report"].values())).all() for r in reps)
    assert [L.ppo.model_optimizer_step(m) for m in (0, 1)] == [4, 0]
    params = L.ppo.flat().clone()
    L2 = Learner(LearnerConfig(num_arenas=8, rollout_len=2, policy_layers=(32, 32), critic_layers=(32, 32), seed=6,
                               train_against_old_versions=False, checkpoint_folder=str(tmp_path / "ckpt")), device=gpu)
    assert checkpoint.load(L2, str(tmp_path / "ckpt")) is not None
    assert torch.equal(L2.ppo.flat(), params)
    assert [L2.ppo.model_optimizer_step(m) for m in (0, 1)] == [4, 0]
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="POLICY.lt"):
        L.start_transfer_learn(_cfg(old_policy_layers=(48,), old_models_path=str(empty)), 1)
    with pytest.raises(_lib.RLGPUError, match="host-side evaluation of the old builders"):
        L.start_transfer_learn(_cfg(old_models_path=str(old), map_acts_fn=lambda player, state: list(range(90))), 1)
    assert os.path.isdir(tmp_path / "ckpt")
    L.close()
    L2.close()
    T_.close()


# ------------------------------------------------------------------ the trainer facade
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "reinforcement-learning_amd", "rlgpu", "rlgpu_train")


def test_facade_start_transfer_learn(gpu, tmp_path):
    """GGL::Learner::StartTransferLearn through rlgpu_train --transfer-learn (module docstring)."""
    import torch
    from safetensors.torch import load_file
    from rlgpu import checkpoint
    T_ = _teacher(gpu)
    old, a, b = tmp_path / "old", tmp_path / "a", tmp_path / "b"
    old.mkdir()
    checkpoint.write_model(T_.torch_module(0), checkpoint.model_path(str(old), "policy"))
    T_.close()
    base = [TRAIN, "--arenas", "8", "--rollout", "2", "--seed", "11", "--c2-model"]
    tl = ["--transfer-learn", str(old), "--old-policy-layers", "48", "--tl-epochs", "3", "--tl-kl", "--tl-lr", "1e-3",
          "--tl-loss-scale", "100", "--tl-loss-exponent", "2"]
    # two iterations of Start()'s loop: the first displays its report, the last saves and leaves
    r = subprocess.run([*base, *tl, "--iterations", "2", "--checkpoint-folder", str(a)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for key in ("Transfer Learn Loss", "Transfer Learn Accuracy", "Old Policy Entropy", "Policy Update Magnitude"):
        assert key in r.stdout, r.stdout
    dirs = sorted(int(d) for d in os.listdir(a) if d.isdigit())
    assert dirs == [4 * 32], os.listdir(a)  # two iterations' steps
    fa = os.path.join(a, str(dirs[-1]))
    sa = load_file(os.path.join(fa, "RLGPU_OPTIM.safetensors"))
    assert (int(sa["step"][0]), int(sa["policy.step"][0]), int(sa["critic.step"][0])) == (6, 6, 0)  # 2 iterations x 3 epochs
    assert not bool(sa["critic.exp_avg"].any()) and bool(sa["policy.exp_avg"].any())
    shapes = {"policy": [(512, 167), (512,), (512,), (512,), (512, 512), (512,), (512,), (512,), (90, 512), (90,)],
              "critic": [(512, 167), (512,), (512,), (512,), (512, 512), (512,), (512,), (512,), (1, 512), (1,)]}
    for name, want in (("policy", 6), ("critic", 0)):
        assert checkpoint.read_optim_archive(os.path.join(fa, name.upper() + "_OPTIM.lt"), shapes[name])[0] == want
    # Load + Save reproduce the counts
    r = subprocess.run([*base, "--checkpoint-folder", str(a), "--resave-to", str(b)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    sb = load_file(os.path.join(b, str(dirs[-1]), "RLGPU_OPTIM.safetensors"))
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    # a mapActsFn is refused with the message naming the gap; a folder without POLICY.lt names the file
    r = subprocess.run([*base, *tl, "--tl-map-acts", "--iterations", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "mapActsFn is set" in r.stderr and "host-side evaluation of the old builders" in r.stderr, \
        r.stdout + r.stderr
    empty = tmp_path / "empty"
    empty.mkdir()
    r = subprocess.run([*base, "--transfer-learn", str(empty), "--old-policy-layers", "48", "--iterations", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "POLICY.lt does not exist" in r.stderr, r.stdout + r.stderr

"""The guiding policy through the C++ Learner, its Python config and the trainer (rlgpu_learner_set_guide,
LearnerConfig.use_guiding_policy, rlgpu_train --guiding-policy).

24 arenas, T = 24, one epoch, batch = the whole rollout, one minibatch:
  * the Learner's guide-logit buffer after learn() is the guide's 16-bit forward over obs[0 .. T), bit for bit;
  * the first batch's gradient (the grad hook) agrees with a twin PPO holding the pre-learn parameters, driven by
    minibatch(guide_logits=...) over the exported permutation with adv_normalizer, normwise to 1e-5 (the project's
    bound for the same rows in test_dist_gpu); whether the two are in fact bit-equal is printed;
  * "Guiding Loss" is reported, positive and finite;
  * the trajectory mode runs its guide pass over the combined batch's rows;
  * LearnerConfig(use_guiding_policy=True, guiding_policy_path=<a saved checkpoint>) trains, and a folder without
    POLICY.lt raises, naming the file; rlgpu_train --guiding-policy does the same from the command line.
"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "reinforcement-learning_amd", "rlgpu", "rlgpu_train")
STRENGTH = 0.5


def _learner(gpu, **kw):
    from rlgpu.learner import Learner, LearnerConfig
    T, n = 24, 24
    base = dict(num_arenas=n, rollout_len=T, mini_batch_size=T * 4 * n, epochs=1, seed=5, train_against_old_versions=False)
    return Learner(LearnerConfig(**{**base, **kw}), device=gpu)


def _other_policy(L, seed):
    """The flat policy parameters (+ shared head) of another initialisation of L's architecture."""
    from rlgpu.ppo import PPO
    q = PPO(policy_layers=L.cfg.policy_layers, critic_layers=L.cfg.critic_layers, shared_layers=L.cfg.shared_layers,
            max_rows=64, seed=seed)
    v = q.policy_version().clone()
    q.close()
    return v


def test_learner_guide_buffer_gradient_and_metric(gpu):
    import torch
    from rlgpu.ppo import PPO, permutation
    L = _learner(gpu)
    T, P, W = L.T, L.P, L.W
    guide_params = _other_policy(L, 77)
    L.set_guide(guide_params, STRENGTH)
    assert L.guide_logits_view() is None  # nothing before the first guided learn
    grads = []
    L.set_grad_hook(lambda g, epoch, batch: grads.append((epoch, batch, g.clone())))
    L.collect()
    L.consume()
    torch.cuda.synchronize()
    pre = {m: L.ppo.model_slice(m).clone() for m in L.ppo.models}
    it = L.iteration
    L.learn()
    torch.cuda.synchronize()
    # the guide buffer: the guide's 16-bit forward over the rows Learn trains on
    view = L.guide_logits_view()
    assert view is not None and view.shape == (T * P, 90) and view.dtype == torch.bfloat16
    obs = L.obs[:T].reshape(T * P, W)
    assert torch.equal(view.view(torch.int16), L.ppo.guide_logits(obs).view(torch.int16))
    # the first batch's gradient against a twin handle on the same rows in the same order
    assert len(grads) == 1 and grads[0][:2] == (0, 0)
    twin = PPO(policy_layers=L.cfg.policy_layers, critic_layers=L.cfg.critic_layers, max_rows=T * P, seed=1, init=False)
    for m in twin.models:
        twin.model_slice(m).copy_(pre[m])
    twin.refresh_half()
    twin.set_guide(guide_params)
    tg = twin.guide_logits(obs)
    assert torch.equal(tg.view(torch.int16), view.view(torch.int16))
    perm = permutation(T * P, L.cfg.seed, it * L.cfg.epochs, device=gpu)
    adv = L.adv.reshape(-1)
    twin.adv_normalizer(adv)
    twin.zero_grad()
    twin.minibatch(obs, L.masks[:T].reshape(T * P, 90), L.actions.reshape(-1), L.logp.reshape(-1), adv,
                   L.target.reshape(-1), perm, 0, T * P, T * P, guide_logits=tg, guiding_strength=STRENGTH)
    torch.cuda.synchronize()
    g, w = grads[0][2].double(), twin.grads.double()
    rel = float((g - w).norm() / w.norm())
    print(f"learner vs twin first-batch gradient: ||diff|| / ||g|| = {rel:.3g}, bit-equal: {torch.equal(grads[0][2], twin.grads)}")
    assert float(w.norm()) > 0 and rel <= 1e-5, rel
    # without the guide the twin's gradient is another one: the learner's batch did include the term
    twin.zero_grad()
    twin.minibatch(obs, L.masks[:T].reshape(T * P, 90), L.actions.reshape(-1), L.logp.reshape(-1), adv,
                   L.target.reshape(-1), perm, 0, T * P, T * P)
    torch.cuda.synchronize()
    o, c = twin.model_range(0)
    assert float((twin.grads[o:o + c].double() - g[o:o + c]).norm() / g[o:o + c].norm()) > 1e-4
    m = L.ppo.read_metrics()
    assert np.isfinite(m["Guiding Loss"]) and m["Guiding Loss"] > 0
    twin.close()
    L.close()


def test_learner_guide_trajectory_mode(gpu):
    """experience_mode 1: one iterate() with a guide; the guide rows are the combined batch's rows."""
    import torch
    L = _learner(gpu, num_arenas=16, rollout_len=8, mini_batch_size=700, max_episode_duration=1.0, experience_mode=1,
                 ts_per_itr=1200, epochs=2)
    L.set_guide(_other_policy(L, 77), STRENGTH)
    L.collect()
    L.consume()
    rows = L.batch()["num_rows"]
    obs = L.batch()["obs"].clone()
    L.learn()
    torch.cuda.synchronize()
    view = L.guide_logits_view()
    assert rows > 0 and view is not None and view.shape[0] == rows
    assert torch.equal(view.view(torch.int16), L.ppo.guide_logits(obs).view(torch.int16))
    L.finish_iteration()
    L.iterate()
    assert torch.isfinite(L.ppo.flat()).all()
    m = L.ppo.read_metrics()
    assert np.isfinite(m["Guiding Loss"]) and m["Guiding Loss"] > 0
    L.close()


def test_learner_config_guiding_policy_path(gpu, tmp_path):
    """use_guiding_policy reads <path>/POLICY.lt (and SHARED_HEAD.lt with a shared head) of a saved checkpoint; a
    folder without POLICY.lt raises, naming the file; so does a model of another size."""
    import torch
    folder = str(tmp_path / "ckpt")
    kw = dict(shared_layers=(64,), policy_layers=(96, 33), critic_layers=(40, 64))
    A = _learner(gpu, checkpoint_folder=folder, ts_per_save=0, **kw)
    A.iterate()
    ckpt = A.last_checkpoint
    want = A.ppo.policy_version().clone()
    A.close()
    assert ckpt and os.path.exists(os.path.join(ckpt, "POLICY.lt")) and os.path.exists(os.path.join(ckpt, "SHARED_HEAD.lt"))
    L = _learner(gpu, use_guiding_policy=True, guiding_policy_path=ckpt, guiding_strength=STRENGTH, seed=9, **kw)
    assert torch.equal(L._guide_params, want)
    before = L.ppo.flat().clone()
    L.iterate()
    assert torch.isfinite(L.ppo.flat()).all() and not torch.equal(before, L.ppo.flat())
    m = L.ppo.read_metrics()
    assert np.isfinite(m["Guiding Loss"]) and m["Guiding Loss"] > 0
    L.close()
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="POLICY.lt"):
        _learner(gpu, use_guiding_policy=True, guiding_policy_path=str(empty), **kw)
    with pytest.raises(ValueError, match="POLICY.lt"):
        _learner(gpu, use_guiding_policy=True, guiding_policy_path=ckpt, **dict(kw, policy_layers=(96, 40)))


def test_rlgpu_train_guiding_policy(gpu, tmp_path):
    """rlgpu_train: a 2-iteration run saves a checkpoint; a second run guided by that numbered folder exits 0 and
    prints a finite positive Guiding Loss; a missing folder exits non-zero and names the file."""
    a = tmp_path / "a"
    args = ["--arenas", "32", "--rollout", "16", "--seed", "11"]
    r = subprocess.run([TRAIN, *args, "--iterations", "2", "--checkpoint-folder", str(a)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    dirs = sorted(int(d) for d in os.listdir(a) if d.isdigit())
    ckpt = os.path.join(str(a), str(dirs[-1]))
    r = subprocess.run([TRAIN, *args, "--iterations", "2", "--guiding-policy", ckpt, "--guiding-strength", "0.5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    vals = [float(v) for v in re.findall(r"Guiding Loss: (\S+)", r.stdout)]
    assert len(vals) == 2 and all(np.isfinite(v) and v > 0 for v in vals), r.stdout
    r = subprocess.run([TRAIN, *args, "--iterations", "1", "--guiding-policy", str(tmp_path / "nowhere")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "POLICY.lt" in r.stdout + r.stderr, r.stdout + r.stderr
    r = subprocess.run([TRAIN, *args, "--iterations", "1", "--guiding-policy", ckpt, "--fp32-inference"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "useGuidingPolicy" in r.stdout + r.stderr, r.stdout + r.stderr

"""policyTemperature and maskEntropy through the C++ Learner (LearnerConfig.policy_temperature / mask_entropy) and
the trainer facade (rlgpu_train --policy-temperature X --mask-entropy): collection samples at the temperature, Learn
applies the same temperature, the entropy report is normalised per row."""
import os
import subprocess

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "reinforcement-learning_amd", "rlgpu", "rlgpu_train")


def _run(gpu, temperature, mask_entropy):
    """One collect / consume / learn of a Learner whose iteration is exactly one minibatch (8 arenas x 4 players x 8
    steps = 256 rows), so the learn metrics describe the pre-update parameters.  Returns what the tests compare."""
    import torch
    from rlgpu.learner import Learner, LearnerConfig
    L = Learner(LearnerConfig(num_arenas=8, rollout_len=8, epochs=1, mini_batch_size=256,
                              train_against_old_versions=False, policy_temperature=temperature,
                              mask_entropy=mask_entropy), device=gpu)
    assert L.T * L.P == 256
    step0 = L._stats().rng_step
    pol = L.ppo.torch_module(0)  # the initial policy, on the CPU
    L.collect()
    torch.cuda.synchronize()
    f = L.ppo.forward(0, L.obs[0], half=True).cpu().numpy()  # the exact 16-bit logits of the step-0 obs
    out = {"seed": L.cfg.seed, "step0": step0, "logits0": f, "pol": pol,
           "obs": L.obs[:L.T].cpu().numpy().reshape(256, -1), "masks": L.masks[:L.T].cpu().numpy().reshape(256, -1),
           "acts": L.actions.cpu().numpy().reshape(256), "logp": L.logp.cpu().numpy().reshape(256)}
    L.consume()
    L.learn()
    torch.cuda.synchronize()
    out["metrics"] = L.ppo.read_metrics()
    assert bool(torch.isfinite(L.ppo.flat()).all())
    L.close()
    return out


@pytest.fixture(scope="module")
def runs(gpu):
    return {(t, me): _run(gpu, t, me) for t, me in ((3.0, True), (1.0, True), (3.0, False))}


def test_collection_samples_at_the_temperature(runs):
    """The rollout's step-0 actions and log probs equal the oracle sampler's on the tempered 16-bit logits of the
    step-0 obs (seed, step and row numbering as in test_learner_gpu's append tests)."""
    r = runs[(3.0, True)]
    P = r["logits0"].shape[0]
    wa, wlp = oracle.sample_actions(r["logits0"] / np.float32(3.0), r["masks"][:P], False, r["seed"], r["step0"], 0)
    np.testing.assert_array_equal(r["acts"][:P], wa)
    np.testing.assert_array_equal(r["logp"][:P].view(np.uint32), wlp.view(np.uint32))
    # and not the untempered draw
    ua, ulp = oracle.sample_actions(r["logits0"], r["masks"][:P], False, r["seed"], r["step0"], 0)
    assert (ulp.view(np.uint32) != wlp.view(np.uint32)).any()


def missing_temperature_kl(r, temperature):
    """The KL metric (mean(exp(lr) - 1 - lr)) Learn would report for run r's rollout if it left the temperature out:
    lr = the untempered float64 log prob of each collected action minus its tempered one, on the initial policy."""
    import copy
    import torch
    with torch.no_grad():
        logits = copy.deepcopy(r["pol"]).double()(torch.from_numpy(r["obs"]).double())
        off = -1e10 * torch.from_numpy(r["masks"]).bool().logical_not()
        ai = torch.from_numpy(r["acts"]).long().unsqueeze(-1)
        lp = [torch.softmax(z + off, -1).clamp(1e-11, 1.0).gather(-1, ai).squeeze(-1).log()
              for z in (logits, logits / temperature)]
        lr = lp[0] - lp[1]
        return float((lr.exp() - 1 - lr).mean())


def test_learn_applies_the_sampling_temperature(runs):
    """With one minibatch per iteration the KL metric compares Learn's log probs with the collection's on the same
    parameters: at T = 1 it is the bf16-inference against fp32-training gap, KL_1; at T = 3 the same gap with the
    logit errors scaled down by 3, on other sampled actions: KL_3 <= 4 KL_1 + 1e-5.  A Learn without the temperature
    would report the KL of missing_temperature_kl, which is asserted to be at least 10 x that bound.
    Measured on an MI355X: KL_1 = 1.83e-06, KL_3 = 1.98e-07 (a bound of 1.73e-05); without the temperature in Learn
    the KL would be 3.98e-02, 2300 x the bound."""
    kl3 = runs[(3.0, True)]["metrics"]["Mean KL Divergence"]
    kl1 = runs[(1.0, True)]["metrics"]["Mean KL Divergence"]
    bound = 4 * kl1 + 1e-5
    missing = missing_temperature_kl(runs[(3.0, True)], 3.0)
    print(f"KL_1 {kl1:.3e} KL_3 {kl3:.3e} bound {bound:.3e} missing-temperature KL {missing:.3e}")
    assert np.isfinite(kl1) and np.isfinite(kl3) and kl1 >= -1e-7
    assert missing >= 10 * bound, (missing, bound)
    assert kl3 <= bound, (kl3, kl1)


def test_mask_entropy_raises_the_entropy_report(runs):
    """maskEntropy divides each row's entropy by log(its legal actions) < log(90): "Policy Entropy" is strictly
    larger than without it on the same rollout (same seed and temperature; collection does not depend on it)."""
    on, off = runs[(3.0, True)], runs[(3.0, False)]
    np.testing.assert_array_equal(on["acts"], off["acts"])
    legal = on["masks"].sum(1)
    assert (legal >= 2).all() and (legal < on["masks"].shape[1]).all()
    e_on, e_off = on["metrics"]["Policy Entropy"], off["metrics"]["Policy Entropy"]
    print(f"Policy Entropy masked {e_on:.6f} unmasked {e_off:.6f}")
    assert np.isfinite(e_on) and np.isfinite(e_off)
    assert e_on > e_off > 0


def test_rlgpu_train_policy_options(gpu, tmp_path):
    """The trainer facade accepts both fields (rlgpu_train --policy-temperature X --mask-entropy), with self-play too
    (old versions sample at the temperature; self-play keeps its versions in a checkpoint folder, so it gets one),
    and refuses a temperature of 0 by the reference's field name."""
    args = ["--arenas", "16", "--rollout", "8", "--seed", "3", "--iterations", "2"]
    opts = ["--policy-temperature", "1.5", "--mask-entropy"]
    r = subprocess.run([TRAIN, *args, "--c2-model", *opts], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([TRAIN, *args, "--self-play", "--checkpoint-folder", str(tmp_path / "ckpt"), *opts],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([TRAIN, *args, "--c2-model", "--policy-temperature", "0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0
    assert "policyTemperature" in r.stdout + r.stderr, r.stdout + r.stderr

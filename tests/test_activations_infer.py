"""SIGMOID / TANH activations and addLayerNorm = false on the inference paths (the fused kernel infer::mlp_infer and the
layer-by-layer forward_half), through the C++ Learner (LearnerConfig.activation / layer_norm) and through the trainer
facade (rlgpu_train --activation X --no-layer-norm).

KL consistency (test_learn_applies_the_collection_activation), measured on an MI355X: KL_default = 1.83e-06, a bound
of 1.73e-05; (tanh, LayerNorm) KL = 1.53e-06, and a Learn that applied LeakyReLU to that rollout would report
7.17e-02, 4100 x the bound; (sigmoid, no LayerNorm) KL = 4.92e-07 (wrong activation: 2.77e-02).  Step-0 logits
against the torch restatement in bf16: 1.5e-08 (tanh) and 0 (sigmoid) at scales 1.03 and 0.68, the bound 2.2e-02 /
1.5e-02; against the same parameters under LeakyReLU 1.07 and 0.58.
"""
import copy
import os
import subprocess

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "reinforcement-learning_amd", "rlgpu", "rlgpu_train")
ACTS = ("sigmoid", "tanh")
TORCH_CLS = {"sigmoid": "Sigmoid", "tanh": "Tanh", "leaky_relu": "LeakyReLU"}
# (layers, layer_norm, infer_fp16, rows, max_rows): odd widths (LDS zero padding) with a chunked layer path, no
# LayerNorm, fp16 with a 512-wide last hidden layer (the FULL column path), the default widths
SHAPES = [((40, 72, 130), True, False, 777, 300), ((256,), False, False, 300, 300),
          ((96, 200, 512), True, True, 129, 129), ((512, 512), True, False, 1000, 1000)]
SHAPE_IDS = ["odd-bf16", "noln-bf16", "fp16", "c2-bf16"]


def close_16bit(got, want):
    """test_forward_bf16_close_to_fp32's bound: a sanity bound on the distance, not the 16-bit contract, which
    test_infer_reference_gpu.py pins (tests/infer_reference.py: this bound passes six of its nine wrong variants)."""
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    return err <= 2e-2 * scale + 1e-3, err, scale


# ------------------------------------------------------------------ 16-bit inference
@pytest.mark.parametrize("layers,ln,fp16,n,rows", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("act", ACTS)
def test_fused_inference_matches_layer_path(gpu, monkeypatch, act, layers, ln, fp16, n, rows):
    """test_ppo.test_fused_inference_matches_layer_path's body with the new activations: logits, critic values,
    actions, log probs, deterministic actions and the mixed-version draws of infer::mlp_infer<F16, ACT> equal those
    of the layer path (RLGPU_FUSED_INFER=0: gemm_bf16 + ln_act_fwd_bf16<M, F16, ACT>) bit for bit -- both call
    mlp::act_fwd<ACT> on the same 16-bit-rounded LayerNorm output.  Then the 16-bit logits and values against the
    torch restatement in bf16, and the draws against the oracle sampler on the engine's own logits."""
    import torch
    from test_ppo import make_batch
    from rlgpu.ppo import PPO
    p = PPO(policy_layers=layers, critic_layers=layers, layer_norm=ln, max_rows=rows, seed=11, infer_fp16=fp16,
            activation=act)
    rng = np.random.default_rng(n)
    obs, masks, *_ = make_batch(rng, n)
    o, m = torch.from_numpy(obs).to(gpu), torch.from_numpy(masks).to(gpu)
    old_rows = torch.from_numpy((rng.random(n) < 0.5).astype(np.uint8)).to(gpu)
    p.set_version(p.model_slice(0) * 0.5)

    def run():
        torch.cuda.synchronize()
        res = [p.forward(0, o[:rows], half=True).cpu(), p.infer_critic(o).cpu()]
        for det in (False, True):
            a, lp = p.infer_actions(o, m, step=5, deterministic=det)
            res += [a.cpu(), lp.cpu()]
        a, lp = p.infer_actions_mixed(o, m, old_rows, step=9)
        res += [a.cpu(), lp.cpu()]
        torch.cuda.synchronize()
        return res

    fused = run()
    monkeypatch.setenv("RLGPU_FUSED_INFER", "0")
    layer = run()
    monkeypatch.delenv("RLGPU_FUSED_INFER")
    names = ["logits", "values", "actions", "logp", "argmax", "logp_det", "mixed_actions", "mixed_logp"]
    for nm, f, l in zip(names, fused, layer):
        assert torch.equal(f, l), (nm, (f != l).sum().item())
    assert (masks[np.arange(n), fused[2].numpy()] == 1).all()
    # against the torch module chain in bf16
    x = torch.from_numpy(obs)
    for mi, got in ((0, fused[0].numpy()), (1, fused[1].numpy())):
        chain = p.torch_chain(mi)
        assert TORCH_CLS[act] in {type(q).__name__ for q in chain}
        with torch.no_grad():
            want = chain.to(torch.bfloat16)(x.to(torch.bfloat16)).float().numpy()
        want = want[:rows] if mi == 0 else want.reshape(-1)
        ok, err, scale = close_16bit(got.reshape(want.shape), want)
        assert ok, (mi, err, scale)
    # the draws against the oracle on the engine's own 16-bit logits (rows beyond max_rows: in chunks)
    logits = np.concatenate([p.forward(0, o[i:i + rows], half=True).cpu().numpy() for i in range(0, n, rows)])
    for det, (a, lp) in ((False, fused[2:4]), (True, fused[4:6])):
        wa, wlp = oracle.sample_actions(logits, masks, det, p.cfg.seed, 5, 0)
        np.testing.assert_array_equal(a.numpy(), wa)
        np.testing.assert_array_equal(lp.numpy().view(np.uint32), wlp.view(np.uint32))
    p.close()


@pytest.mark.parametrize("act", ACTS)
def test_fp32_inference_sampler_vs_oracle(gpu, act):
    """infer_fp16 = 2 (useHalfPrecision = false): the fp32 training forward with the activation, then the same
    sampler -- actions and log-prob bits equal the oracle's on the engine's fp32 logits."""
    import torch
    from test_ppo import make_batch
    from rlgpu.ppo import PPO
    n = 203
    p = PPO(policy_layers=(130, 512), critic_layers=(64,), max_rows=n, seed=31, infer_fp16=2, activation=act)
    obs, masks, *_ = make_batch(np.random.default_rng(7), n)
    o, m = torch.from_numpy(obs).to(gpu), torch.from_numpy(masks).to(gpu)
    logits = p.forward(0, o).cpu().numpy()
    with torch.no_grad():
        want = p.torch_module(0)(torch.from_numpy(obs)).numpy()
    assert np.allclose(logits, want, rtol=1e-4, atol=1e-5)
    for det in (True, False):
        a, lp = p.infer_actions(o, m, step=77, deterministic=det)
        wa, wlp = oracle.sample_actions(logits, masks, det, p.cfg.seed, 77, 0)
        np.testing.assert_array_equal(a.cpu().numpy(), wa)
        np.testing.assert_array_equal(lp.cpu().numpy().view(np.uint32), wlp.view(np.uint32))
    p.close()


# ------------------------------------------------------------------ the Learner
def _run(gpu, activation, layer_norm, folder=None):
    """test_policy_options_learner._run with the model options: one collect / consume / learn of a Learner whose
    iteration is exactly one minibatch (256 rows), so the learn metrics describe the pre-update parameters."""
    import torch
    from rlgpu.learner import Learner, LearnerConfig
    cfg = dict(num_arenas=8, rollout_len=8, epochs=1, mini_batch_size=256, train_against_old_versions=False,
               activation=activation, layer_norm=layer_norm)
    L = Learner(LearnerConfig(checkpoint_folder=folder, **cfg), device=gpu)
    assert L.T * L.P == 256
    step0 = L._stats().rng_step
    pol = L.ppo.torch_module(0)  # the initial policy, on the CPU
    before = L.ppo.flat().clone()
    L.collect()
    torch.cuda.synchronize()
    f = L.ppo.forward(0, L.obs[0], half=True).cpu().numpy()  # the exact 16-bit logits of the step-0 obs
    out = {"seed": L.cfg.seed, "step0": step0, "logits0": f, "pol": pol, "obs0": L.obs[0].cpu().numpy(),
           "obs": L.obs[:L.T].cpu().numpy().reshape(256, -1), "masks": L.masks[:L.T].cpu().numpy().reshape(256, -1),
           "acts": L.actions.cpu().numpy().reshape(256), "logp": L.logp.cpu().numpy().reshape(256)}
    L.consume()
    L.learn()
    torch.cuda.synchronize()
    out["metrics"] = L.ppo.read_metrics()
    after = L.ppo.flat().clone()
    out["finite"], out["changed"] = bool(torch.isfinite(after).all()), not torch.equal(before, after)
    if folder:
        L.save()
        L2 = Learner(LearnerConfig(checkpoint_folder=folder, **cfg), device=gpu)
        out["reloaded_equal"] = torch.equal(L2.ppo.flat(), after)
        out["reloaded_modules"] = [type(q).__name__ for q in L2.ppo.torch_module(0)]
        L2.close()
    L.close()
    return out


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("act_ckpt")
    return {("tanh", True): _run(gpu, "tanh", True, str(d / "tanh")),
            ("sigmoid", False): _run(gpu, "sigmoid", False, str(d / "sigmoid")),
            ("leaky_relu", True): _run(gpu, "leaky_relu", True)}


def with_leaky(pol):
    """pol's parameters under LeakyReLU(0.01): what an engine that ignored the activation would compute."""
    import torch
    return torch.nn.Sequential(*[torch.nn.LeakyReLU(0.01) if type(q).__name__ in ("Sigmoid", "Tanh") else q
                                 for q in copy.deepcopy(pol)])


@pytest.mark.parametrize("key", [("tanh", True), ("sigmoid", False)], ids=["tanh-ln", "sigmoid-noln"])
def test_collection_runs_the_activation(runs, key):
    """Step 0 of the rollout: actions and log probs equal the oracle sampler's on the engine's 16-bit logits of
    obs[0]; those logits are the torch restatement's (L.ppo.torch_module(0) holds the configured modules) in bf16
    within the 16-bit bound, and for the tanh run farther than that bound from the same parameters under LeakyReLU."""
    import torch
    r = runs[key]
    P = r["logits0"].shape[0]
    wa, wlp = oracle.sample_actions(r["logits0"], r["masks"][:P], False, r["seed"], r["step0"], 0)
    np.testing.assert_array_equal(r["acts"][:P], wa)
    np.testing.assert_array_equal(r["logp"][:P].view(np.uint32), wlp.view(np.uint32))
    kinds = [type(q).__name__ for q in r["pol"]]
    assert TORCH_CLS[key[0]] in kinds and ("LayerNorm" in kinds) == key[1] and "LeakyReLU" not in kinds
    x = torch.from_numpy(r["obs0"]).to(torch.bfloat16)
    with torch.no_grad():
        want = copy.deepcopy(r["pol"]).to(torch.bfloat16)(x).float().numpy()
        leaky = with_leaky(r["pol"]).to(torch.bfloat16)(x).float().numpy()
    ok, err, scale = close_16bit(r["logits0"], want)
    assert ok, (err, scale)
    far, err_l, scale_l = close_16bit(r["logits0"], leaky)
    print(f"{key}: |engine - torch bf16| {err:.3e} (scale {scale:.3e}); against LeakyReLU {err_l:.3e}")
    if key[0] == "tanh":
        assert not far, (err_l, scale_l)


def wrong_activation_kl(r):
    """The KL metric (mean(exp(lr) - 1 - lr)) Learn would report for run r's rollout if it applied LeakyReLU: lr =
    the float64 log prob of each collected action under LeakyReLU minus its log prob under the run's activation,
    on the initial policy."""
    import torch
    with torch.no_grad():
        x = torch.from_numpy(r["obs"]).double()
        off = -1e10 * torch.from_numpy(r["masks"]).bool().logical_not()
        ai = torch.from_numpy(r["acts"]).long().unsqueeze(-1)
        lp = [torch.softmax(mod.double()(x) + off, -1).clamp(1e-11, 1.0).gather(-1, ai).squeeze(-1).log()
              for mod in (with_leaky(r["pol"]), copy.deepcopy(r["pol"]))]
        lr = lp[0] - lp[1]
        return float((lr.exp() - 1 - lr).mean())


def test_learn_applies_the_collection_activation(runs):
    """With one minibatch per iteration the KL metric compares Learn's log probs (fp32 training kernels) with the
    collection's (16-bit inference kernels) on the same parameters: it is the 16-bit against fp32 gap, as in the
    default-activation run of the same test, KL_default -- within 4 KL_default + 1e-5 (the form and margin of
    test_learn_applies_the_sampling_temperature).  A Learn that ran LeakyReLU on the tanh rollout would report
    wrong_activation_kl, asserted to be at least 10 x that bound."""
    kl0 = runs[("leaky_relu", True)]["metrics"]["Mean KL Divergence"]
    bound = 4 * kl0 + 1e-5
    assert np.isfinite(kl0) and kl0 >= -1e-7
    for key in (("tanh", True), ("sigmoid", False)):
        kl = runs[key]["metrics"]["Mean KL Divergence"]
        wrong = wrong_activation_kl(runs[key])
        print(f"{key}: KL_default {kl0:.3e} bound {bound:.3e} KL {kl:.3e} wrong-activation KL {wrong:.3e}")
        assert np.isfinite(kl) and kl >= -1e-7
        if key[0] == "tanh":
            assert wrong >= 10 * bound, (wrong, bound)
        assert kl <= bound, (key, kl, kl0)


@pytest.mark.parametrize("key", [("tanh", True), ("sigmoid", False)], ids=["tanh-ln", "sigmoid-noln"])
def test_learner_updates_and_checkpoints(runs, key):
    """The update leaves finite, changed parameters; a second Learner on the checkpoint folder loads them bit for
    bit, and its torch restatement holds the configured modules."""
    r = runs[key]
    assert r["finite"] and r["changed"]
    assert r["reloaded_equal"]
    kinds = r["reloaded_modules"]
    assert TORCH_CLS[key[0]] in kinds and "LeakyReLU" not in kinds and ("LayerNorm" in kinds) == key[1]


# ------------------------------------------------------------------ the trainer
def _newest(base):
    dirs = sorted(int(d) for d in os.listdir(base) if d.isdigit())
    assert dirs, os.listdir(base)
    return os.path.join(base, str(dirs[-1]))


def test_rlgpu_train_activation_options(gpu, tmp_path):
    """rlgpu_train --activation sigmoid --no-layer-norm trains; with self-play and a checkpoint folder its POLICY.lt
    holds two tensors per Linear and no LayerNorm tensors, and --resave-to reproduces every model's parameters bit
    for bit (the facade's model-save / model-load pass the setting); an unknown activation is refused by the
    reference's field name."""
    import torch
    from rlgpu import checkpoint as ck
    args = ["--arenas", "16", "--rollout", "8", "--seed", "3", "--iterations", "2", "--c2-model"]
    opts = ["--activation", "sigmoid", "--no-layer-norm"]
    r = subprocess.run([TRAIN, *args, *opts], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    a, b = tmp_path / "a", tmp_path / "b"
    r = subprocess.run([TRAIN, *args, *opts, "--self-play", "--checkpoint-folder", str(a)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    fa = _newest(a)
    state = ck.read_model_state(os.path.join(fa, "POLICY.lt"))
    assert [tuple(t.shape) for t in state] == [(512, 167), (512,), (512, 512), (512,), (90, 512), (90,)]
    r = subprocess.run([TRAIN, *args, *opts, "--self-play", "--checkpoint-folder", str(a), "--resave-to", str(b)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    fb = _newest(b)
    for f in ("POLICY.lt", "CRITIC.lt"):
        x = torch.cat([t.reshape(-1) for t in ck.read_model_state(os.path.join(fa, f))])
        y = torch.cat([t.reshape(-1) for t in ck.read_model_state(os.path.join(fb, f))])
        assert x.numel() > 0 and torch.equal(x, y), f
    r = subprocess.run([TRAIN, *args, "--activation", "swish"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "activationType" in r.stdout + r.stderr, r.stdout + r.stderr

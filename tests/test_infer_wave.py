"""The one-wave form of the fused inference kernel (infer::mlp_infer_wave, 16 rows per 64-thread workgroup: the
forward the collection loop runs inside the env workgroups) against the 8-wave kernel behind
rlgpu_ppo_infer_actions_rows / rlgpu_ppo_forward's 16-bit precision: the same per-row arithmetic, so the actions,
the log probs and the f32 outputs are compared byte for byte.  Row counts: a single row, an exact 16-row tile, a
ragged tile and several workgroups."""
import numpy as np
import pytest

ROWS = (1, 16, 17, 40)
MODELS = {
    "c2": dict(policy_layers=(512, 512), critic_layers=(512, 512)),                          # 167 -> 512 -> 512 -> 90
    "small_no_ln": dict(policy_layers=(64,), critic_layers=(64,), layer_norm=False),          # 167 -> 64 -> 90
}


def make_inputs(n, gpu, seed):
    import torch
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((n, 167)).astype(np.float32)
    masks = (rng.random((n, 90)) < 0.4).astype(np.uint8)
    masks[np.arange(n), rng.integers(0, 90, n)] = 1  # at least one legal action per row
    old = (rng.random(n) < 0.5).astype(np.uint8)
    return torch.from_numpy(obs).to(gpu), torch.from_numpy(masks).to(gpu), torch.from_numpy(old).to(gpu)


def blank(n, gpu):
    import torch
    return torch.full((n,), -1, dtype=torch.int32, device=gpu), torch.full((n,), float("nan"), device=gpu)


def wave_vs_fused(gpu, model, temp, random_ln):
    """random_ln: every LayerNorm weight and bias drawn by infer_reference.randomise_layer_norm instead of the initial
    1 / 0 (the one-wave kernel reads them from the 16-bit parameter copy, the 8-wave kernel from its LDS copy)."""
    import torch
    from rlgpu.ppo import PPO
    p = PPO(max_rows=64, seed=5, policy_temperature=temp, **MODELS[model])
    if random_ln:
        from infer_reference import randomise_layer_norm
        randomise_layer_norm(p, 77)
    assert p.wave_infer_ok(0) and p.wave_infer_ok(1)
    p.set_version(p.model_slice(0) * 0.5)
    for n in ROWS:
        obs, masks, old = make_inputs(n, gpu, 100 + n)
        for det in (False, True):
            for old_rows in (None, old):
                wa, wl = blank(n, gpu)
                p.infer_actions_rows(obs, masks, row0=37, step=11, deterministic=det, old_rows=old_rows, actions=wa, logp=wl)
                a, lp = blank(n, gpu)
                p.infer_actions_wave(obs, masks, row0=37, step=11, deterministic=det, old_rows=old_rows, actions=a, logp=lp)
                assert (wa >= 0).all()
                assert bool((masks.gather(1, a.long().unsqueeze(1)) == 1).all()), "sampled a masked action"
                assert torch.equal(a, wa), (model, n, det, (a != wa).sum().item())
                assert torch.equal(lp.view(torch.int32), wl.view(torch.int32)), (model, n, det)
        for m in (0, 1):  # the f32-output mode: the 16-bit-rounded output Linear
            want = p.forward(m, obs, half=True)
            got = p.infer_values_wave(m, obs)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (model, n, m)
        if n > 1:  # another row0 draws other uniforms: the row number reaches the sampler
            a2, _ = p.infer_actions_wave(obs, masks, row0=38, step=11)
            w2, _ = p.infer_actions_rows(obs, masks, row0=38, step=11)
            assert torch.equal(a2, w2)


@pytest.mark.gpu
@pytest.mark.parametrize("temp", (1.0, 0.7))
@pytest.mark.parametrize("model", sorted(MODELS))
def test_wave_matches_fused_kernel(gpu, model, temp):
    wave_vs_fused(gpu, model, temp, random_ln=False)


@pytest.mark.gpu
@pytest.mark.parametrize("temp", (1.0, 0.7))
def test_wave_matches_fused_kernel_random_layer_norm(gpu, temp):
    """The same body with randomised LayerNorm parameters (the model that has a LayerNorm)."""
    wave_vs_fused(gpu, "c2", temp, random_ln=True)


@pytest.mark.gpu
def test_wave_fp16(gpu):
    """fp16 inference (infer_fp16) runs the other instance of both kernels."""
    import torch
    from rlgpu.ppo import PPO
    p = PPO(max_rows=64, seed=6, infer_fp16=True, policy_layers=(96, 40), critic_layers=(32,))
    obs, masks, _ = make_inputs(23, gpu, 9)
    wa, wl = p.infer_actions_rows(obs, masks, row0=3, step=2)
    a, lp = p.infer_actions_wave(obs, masks, row0=3, step=2)
    assert torch.equal(a, wa) and torch.equal(lp.view(torch.int32), wl.view(torch.int32))
    assert torch.equal(p.infer_values_wave(1, obs).view(torch.int32), p.forward(1, obs, half=True).view(torch.int32))


@pytest.mark.gpu
def test_wave_refuses_sigmoid(gpu):
    from rlgpu import _lib
    from rlgpu.ppo import PPO
    p = PPO(max_rows=64, seed=7, policy_layers=(64,), critic_layers=(64,), activation="sigmoid")
    assert not p.wave_infer_ok(0)
    obs, masks, _ = make_inputs(4, gpu, 1)
    with pytest.raises(_lib.RLGPUError, match="not eligible"):
        p.infer_actions_wave(obs, masks)
    with pytest.raises(_lib.RLGPUError, match="not eligible"):
        p.infer_values_wave(1, obs)

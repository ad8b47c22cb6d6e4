"""PPO actor/critic (include/rlgpu_ppo.h) against a plain PyTorch fp32 restatement of the
reference's libtorch code (GigaLearnCPP PPOLearner.cpp:78-184 and :341-529, Models.cpp:7-69).

libtorch itself is not vendored and unpinned -> this CPU torch restatement is the
checker; tolerances are written per test: fp32 training path rtol 1e-4 (summation order of the
MFMA GEMMs differs from torch's), bf16 inference path 2e-2 of the output scale against the fp32
forward.  The 16-bit forward's own contract is not that bound: tests/infer_reference.py restates its
rounding points in float64 and test_infer_reference_gpu.py holds every 16-bit entry point to its two
rules (the share of outputs not bit-equal to the reference, and max |got - ref|, each within 4 x what
a change of summation order alone costs).
"""
import math

import numpy as np
import pytest

from rlgpu.ppo import param_count


# ------------------------------------------------------------------ CPU: known answers
def test_param_count_known_answers():
    """run_out.log:36-39: shared head [384,384] / policy [384]x3 / critic [384]x3."""
    assert param_count(167, 0, [384, 384], out=0) == 213_888
    assert param_count(384, 90, [384, 384, 384]) == 480_474
    assert param_count(384, 1, [384, 384, 384], out=1) == 446_209


def test_param_count_c2():
    a = param_count(167, 90, [512, 512])
    c = param_count(167, 1, [512, 512], out=1)
    assert (a, c, a + c) == (396_890, 351_233, 748_123)


# ------------------------------------------------------------------ torch reference
def torch_models(ppo):
    return ppo.torch_module(0), ppo.torch_module(1)


def ref_minibatch(pol, crit, obs, masks, acts, old_logp, adv, target, batch_size, clip=0.2, ent_scale=0.035,
                  shared=None):
    """PPOLearner::Learn minibatch body (PPOLearner.cpp:341-475), fp32 torch; shared: the shared head both models
    read (:395-398 one shared forward per minibatch, :403/:474 both heads read it, :498 one backward)."""
    import torch
    n = obs.shape[0]
    bsr = n / float(batch_size)
    if shared is not None:
        obs = shared(obs)
    logits = pol(obs)
    logits = logits + -1e10 * masks.bool().logical_not()
    probs = torch.softmax(logits, -1).clamp(1e-11, 1.0)
    logp = probs.gather(-1, acts.long().unsqueeze(-1)).squeeze(-1).log()
    ent = -(probs.log() * probs).sum(-1) / math.log(probs.shape[1])
    ent = ent.mean()
    ratio = (logp - old_logp).exp()
    clipped = ratio.clamp(1 - clip, 1 + clip)
    pl = -torch.min(ratio * adv, clipped * adv).mean()
    ppo_loss = (pl - ent * ent_scale) * bsr
    vals = crit(obs).flatten()
    closs = torch.nn.functional.mse_loss(vals, target) * bsr
    (ppo_loss + closs).backward()
    return {"entropy": ent.item(), "policy_loss": pl.item(), "critic_loss": closs.item(),
            "ratio": ratio.mean().item()}


def assert_grads_close(got, *mods, rel_tol=5e-3, frac=0.0):
    """Per parameter tensor: relative Frobenius error < rel_tol and >= frac of the elements within
    1e-3 rel + 1e-4 of the tensor's max.  With the 0.01 LeakyReLU slope a pre-activation within
    rounding of 0 takes the other slope on one side (~0.5 such units expected per 600k) -- a
    discrete, legitimate difference confined to one row of a weight; the kink-free variant
    (slope 1) is held to rel 1e-4 / all elements.)"""
    o = 0
    for m in mods:
        for name, prm in m.named_parameters():
            g = got[o:o + prm.numel()].view_as(prm)
            w = prm.grad
            o += prm.numel()
            rel = ((g - w).norm() / (w.norm() + 1e-30)).item()
            ok = ((g - w).abs() <= 1e-3 * w.abs() + 1e-4 * w.abs().max()).float().mean().item()
            assert rel < rel_tol and ok >= frac, f"{name}: rel {rel:.2e}, within-tol fraction {ok:.5f}"


def flat_grads(*mods):
    import torch
    return torch.cat([p.grad.reshape(-1) for m in mods for p in m.parameters()])


def make_batch(rng, n, obs_size=167, A=90):
    obs = rng.standard_normal((n, obs_size)).astype(np.float32)
    masks = (rng.random((n, A)) < 0.6).astype(np.uint8)
    masks[:, 0] = 1
    acts = np.array([rng.choice(np.nonzero(m)[0]) for m in masks], np.int32)
    old = (np.log(1 / 40.0) + 0.3 * rng.standard_normal(n)).astype(np.float32)
    adv = rng.standard_normal(n).astype(np.float32)
    tgt = rng.standard_normal(n).astype(np.float32)
    return obs, masks, acts, old, adv, tgt


@pytest.mark.gpu
def test_forward_fp32_matches_torch(gpu):
    import torch
    from rlgpu.ppo import PPO
    p = PPO(max_rows=2048, seed=3)
    pol, crit = torch_models(p)
    x = torch.randn(1000, 167)
    for m, ref in ((0, pol), (1, crit)):
        got = p.forward(m, x.to(gpu)).cpu()
        want = ref(x).detach()
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
def test_forward_bf16_close_to_fp32(gpu):
    """The 16-bit forward against the fp32 one (and torch's bf16 chain) within 2e-2 of the output scale: how far 16-bit
    inference is from fp32, a different statement from the 16-bit contract itself, which test_infer_reference_gpu.py
    pins (this bound would pass a wrong LayerNorm variance, eps or rounding point: test_infer_reference.py)."""
    import torch
    from rlgpu.ppo import PPO
    p = PPO(max_rows=4096, seed=5)
    pol, crit = torch_models(p)
    x = torch.randn(3000, 167)
    for m, ref in ((0, pol), (1, crit)):
        got = p.forward(m, x.to(gpu), half=True).cpu().numpy()
        want = ref(x).detach().numpy()
        scale = np.abs(want).max()
        assert np.abs(got - want).max() <= 2e-2 * scale + 1e-3, (m, np.abs(got - want).max(), scale)
        want_h = ref.to(torch.bfloat16)(x.to(torch.bfloat16)).float().detach().numpy()
        assert np.abs(got - want_h).max() <= 2e-2 * scale + 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["x6", "f32", "h3"])
@pytest.mark.parametrize("n,batch,slope", [(300, 600, 0.01), (1029, 1029, 0.01), (777, 1000, 1.0)])
def test_minibatch_grads_match_torch(gpu, n, batch, slope, mode):
    import torch
    from rlgpu.ppo import PPO
    rng = np.random.default_rng(n)
    p = PPO(max_rows=2048, seed=7, leaky_slope=slope, train_gemm=mode)
    pol, crit = torch_models(p)
    obs, masks, acts, old, adv, tgt = make_batch(rng, n)
    T = lambda a: torch.from_numpy(a)  # noqa: E731
    advn = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    ref = ref_minibatch(pol, crit, T(obs), T(masks), T(acts), T(old), T(advn.astype(np.float32)), T(tgt), batch)
    d = {k: T(v).to(gpu) for k, v in dict(obs=obs, masks=masks, acts=acts, old=old, adv=adv, tgt=tgt).items()}
    p.adv_normalizer(d["adv"])
    p.zero_grad()
    p.minibatch(d["obs"], d["masks"], d["acts"], d["old"], d["adv"], d["tgt"], None, 0, n, batch)
    got = p.flat(grads=True).cpu()
    if slope == 1.0:
        assert_grads_close(got, pol, crit, rel_tol=1e-4, frac=1.0)
    else:
        assert_grads_close(got, pol, crit)
    rep = p.read_metrics()
    assert abs(rep["Policy Entropy"] - ref["entropy"]) < 1e-4
    assert abs(rep["Policy Loss"] - ref["policy_loss"]) < 1e-4 * max(1, abs(ref["policy_loss"]))
    assert abs(rep["Critic Loss"] - ref["critic_loss"]) < 1e-4 * max(1, abs(ref["critic_loss"]))


@pytest.mark.gpu
def test_minibatch_gather_and_accumulation(gpu):
    """Two minibatches through a permutation index accumulate the same gradient as one."""
    import torch
    from rlgpu.ppo import PPO, permutation
    rng = np.random.default_rng(11)
    n = 512
    obs, masks, acts, old, adv, tgt = make_batch(rng, n)
    d = {k: torch.from_numpy(v).to(gpu) for k, v in dict(obs=obs, masks=masks, acts=acts, old=old, adv=adv,
                                                              tgt=tgt).items()}
    p = PPO(max_rows=1024, seed=9)
    p.adv_normalizer(d["adv"])
    idx = permutation(n, 5, 0)
    assert torch.equal(torch.sort(idx.long()).values.cpu(), torch.arange(n))
    p.zero_grad()
    p.minibatch(d["obs"], d["masks"], d["acts"], d["old"], d["adv"], d["tgt"], idx, 0, 256, n)
    p.minibatch(d["obs"], d["masks"], d["acts"], d["old"], d["adv"], d["tgt"], idx, 256, 256, n)
    g2 = p.grads.clone()
    p.zero_grad()
    p.minibatch(d["obs"], d["masks"], d["acts"], d["old"], d["adv"], d["tgt"], None, 0, n, n)
    g1 = p.grads.clone()
    rel = ((g1 - g2).norm() / g1.norm()).item()
    assert rel < 1e-4, rel


@pytest.mark.gpu
def test_optimizer_step_matches_torch_adamw(gpu):
    import torch
    from rlgpu.ppo import PPO
    rng = np.random.default_rng(13)
    p = PPO(max_rows=1024, seed=15, policy_lr=1e-3, critic_lr=5e-4)
    pol, crit = torch_models(p)
    opts = [torch.optim.AdamW(pol.parameters(), lr=1e-3), torch.optim.AdamW(crit.parameters(), lr=5e-4)]
    for it in range(3):
        obs, masks, acts, old, adv, tgt = make_batch(rng, 400)
        T = lambda a: torch.from_numpy(a)  # noqa: E731
        advn = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
        for o in opts:
            o.zero_grad(set_to_none=True)
        ref_minibatch(pol, crit, T(obs), T(masks), T(acts), T(old), T(advn.astype(np.float32)), T(tgt), 400)
        torch.nn.utils.clip_grad_norm_(pol.parameters(), 0.5)
        torch.nn.utils.clip_grad_norm_(crit.parameters(), 0.5)
        for o in opts:
            o.step()
        d = [torch.from_numpy(v).to(gpu) for v in (obs, masks, acts, old, adv, tgt)]
        p.adv_normalizer(d[4])
        p.minibatch(*d, None, 0, 400, 400)
        p.optimizer_step()
    want = torch.cat([q.detach().reshape(-1) for m in (pol, crit) for q in m.parameters()])
    got = p.flat().cpu()
    # Adam divides by sqrt(v): coordinates whose gradient is ~0 get an update of O(lr) whose sign
    # follows rounding noise, so a handful may differ by a fraction of lr; all others agree tightly.
    diff = np.abs(got.numpy() - want.numpy())
    tight = diff <= 1e-4 * np.abs(want.numpy()) + 2e-6
    assert tight.mean() > 0.9999, tight.mean()
    assert diff.max() < 0.1 * 1e-3, diff.max()
    assert float(p.grads.abs().max()) == 0.0  # zero_grad after the step


@pytest.mark.gpu
def test_infer_actions_respect_masks_and_distribution(gpu):
    import torch
    from rlgpu.ppo import PPO
    p = PPO(max_rows=8192, seed=17)
    rng = np.random.default_rng(3)
    obs, masks, *_ = make_batch(rng, 4096)
    o, m = torch.from_numpy(obs).to(gpu), torch.from_numpy(masks).to(gpu)
    a, lp = p.infer_actions(o, m, step=1)
    a = a.cpu().numpy()
    assert (masks[np.arange(4096), a] == 1).all()
    logits = p.forward(0, o, half=True).cpu()
    probs = torch.softmax(logits + -1e10 * torch.from_numpy(masks == 0), -1).clamp(1e-11, 1).numpy()
    np.testing.assert_allclose(lp.cpu().numpy(), np.log(probs[np.arange(4096), a]), rtol=1e-3, atol=1e-4)
    ad, _ = p.infer_actions(o, m, deterministic=True)
    np.testing.assert_array_equal(ad.cpu().numpy(), probs.argmax(1))
    # one row sampled many times: empirical frequencies ~ probs
    row = np.repeat(obs[:1], 8192, 0)
    rm = np.repeat(masks[:1], 8192, 0)
    counts = np.zeros(90)
    for s in range(4):
        aa, _ = p.infer_actions(torch.from_numpy(row).to(gpu), torch.from_numpy(rm).to(gpu), step=100 + s)
        counts += np.bincount(aa.cpu().numpy(), minlength=90)
    freq = counts / counts.sum()
    pr = probs[0] / probs[0].sum()
    assert np.abs(freq - pr).max() < 0.02


FUSED_SHAPES = [((512, 512), True, False, 16384 + 37, 16384 + 37),
                ((512, 512), True, True, 1000, 1000),
                ((40, 72, 130), True, False, 777, 300),
                ((256,), False, False, 300, 300),
                ((96, 200, 512), True, True, 129, 129)]


def fused_vs_layer_path(gpu, monkeypatch, layers, ln, fp16, n, rows, random_ln):
    """infer::mlp_infer (one launch per forward) against the layer-by-layer path forward_half ->
    sample_actions (RLGPU_FUSED_INFER=0): the same MFMA instruction over the same K order, the same
    roundings and the same sampler, so logits, critic values, actions and log probs are bit-identical
    -- for odd widths (LDS zero padding), without LayerNorm, in fp16 and bf16, for row counts off the
    64-row workgroup tile, and for the mixed-version (self-play) inference.  With n > max_rows the
    layer path works in max_rows chunks and the fused critic in one launch.  random_ln: every LayerNorm weight and
    bias drawn by infer_reference.randomise_layer_norm instead of the initial 1 / 0, where a wrong column map of
    gamma / beta common to both paths would be invisible (the old version then differs in them too)."""
    import torch
    from rlgpu.ppo import PPO
    p = PPO(policy_layers=layers, critic_layers=layers, layer_norm=ln, max_rows=rows, seed=11, infer_fp16=fp16)
    if random_ln:
        from infer_reference import randomise_layer_norm
        randomise_layer_norm(p, n)
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
    names = ["logits", "values", "actions", "logp", "argmax", "logp_det", "mixed_actions", "mixed_logp"]
    for nm, f, l in zip(names, fused, layer):
        assert torch.equal(f, l), (nm, (f != l).sum().item())
    assert (masks[np.arange(n), fused[2].numpy()] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("layers,ln,fp16,n,rows", FUSED_SHAPES)
def test_fused_inference_matches_layer_path(gpu, monkeypatch, layers, ln, fp16, n, rows):
    """fused_vs_layer_path at the initial parameters (LayerNorm weight 1, bias 0)."""
    fused_vs_layer_path(gpu, monkeypatch, layers, ln, fp16, n, rows, random_ln=False)


@pytest.mark.gpu
@pytest.mark.parametrize("layers,ln,fp16,n,rows", [s for s in FUSED_SHAPES if s[1]])
def test_fused_inference_matches_layer_path_random_layer_norm(gpu, monkeypatch, layers, ln, fp16, n, rows):
    """The same body with randomised LayerNorm parameters (the shapes that have a LayerNorm)."""
    fused_vs_layer_path(gpu, monkeypatch, layers, ln, fp16, n, rows, random_ln=True)


@pytest.mark.gpu
def test_infer_actions_rows_matches_whole_call(gpu, monkeypatch):
    """rlgpu_ppo_infer_actions_rows (the collection in arena groups; not bound in rlgpu.ppo) over the row blocks
    [0, 77) and [77, 200) of a 200-row step -- off the fused kernel's 64-row tile -- draws the actions and log
    probs of one rlgpu_ppo_infer_actions call over the 200 rows (d_old_rows NULL), and with the matching slices
    of old_rows those of one rlgpu_ppo_infer_actions_mixed call, bit for bit: the sampler's rows are global
    (row0).  Off the fused kernel (RLGPU_FUSED_INFER=0) it is refused with RLGPU_ERR_UNSUPPORTED."""
    import ctypes
    import torch
    from rlgpu import _lib
    from rlgpu.ppo import PPO
    n, cut = 200, 77
    p = PPO(policy_layers=(40, 72), max_rows=n, seed=23)
    L = _lib.lib()
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    L.rlgpu_ppo_infer_actions_rows.argtypes = [vp, vp, vp, i32, i64, i32, u64, vp, vp, vp, vp]
    rng = np.random.default_rng(n)
    obs, masks, *_ = make_batch(rng, n)
    o, m = torch.from_numpy(obs).to(gpu), torch.from_numpy(masks).to(gpu)
    old_rows = torch.from_numpy((rng.random(n) < 0.5).astype(np.uint8)).to(gpu)
    p.set_version(p.model_slice(0) * 0.5)

    def rows(b, e, old, a, lp):
        return L.rlgpu_ppo_infer_actions_rows(p._h, _lib.ptr(o[b:e]), _lib.ptr(m[b:e]), e - b, b, 0, 7,
                                              _lib.ptr(old[b:e]) if old is not None else None, _lib.ptr(a[b:e]),
                                              _lib.ptr(lp[b:e]), _lib.stream_ptr())

    def blank():  # the old version's rows get no log prob: both sides start from the same NaN
        return torch.full((n,), -1, dtype=torch.int32, device=gpu), torch.full((n,), float("nan"), device=gpu)

    assert old_rows.any() and not old_rows.all()
    for old in (None, old_rows):
        wa, wlp = blank()
        if old is None:
            p.infer_actions(o, m, step=7, actions=wa, logp=wlp)
        else:
            p.infer_actions_mixed(o, m, old, step=7, actions=wa, logp=wlp)
        a, lp = blank()
        for b, e in ((0, cut), (cut, n)):
            _lib.check(rows(b, e, old, a, lp), "rlgpu_ppo_infer_actions_rows")
        assert (wa >= 0).all() and not torch.isnan(wlp[old_rows == 0]).any()
        assert torch.equal(a, wa), (a != wa).sum().item()
        assert torch.equal(lp.view(torch.int32), wlp.view(torch.int32))
    monkeypatch.setenv("RLGPU_FUSED_INFER", "0")
    a, lp = torch.empty(n, dtype=torch.int32, device=gpu), torch.empty(n, device=gpu)
    assert rows(0, cut, None, a, lp) == -5  # RLGPU_ERR_UNSUPPORTED
    assert "not on the fused kernel" in _lib.last_error()


@pytest.mark.gpu
def test_mean_std(gpu):
    import torch
    from rlgpu.ppo import PPO
    p = PPO(max_rows=64, seed=1)
    x = torch.randn(100_003) * 3 + 1
    st = p.adv_normalizer(x.to(gpu)).cpu().numpy()
    np.testing.assert_allclose(st, [x.mean().item(), x.std().item()], rtol=1e-5)


# ------------------------------------------------------------------ GEMM arithmetic
GEMM_SHAPES = [  # (a_layout, b_layout, I, J, K, splits): the PPO shapes' layouts, ragged edges
    (0, 0, 1029, 512, 167, 1), (0, 0, 777, 90, 512, 1), (0, 0, 300, 130, 33, 1),
    (0, 1, 1029, 167, 512, 1), (0, 1, 513, 512, 90, 1),
    (1, 1, 512, 167, 3001, 7), (1, 1, 90, 512, 2048, 4), (1, 1, 130, 200, 97, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("la,lb,I,J,K,splits", GEMM_SHAPES)
def test_gemm_modes_fp32_class_accuracy(gpu, la, lb, I, J, K, splits):
    """rlgpu_gemm in every training arithmetic against an fp64 product: the three-way bf16 split
    (RLGPU_GEMM_F32X6) and the scaled two-way fp16 split (RLGPU_GEMM_F16X3) must carry f32-class
    error -- within 4x of torch's own fp32 matmul error on the same operands (the reference's
    libtorch fp32 Linear) -- and so must the f32 MFMA."""
    import ctypes
    import torch
    from rlgpu import _lib
    from rlgpu.ppo import _bind
    L = _bind()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.rlgpu_gemm.argtypes = [i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, i32, i32, i32, i32, vp]
    g = torch.Generator().manual_seed(I * 7 + J * 3 + K)
    A = torch.randn((I, K) if la == 0 else (K, I), generator=g)
    B = torch.randn((J, K) if lb == 0 else (K, J), generator=g)
    bias = torch.randn(J, generator=g) if splits == 1 else None
    tA, tB = (A if la == 0 else A.t()), (B.t() if lb == 0 else B)
    ref = tA.double() @ tB.double() + (bias.double() if bias is not None else 0)
    scale = ref.abs().max().item()
    terr = ((tA @ tB + (bias if bias is not None else 0)).double() - ref).abs().max().item() / scale
    dA, dB = A.to(gpu), B.to(gpu)
    db = bias.to(gpu) if bias is not None else None
    for mode in (0, 1, 2):
        C = torch.full((splits, I, J), float("nan"), device=gpu)
        _lib.check(L.rlgpu_gemm(mode, la, lb, _lib.ptr(dA), A.shape[1], _lib.ptr(dB), B.shape[1], _lib.ptr(C), J,
                                _lib.ptr(db), I, J, K, splits, _lib.stream_ptr()), "rlgpu_gemm")
        got = C.sum(0).double().cpu()
        err = (got - ref).abs().max().item() / scale
        assert err <= 4 * terr + 1e-7, f"mode {mode}: rel err {err:.2e} vs torch fp32 {terr:.2e}"


def _gemm(gpu, mode, la, lb, A, B, I, J, K, splits=1, bias=None):
    import ctypes
    import torch
    from rlgpu import _lib
    from rlgpu.ppo import _bind
    L = _bind()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.rlgpu_gemm.argtypes = [i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, i32, i32, i32, i32, vp]
    dA, dB = A.to(gpu), B.to(gpu)
    db = bias.to(gpu) if bias is not None else None
    C = torch.full((splits, I, J), float("nan"), device=gpu)
    _lib.check(L.rlgpu_gemm(mode, la, lb, _lib.ptr(dA), A.shape[1], _lib.ptr(dB), B.shape[1], _lib.ptr(C), J,
                            _lib.ptr(db), I, J, K, splits, _lib.stream_ptr()), "rlgpu_gemm")
    return C.sum(0).double().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("la,lb,splits", [(0, 0, 1), (0, 1, 1), (1, 1, 3)])
def test_gemm_h3_scales(gpu, la, lb, splits):
    """RLGPU_GEMM_F16X3's power-of-two operand scales.  Tensors far outside fp16's range (1e-30,
    1e25) and rows spread over 2^+-8 (a 2^16 range inside one tensor) keep f32-class error on every
    element, normwise (|C - C64| / (|A||B|) <= 4 x torch fp32's); with rows spread over 2^+-20 the
    smallest rows sit 2^40 below the tensor's largest, under fp16's range after the per-tensor scale,
    and the error stays f32-class relative to the output's scale (max |A||B|), not per element.
    An all-zero operand gives exactly zero, and a NaN in an operand reaches the output."""
    import torch
    I, J, K = 300, 200, 257
    g = torch.Generator().manual_seed(5)
    for sa, sb, spread in ((1e-30, 1e25, 0), (1.0, 1.0, 8), (3e5, 2e-7, 8), (1.0, 1.0, 20)):
        A = torch.randn((I, K) if la == 0 else (K, I), generator=g) * sa
        B = torch.randn((J, K) if lb == 0 else (K, J), generator=g) * sb
        if spread:  # rows of A (output rows i) at scales 2^-spread .. 2^spread
            ei = torch.randint(-spread, spread + 1, (I,), generator=g).double()
            if la == 0:
                A = (A.double() * torch.pow(2.0, ei)[:, None]).float()
            else:
                A = (A.double() * torch.pow(2.0, ei)[None, :]).float()
        tA, tB = (A if la == 0 else A.t()), (B.t() if lb == 0 else B)
        ref = tA.double() @ tB.double()
        norm = tA.double().abs() @ tB.double().abs()
        if spread <= 8:
            nrm = norm
        else:
            nrm = norm.max()
        terr = ((tA @ tB).double() - ref).abs().div(nrm).max().item()
        got = _gemm(gpu, 2, la, lb, A, B, I, J, K, splits)
        err = (got - ref).abs().div(nrm).max().item()
        assert err <= 4 * terr + 1e-7, (sa, sb, spread, err, terr)
    Z = torch.zeros((I, K) if la == 0 else (K, I))
    B = torch.randn((J, K) if lb == 0 else (K, J), generator=g)
    assert (_gemm(gpu, 2, la, lb, Z, B, I, J, K, splits) == 0).all()
    A = torch.randn((I, K) if la == 0 else (K, I), generator=g)
    A[3, 5] = float("nan")
    assert torch.isnan(_gemm(gpu, 2, la, lb, A, B, I, J, K, splits)).any()


@pytest.mark.gpu
def test_forward_fp32_h3_matches_torch(gpu):
    """The training forward in RLGPU_GEMM_F16X3 against torch fp32 (rtol 1e-4), at C2 and C5 widths."""
    import torch
    from rlgpu.ppo import PPO
    x = torch.randn(700, 167)
    for layers in ((512, 512), (2048,) * 4):
        p = PPO(policy_layers=layers, critic_layers=layers, max_rows=1024, seed=3, train_gemm=2)
        pol, crit = torch_models(p)
        for m, ref in ((0, pol), (1, crit)):
            got = p.forward(m, x.to(gpu)).cpu()
            np.testing.assert_allclose(got.numpy(), ref(x).detach().numpy(), rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ BASELINE config C5 (4 x 2048, fp16 inference)
def test_param_count_c5():
    """actor + critic [2048] x 4 = 26.1 M parameters."""
    a = param_count(167, 90, [2048] * 4)
    c = param_count(167, 1, [2048] * 4, out=1)
    assert (a, c, a + c) == (13_133_914, 12_951_553, 26_085_467)


@pytest.mark.gpu
def test_c5_forward_fp32_and_fp16_inference(gpu):
    """C5 shapes: fp32 training forward vs torch fp32 (rtol 1e-4), fp16 inference copy (v_mfma_f32_32x32x16_f16)
    within 1e-2 of the output scale of fp32, and closer than the bf16 copy of the same weights.  That compares 16 bit
    with fp32; the 16-bit contract itself (its rounding points) is pinned in test_infer_reference_gpu.py."""
    import torch
    from rlgpu.ppo import PPO
    x = torch.randn(300, 167)
    p16 = PPO(policy_layers=(2048,) * 4, critic_layers=(2048,) * 4, max_rows=512, seed=5, infer_fp16=True)
    pbf = PPO(policy_layers=(2048,) * 4, critic_layers=(2048,) * 4, max_rows=512, seed=5)
    assert torch.equal(p16.params, pbf.params)
    for m in (0, 1):
        want = p16.torch_module(m)(x).detach()
        got = p16.forward(m, x.to(gpu)).cpu()
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=1e-4)
        scale = want.abs().max().item()
        e16 = (p16.forward(m, x.to(gpu), half=True).cpu() - want).abs().max().item() / scale
        ebf = (pbf.forward(m, x.to(gpu), half=True).cpu() - want).abs().max().item() / scale
        assert e16 < 1e-2 and e16 < ebf, (m, e16, ebf)


@pytest.mark.gpu
def test_c5_minibatch_grads_match_torch(gpu):
    """The full PPO minibatch at C5 shapes (kink-free slope 1.0) against the torch fp32 restatement."""
    import torch
    from rlgpu.ppo import PPO
    rng = np.random.default_rng(55)
    n = 256
    p = PPO(policy_layers=(2048,) * 4, critic_layers=(2048,) * 4, max_rows=512, seed=9, leaky_slope=1.0)
    pol, crit = torch_models(p)
    obs, masks, acts, old, adv, tgt = make_batch(rng, n)
    T = lambda a: torch.from_numpy(a)  # noqa: E731
    advn = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    ref_minibatch(pol, crit, T(obs), T(masks), T(acts), T(old), T(advn.astype(np.float32)), T(tgt), n)
    d = {k: T(v).to(gpu) for k, v in dict(obs=obs, masks=masks, acts=acts, old=old, adv=adv, tgt=tgt).items()}
    p.adv_normalizer(d["adv"])
    p.zero_grad()
    p.minibatch(d["obs"], d["masks"], d["acts"], d["old"], d["adv"], d["tgt"], None, 0, n, n)
    assert_grads_close(p.flat(grads=True).cpu(), pol, crit, rel_tol=1e-4, frac=1.0)


_QUAD_CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [sys.argv[2], sys.argv[2] + "/reinforcement-learning_amd", sys.argv[2] + "/tests"]
from rlgpu.ppo import PPO
from test_ppo import make_batch
dev = torch.device("cuda:0")
out = []
for n, layers in ((1000, (512, 512)), (3000, (256, 768, 512)), (700, (2048, 1024))):
    p = PPO(policy_layers=layers, critic_layers=layers, max_rows=4096, seed=5)
    obs, masks, acts, old, adv, tgt = make_batch(np.random.default_rng(n), n)
    d = [torch.from_numpy(v).to(dev) for v in (obs, masks, acts, old, adv, tgt)]
    p.adv_normalizer(d[4])
    p.zero_grad()
    p.minibatch(*d, None, 0, n, n)
    out += [p.flat(grads=True).cpu().numpy(), p.forward(0, d[0]).cpu().numpy().ravel()]
np.save(sys.argv[1], np.concatenate(out))
"""


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_h3_quad_tiles_bit_identical(gpu, tmp_path):
    """The 256 x 256 tile H3 GEMM (mlp::gemm_h3q: RLGPU_H3_QUAD=1 for every width that is a multiple of 256, by
    default from 1024 columns) gives the same minibatch gradients and forward outputs, bit for bit, as the
    128 x 128 gemm_x6 path (RLGPU_H3_QUAD=0): same products, same order into one
    accumulator.  Row counts off the 256-row tile, widths 256 / 512 / 768 / 1024 / 2048.  The knob is read once
    per process: child processes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for v in ("0", "1"):
        f = str(tmp_path / f"q{v}.npy")
        r = subprocess.run([sys.executable, "-c", _QUAD_CHILD, f, root], env=dict(os.environ, RLGPU_H3_QUAD=v),
                           capture_output=True, text=True, timeout=240, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res[v] = np.load(f)
    assert res["0"].shape == res["1"].shape
    np.testing.assert_array_equal(res["0"].view(np.uint32), res["1"].view(np.uint32))

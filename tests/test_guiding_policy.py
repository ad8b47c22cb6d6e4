"""PPOLearnerConfig::useGuidingPolicy: the L1 pull toward a frozen policy in the PPO minibatch loss
(rlgpu_ppo_set_guide, rlgpu_ppo_infer_guide_logits, rlgpu_ppo_minibatch_guided).

The reference (PPOLearner.cpp:458-468): guidingLoss = mean over all n A elements of |g - c| with g the guide's clamped
masked softmax of (guide logits / temperature) and c the trained policy's clamped probabilities, added to the loss as
guidingLoss * guidingStrength after the batch-size-ratio scaling.  Here the guide logits are an explicit 16-bit input
of the minibatch, so the term is checked against a float64 reference built entirely on the CPU:

  * ppo_reference.minibatch_ref with guide_logits (at strength 0 it reproduces its own gradients and metrics without
    a guide exactly, asserted here).  The GPU cases are held to ppo_reference's rules and constants unchanged
    (check_grads, check_metrics, check_forward); the guiding-loss metric is a one-element result under that module's
    scalar rule with S = mean over (row, action) of c_k (1 + |z_k| + zmax) + g_k (1 + |zg_k| + zgmax).
  * Guide logits per case: a numpy stream N(0, 1) * gscale (seed 4242 + the case's seed), rounded to bf16 with
    round-to-nearest-even (fp16 for the fp16 case), so they are exactly representable in the handle's format.
  * Side conditions, decided by the float64 reference alone: ppo_reference.side_conditions, two legal actions per
    row under mask_entropy, and the sign margin -- d |g - c| / d c = sign(c - g) is decided by float64 only where the
    gap is well above fp32's error: for every legal (row, action) either the row has a single legal action
    (c = g = 1 exactly in any precision) or |c - g| >= GUIDE_DELTA * max(c, g).  GUIDE_DELTA is 10 x the largest
    |(c32 - g32) - (c64 - g64)| / max(c64, g64) of the torch fp32 yardstick over the case table
    (test_guide_delta_covers_fp32 recomputes it and asserts that the yardstick has float64's signs everywhere).
    Measured on the CPU over the table below without the edge case: largest fp32 error 8.0e-7 (d64), smallest gap
    6.1e-5 (rows37_f16), 0 sign flips, masked columns differ by exactly 0; a2's only zero gaps are its rows with a
    single legal action.
  * The edge case (logits over about +-60, out_scale 50) needs two additions, both by the same reasoning.  Its legal
    actions under the clamp meet guide probabilities under the clamp (571 elements): there c = g = 1e-11 exactly in any
    precision -- side_conditions keeps c's raw probability 0.1 % away from the clamp, the same is asserted for g's --
    so they are exempt like the single-legal rows.  And fp32's error of c grows with |z|: the yardstick's largest error
    there is 4.4e-5, so that case's margin is EDGE_DELTA = 5e-4 (10 x, rounded up); its smallest gap is 6.0e-3.
  * test_guide_term_is_a_real_share: the issue behind this file expected the guide to move every policy tensor's
    float64 gradient by 1 % at strength 0.5.  That holds for A = 2 only: the term's logit gradient is
    strength / (n A) p_k (sign_k - sum_j p_j sign_j) against the surrogate's |adv| ratio / n (delta_ka - p_k), a share
    of about strength / A * ||p||_2.  Measured smallest share over a case's policy tensors: a2 9.4e-2, b17 7.7e-3,
    rows1 2.6e-3, d64 1.8e-3, rows37 1.4e-3, rows33 1.1e-3, rows37_f16 9.0e-4, a128 5.8e-4, edge 3.6e-4.  What the
    share has to guarantee is that a kernel without the term fails check_grads' normwise ceiling of 1e-4: the test
    asserts 1 % where A = 2 and at least 2e-4 (twice the ceiling: the engine's own error, bounded by the ceiling,
    cannot cancel it) everywhere.
"""
import numpy as np
import pytest

from ppo_reference import (MODE_IDS, MODES, Case, build_case, check_golden, check_metrics, engine_minibatch,
                           guide_stream, make_engine, one_element, run_engine_case, run_refs, side_conditions)

# loss-kernel edge rows on a default-width policy, logits spanning about +-60: test_ppo_variants' EDGE
EDGE = Case("edge", 167, 90, (512, 512), (64,), seed=20, n=64, out_scale=50.0, edge=True)
STRENGTH = 0.5      # guiding_strength of the gradient cases (the reference's default is 0.03)
GUIDE_DELTA = 2e-5  # sign margin, see the module docstring
EDGE_DELTA = 5e-4   # the edge case's (logits over about +-60)
CLAMP, CLAMP_MARGIN = 1e-11, 1e-3  # ACTION_MIN_PROB and side_conditions' 0.1 % distance from it
M_GUIDE = 10        # RLGPU_M_GUIDING_LOSS


# ------------------------------------------------------------------ the cases
class GuideCase:
    def __init__(self, case, temperature, mask_entropy, gscale, fp16=False, delta=GUIDE_DELTA):
        self.case, self.temperature, self.mask_entropy, self.gscale, self.fp16 = case, temperature, mask_entropy, gscale, fp16
        self.delta = delta


_ROWS = dict(obs=167, A=90, pol=(96, 33), crit=(40, 64), seed=0)
GUIDE_CASES = {
    # loss<6>, ldd 90 -> 92; two 32-row blocks with a ragged tail; temperature and mask_entropy
    "rows37": GuideCase(Case("rows37", n=37, **_ROWS), 2.5, True, 1.0),
    # the 1-row and 33-row block edges
    "rows1": GuideCase(Case("rows1", n=1, **_ROWS), 0.7, True, 8.0),
    "rows33": GuideCase(Case("rows33", n=33, **_ROWS), 2.5, True, 8.0),
    # loss<2>, ldd 17 -> 20; T < 1
    "b17": GuideCase(Case("b17", 168, 17, (64, 128), (65, 33), seed=1), 0.7, False, 1.0),
    # loss<8>, ldd 128 unpadded
    "a128": GuideCase(Case("a128", 168, 128, (130, 64), (65, 128), seed=0), 3.0, True, 1.0),
    # loss<1>, ldd 2 -> 4: rows with one legal action, whose differences are exactly 0
    "a2": GuideCase(Case("a2", 167, 2, (33, 65), (130, 64), seed=0), 1.0, False, 8.0),
    # loss<4>, ldd 64; T = 1 and no options: the guide alone
    "d64": GuideCase(Case("d64", 168, 64, (256, 257), (128, 65), seed=0), 1.0, False, 1.0),
    # the loss kernel's edge rows (single-legal rows, stored action masked, logits over about +-60)
    "edge": GuideCase(EDGE, 1.0, False, 8.0, delta=EDGE_DELTA),
    # the fp16 inference format: guide logits rounded to fp16, an fp16 handle
    "rows37_f16": GuideCase(Case("rows37", n=37, **_ROWS), 2.5, True, 8.0, fp16=True),
}
# 256 blocks of the loss kernel with a one-row last block: the metric reduction over many blocks (slope 1.0)
MANY = GuideCase(Case("rows8161", 167, 90, (64, 36), (64, 36), seed=0, slope=1.0, n=8161, extra=100), 1.5, True, 1.0)


def guide_data(name):
    g = MANY if name == "rows8161" else GUIDE_CASES[name]
    d = build_case(g.case, temperature=g.temperature, mask_entropy=g.mask_entropy, guide=(g.gscale, g.fp16, STRENGTH))
    return dict(d, g=g)


def sign_margin(r64, masks, delta=GUIDE_DELTA):
    """(violations, smallest relative gap) of the sign margin over the legal (row, action) pairs, without those where
    c = g exactly in any precision: rows with one legal action (1 = 1) and elements whose raw probabilities are both
    under the clamp (1e-11 = 1e-11)."""
    legal = np.asarray(masks, bool)
    c, g = r64["probs"].numpy(), r64["gprobs"].numpy()
    both = (r64["raw_probs"].numpy() < CLAMP * (1 - CLAMP_MARGIN)) & (r64["graw"].numpy() < CLAMP * (1 - CLAMP_MARGIN))
    assert (c[legal & both] == g[legal & both]).all()
    sel = legal & (legal.sum(1, keepdims=True) > 1) & ~both
    if not sel.any():
        return 0, float("inf")
    gap = np.abs(c - g)[sel] / np.maximum(c, g)[sel]
    return int((gap < delta).sum()), float(gap.min())


def assert_guide_side_conditions(d):
    import torch
    c, g = d["case"], d["g"]
    masks = d["batch"]["masks"][d["rows"]]
    why = side_conditions(c, d["r64"], torch.from_numpy(masks))
    assert why is None, f"case {c.name}: {why}"
    if g.mask_entropy:
        assert masks.sum(1).min() >= 2, f"case {c.name}: a row with one legal action under mask_entropy"
    near = int(((np.abs(d["r64"]["graw"].numpy() / CLAMP - 1) < CLAMP_MARGIN) & np.asarray(masks, bool)).sum())
    assert near == 0, f"case {c.name}: {near} legal guide probabilities within 0.1 % of the clamp"
    bad, small = sign_margin(d["r64"], masks, g.delta)
    assert bad == 0, f"case {c.name}: {bad} legal elements inside the sign margin (smallest relative gap {small:.2e})"
    # masked columns: both sides are the clamp, the difference is exactly 0
    off = ~np.asarray(masks, bool)
    assert (d["r64"]["probs"].numpy()[off] == d["r64"]["gprobs"].numpy()[off]).all()
    one = masks.sum(1) == 1
    assert (d["r64"]["probs"].numpy()[one] == d["r64"]["gprobs"].numpy()[one]).all()  # c = g = 1 / 1e-11 exactly
    assert np.isfinite(d["r64"]["metrics"]).all() and bool(d["r64"]["grads"].isfinite().all())
    assert np.isfinite(d["r64"]["guiding"]) and d["r64"]["guiding"] > 0


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("name", list(GUIDE_CASES) + ["rows8161"])
def test_reference_matches_golden(name):
    """The float64 reference of every guided case against tests/golden/ppo_reference.npz (ppo_reference.check_golden)."""
    check_golden(f"guide/{name}", guide_data(name))


def test_guide_reference_reduces():
    """minibatch_ref with a guide at strength 0 gives its gradients, six metrics and scales without a guide exactly, in
    float64 and in fp32, with and without the options: the guide branch does not perturb the rest."""
    import torch
    for name in ("b17", "rows37", "d64"):
        d = guide_data(name)
        options = dict(temperature=d["temperature"], mask_entropy=d["mask_entropy"])
        wants = run_refs(d["case"], d["mods"], d["batch"], **options)
        gots = run_refs(d["case"], d["mods"], d["batch"], guide_logits=d["gvals"], strength=0.0, **options)
        for want, got in zip(wants, gots):
            assert torch.equal(got["grads"], want["grads"])
            for k in ("metrics", "scales"):
                np.testing.assert_array_equal(got[k], want[k])
            assert got["head_bias_scale"] == want["head_bias_scale"]
            assert got["guiding"] > 0 and "guiding" not in want


def test_guide_stream_is_exact():
    """The guide logits are values of their 16-bit format: decoding the bits gives the values back, rounding them again
    changes nothing, and the bf16 rounding is to nearest even."""
    for name in ("rows37", "rows37_f16"):
        g = GUIDE_CASES[name]
        bits, vals = guide_stream(g.case, g.gscale, g.fp16)
        assert bits.dtype == np.uint16 and vals.dtype == np.float32 and bits.shape == vals.shape
        if g.fp16:
            np.testing.assert_array_equal(vals.astype(np.float16).view(np.uint16), bits)
        else:
            assert (vals.view(np.uint32) & 0xFFFF == 0).all()
    # ties go to the even mantissa: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6 (bf16 has 7 fraction bits)
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], np.float32).view(np.uint32)
    r = ((x + np.uint32(0x7FFF) + ((x >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint32) << np.uint32(16)
    np.testing.assert_array_equal(r.view(np.float32), np.array([1.0, 1 + 2.0 ** -6], np.float32))


@pytest.mark.parametrize("name", list(GUIDE_CASES) + ["rows8161"])
def test_guide_side_conditions_hold(name):
    """ppo_reference's side conditions and the sign margin (0 violating elements; rows8161 is held to the first only:
    its gradients are not checked), by the float64 reference alone."""
    import torch
    d = guide_data(name)
    if name == "rows8161":
        why = side_conditions(d["case"], d["r64"], torch.from_numpy(d["batch"]["masks"][d["rows"]]))
        assert why is None, why
        return
    assert_guide_side_conditions(d)
    if name == "a2":  # its only zero gaps are the rows with a single legal action
        masks = d["batch"]["masks"][d["rows"]]
        zero = (d["r64"]["probs"].numpy() == d["r64"]["gprobs"].numpy()) & np.asarray(masks, bool)
        assert zero.any() and (masks.sum(1)[zero.any(1)] == 1).all()
    if d["case"].edge:
        masks = d["batch"]["masks"][d["rows"]]
        assert (masks.sum(1) == 1).sum() == 8


def test_guide_delta_covers_fp32():
    """GUIDE_DELTA is at least 10 x the largest |(c32 - g32) - (c64 - g64)| / max(c64, g64) of the torch fp32 yardstick
    over the case table (the edge case: EDGE_DELTA over its own), and the yardstick's sign(c - g) is float64's on every
    element."""
    worst = {GUIDE_DELTA: 0.0, EDGE_DELTA: 0.0}
    small = {GUIDE_DELTA: float("inf"), EDGE_DELTA: float("inf")}
    for name, g in GUIDE_CASES.items():
        d = guide_data(name)
        c64, g64 = d["r64"]["probs"].numpy(), d["r64"]["gprobs"].numpy()
        c32, g32 = d["r32"]["probs"].double().numpy(), d["r32"]["gprobs"].double().numpy()
        err = np.abs((c32 - g32) - (c64 - g64)) / np.maximum(c64, g64)
        worst[g.delta] = max(worst[g.delta], float(err.max()))
        small[g.delta] = min(small[g.delta], sign_margin(d["r64"], d["batch"]["masks"][d["rows"]], g.delta)[1])
        assert (np.sign(c32 - g32) == np.sign(c64 - g64)).all(), name
    for delta in worst:
        print(f"margin {delta:.0e}: largest fp32 error of c - g {worst[delta]:.2e}, smallest relative gap {small[delta]:.2e}")
        assert 10 * worst[delta] <= delta <= small[delta], (delta, worst[delta], small[delta])


@pytest.mark.parametrize("name", list(GUIDE_CASES))
def test_guide_term_is_a_real_share(name):
    """At the tested strength (0.5) the float64 policy gradient with the guide differs from the one without it, normwise
    in every policy tensor, by at least 1 % where A = 2 and by at least 2e-4 in every case (module docstring: the 1 % does
    not hold for more actions): a kernel that ignores the guide cannot pass check_grads' normwise ceiling of 1e-4."""
    import torch
    d = guide_data(name)
    c = d["case"]
    base, _ = run_refs(c, d["mods"], d["batch"], temperature=d["temperature"], mask_entropy=d["mask_entropy"])
    o = 0
    for pname, prm in d["mods"][0].named_parameters():
        k = prm.numel()
        a, w = d["r64"]["grads"][o:o + k], base["grads"][o:o + k]
        o += k
        share = float((a - w).norm()) / float(w.norm())
        assert share >= (0.01 if c.A == 2 else 2e-4), (name, pname, share)
    assert torch.equal(d["r64"]["grads"][o:], base["grads"][o:])  # the critic does not see the guide


# ------------------------------------------------------------------ GPU
def guide_tensor(gpu, bits, fp16):
    import torch
    t = torch.from_numpy(bits.view(np.int16).copy()).to(gpu)
    return t.view(torch.float16 if fp16 else torch.bfloat16)


def check_guiding_metric(p, r64, r32, mode, tag, n):
    got = float(p.metrics.cpu().double().numpy()[M_GUIDE])
    ok, figures = one_element("guiding_loss", got, r64["guiding"], r32["guiding"], r64["guide_scale"], mode, n)
    print(f"{tag}: {figures}")
    assert ok, f"{tag}: {figures}"


def guided_engine_kw(d):
    g = d["g"]
    return dict(policy_temperature=g.temperature, mask_entropy=g.mask_entropy, infer_fp16=g.fp16)


def make_guided_engine(gpu, d, mode):
    return make_engine(gpu, d["case"], d["mods"], mode, **guided_engine_kw(d))


PAIRS = [(False, ()), (False, (64,)), (True, ()), (True, (64,))]


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layer"])
@pytest.mark.parametrize("fp16,shared", PAIRS, ids=["bf16", "bf16-shared", "fp16", "fp16-shared"])
def test_guide_logits_are_the_16bit_forward(gpu, monkeypatch, fp16, shared, fused):
    """set_guide(X) then guide_logits(obs), after the handle's own parameters were overwritten with another seed's,
    equals forward(0, obs, half=True) taken while the handle held X, bit for bit: n = 1, 37, 65 (the fused kernel's
    64-row workgroup edge) on max_rows = 128, and n = max_rows + 3 on max_rows = 40 (the chunk edge)."""
    import torch
    from rlgpu.ppo import PPO
    if not fused:
        monkeypatch.setenv("RLGPU_FUSED_INFER", "0")
    rng = np.random.default_rng(11)
    for max_rows, ns in ((128, (1, 37, 65)), (40, (43,))):
        p = PPO(policy_layers=(96, 33), critic_layers=(40, 64), shared_layers=shared, max_rows=max_rows, seed=5,
                infer_fp16=fp16)
        assert bool(_fused(p)) == fused
        obs = torch.from_numpy(rng.standard_normal((max(ns), 167)).astype(np.float32)).to(gpu)
        want = {n: torch.cat([p.forward(0, obs[i:min(i + max_rows, n)], half=True) for i in range(0, n, max_rows)]).clone()
                for n in ns}
        p.set_guide(p.policy_version())
        p.init_params(97)
        assert not torch.equal(p.forward(0, obs[:1], half=True), want[ns[0]][:1])  # the handle now holds another policy
        for n in ns:
            got = p.guide_logits(obs[:n])
            assert got.dtype == (torch.float16 if fp16 else torch.bfloat16) and got.shape == (n, 90)
            assert torch.equal(got.float().view(torch.int32), want[n].view(torch.int32)), (max_rows, n)
        p.close()


def _fused(p):
    from rlgpu import _lib
    return _lib.lib().rlgpu_ppo_fused_infer(p._h, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(GUIDE_CASES))
def test_minibatch_guided(gpu, name, mode):
    """One guided minibatch from zero_grad per case of GUIDE_CASES and GEMM mode at guiding_strength 0.5: gradients, the
    six metrics and the fp32 forward against minibatch_ref in float64 under ppo_reference's rules, and the
    guiding-loss metric under its one-element rule."""
    d = guide_data(name)
    assert_guide_side_conditions(d)
    tag = f"{name}/{MODE_IDS[mode]}"

    def named_metric(p):
        assert "Guiding Loss" in p.read_metrics(reset=False), f"{tag}: no Guiding Loss among the named metrics"

    run_engine_case(gpu, d, mode, tag, engine_kw=guided_engine_kw(d),
                    guide=(guide_tensor(gpu, d["bits"], d["g"].fp16), STRENGTH),
                    extra_checks=(lambda p: check_guiding_metric(p, d["r64"], d["r32"], mode, tag, d["case"].n),
                                  named_metric))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rows37", "d64"])
def test_null_guide_is_todays_minibatch(gpu, name):
    """From the same state, the gradient buffer after minibatch_guided without a guide is bit-equal to minibatch's (the
    metrics' atomic order is free), with the options (rows37) and without them (d64)."""
    import torch
    d = guide_data(name)
    c, b = d["case"], d["batch"]
    p = make_guided_engine(gpu, d, 2)
    D = {k: torch.from_numpy(b[k]).to(gpu) for k in ("obs", "masks", "acts", "old", "adv", "tgt", "index")}
    p.adv_normalizer(D["adv"])
    args = (D["obs"], D["masks"], D["acts"], D["old"], D["adv"], D["tgt"], D["index"], b["start"], c.n, b["batch_size"])
    p.zero_grad()
    p.minibatch(*args)
    want = p.grads.clone()
    p.zero_grad()
    p.minibatch_guided(*args, None, 0.7)
    torch.cuda.synchronize()
    assert float(want.abs().max()) > 0
    assert torch.equal(p.grads.view(torch.int32), want.view(torch.int32))
    assert "Guiding Loss" not in p.read_metrics()
    p.close()


@pytest.mark.gpu
def test_guided_minibatch_rejects_bad_arguments(gpu):
    """A negative or non-finite guiding_strength is refused by name; set_guide and guide logits are refused on an
    fp32-inference handle (RLGPU_ERR_UNSUPPORTED), as old versions are."""
    import torch
    from rlgpu import _lib
    from rlgpu.ppo import PPO
    d = guide_data("rows37")
    c, b = d["case"], d["batch"]
    p = make_guided_engine(gpu, d, 2)
    D = {k: torch.from_numpy(b[k]).to(gpu) for k in ("obs", "masks", "acts", "old", "adv", "tgt", "index")}
    args = (D["obs"], D["masks"], D["acts"], D["old"], D["adv"], D["tgt"], D["index"], b["start"], c.n, b["batch_size"])
    guide = guide_tensor(gpu, d["bits"], False)
    for s in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.RLGPUError, match="guiding_strength"):
            p.minibatch_guided(*args, guide, s)
    with pytest.raises(_lib.RLGPUError, match="no guide set"):
        p.guide_logits(D["obs"])
    p.close()
    q = PPO(policy_layers=(96, 33), critic_layers=(40, 64), max_rows=128, infer_fp16=2)
    with pytest.raises(_lib.RLGPUError, match="fp32 inference"):
        q.set_guide(q.policy_version())
    with pytest.raises(_lib.RLGPUError, match="fp32-inference"):
        q.minibatch_guided(*args, guide, 0.5)
    q.close()


@pytest.mark.gpu
def test_guided_metrics_many_rows(gpu):
    """rows8161 (256 loss blocks, slope 1.0) in the h3 mode: the six metrics and the guiding loss over many blocks.  The
    guiding-loss mean is continuous in c, so no sign margin is needed at this row count; gradients are not checked."""
    import torch
    d = guide_data("rows8161")
    c, g = d["case"], d["g"]
    why = side_conditions(c, d["r64"], torch.from_numpy(d["batch"]["masks"][d["rows"]]))
    assert why is None, why
    p = make_guided_engine(gpu, d, 2)
    p.zero_grad()
    engine_minibatch(gpu, p, c, d["batch"], guide_tensor(gpu, d["bits"], g.fp16), STRENGTH)
    check_metrics(p, d["r64"], d["r32"], 2, "rows8161/h3", c.n)
    check_guiding_metric(p, d["r64"], d["r32"], 2, "rows8161/h3", c.n)
    p.close()


@pytest.mark.gpu
def test_guiding_pull(gpu):
    """20 optimizer steps on one fixed 64-row batch with equal advantages (normalised: 0), entropy_scale 0, strength 1,
    lr 1e-3: the guiding-loss metric of the last step is below the first step's (the policy moves toward the guide)."""
    import torch
    from rlgpu.ppo import PPO
    rng = np.random.default_rng(3)
    n = 64
    p = PPO(policy_layers=(96, 33), critic_layers=(40, 64), max_rows=n, seed=5, entropy_scale=0.0, policy_lr=1e-3,
            critic_lr=1e-3)
    q = PPO(policy_layers=(96, 33), critic_layers=(40, 64), max_rows=n, seed=77)  # the guide: another initialisation
    p.set_guide(q.policy_version())
    obs = torch.from_numpy(rng.standard_normal((n, 167)).astype(np.float32)).to(gpu)
    masks = (rng.random((n, 90)) < 0.6).astype(np.uint8)
    masks[np.arange(n), rng.integers(90, size=n)] = 1
    m = torch.from_numpy(masks).to(gpu)
    acts, logp = p.infer_actions(obs, m)
    adv = torch.full((n,), 0.25, device=gpu)
    tgt = torch.zeros(n, device=gpu)
    guide = p.guide_logits(obs)
    assert torch.equal(guide.float(), q.forward(0, obs, half=True))
    p.adv_normalizer(adv)
    assert float(p.adv_stats[1]) == 0.0
    losses = []
    for _ in range(20):
        p.metrics.zero_()
        p.minibatch(obs, m, acts, logp, adv, tgt, None, 0, n, n, guide_logits=guide, guiding_strength=1.0)
        losses.append(float(p.metrics[M_GUIDE]))
        p.optimizer_step()
    print("guiding loss, steps 1 and 20:", losses[0], losses[-1])
    assert all(np.isfinite(losses)) and losses[0] > 0
    assert losses[-1] < losses[0], losses
    p.close()
    q.close()

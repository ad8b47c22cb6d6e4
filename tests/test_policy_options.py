"""PPOLearnerConfig::policyTemperature and maskEntropy (rlgpu_ppo_config.policy_temperature / mask_entropy) in the
sampler and in rlgpu_ppo_minibatch.

The reference (PPOLearner.cpp): InferPolicyProbsFromModels (:97-102) and Learn (:411-415) run the softmax on
logits / temperature + (-1e10) * !mask -- an fp32 division of the fp32-converted logits, the mask term added after it;
with maskEntropy (:426-438) each row's entropy is divided by log(the row's legal actions) instead of log(A).

  * Learn: ppo_reference.minibatch_ref with the two options.  The GPU cases are held to that module's rules and
    constants unchanged (check_grads, check_metrics, check_forward): the only differences come in through the
    reference's return values -- the entropy's rounding scale divides by log(legal count) per row when masked, and
    the z terms of every scale are the tempered logits.  Side conditions (the float64 reference alone decides them,
    on the CPU in test_option_side_conditions_hold and again in each GPU test): the kink margin DELTA, no legal
    probability within 0.1 % of the clamp, no ratio within 1e-4 of 1 +- clip, and with mask_entropy at least two
    legal actions in every minibatch row (one legal action divides by log 1 = 0, in the reference too).
  * Sampler: actions and log-prob bit patterns equal the oracle sampler's on (logits as f32) / np.float32(T), which
    numpy rounds as the IEEE fp32 division it is.  The test first shows on the CPU that a multiply by the reciprocal
    would not pass it.
"""
import ctypes

import numpy as np
import pytest

import oracle
from ppo_reference import MODE_IDS, MODES, Case, build_case, check_golden, run_engine_case, run_refs, side_conditions


# ------------------------------------------------------------------ the cases
# (case, temperature, mask_entropy).  loss<K> = policy_loss<K>, ldd = the dlogits row stride (test_ppo_variants).
OPTION_CASES = {
    # loss<2>, ldd 17 -> 20; T < 1, the launch-constant entropy path with a temperature
    "b17_t0.7": (Case("b17", 168, 17, (64, 128), (65, 33), seed=1), 0.7, False),
    # loss<6>, ldd 90 -> 92; two 32-row blocks with a ragged tail
    "rows37_t2.5_me": (Case("rows37", 167, 90, (96, 33), (40, 64), seed=0, n=37), 2.5, True),
    # the 1-row and 33-row block edges
    "rows1_t0.7_me": (Case("rows1", 167, 90, (96, 33), (40, 64), seed=0, n=1), 0.7, True),
    "rows33_t2.5_me": (Case("rows33", 167, 90, (96, 33), (40, 64), seed=0, n=33), 2.5, True),
    # loss<4>, ldd 64; mask_entropy alone (T = 1)
    "d64_t1_me": (Case("d64", 168, 64, (256, 257), (128, 65), seed=0), 1.0, True),
    # loss<8>, ldd 128 unpadded
    "a128_t3_me": (Case("a128", 168, 128, (130, 64), (65, 128), seed=0), 3.0, True),
    # loss<1>, ldd 2 -> 4; the temperature alone
    "a2_t1.5": (Case("a2", 167, 2, (33, 65), (130, 64), seed=0), 1.5, False),
    # 256 blocks of the loss kernel with a one-row last block: the metric reduction over many blocks (slope 1.0: the
    # kink cannot be avoided at this row count)
    "rows8161_t1.5_me": (Case("rows8161", 167, 90, (64, 36), (64, 36), seed=0, slope=1.0, n=8161, extra=100), 1.5, True),
}


def option_data(name):
    c, temperature, mask_entropy = OPTION_CASES[name]
    return build_case(c, temperature=temperature, mask_entropy=mask_entropy)


def assert_option_side_conditions(d):
    import torch
    c, rows = d["case"], d["rows"]
    masks = d["batch"]["masks"][rows]
    why = side_conditions(c, d["r64"], torch.from_numpy(masks))  # kink, clamp and clip margins, on the tempered probs
    assert why is None, f"case {c.name}: {why}"
    legal = masks.sum(1)
    if d["mask_entropy"]:
        assert legal.min() >= 2, f"case {c.name}: a minibatch row with {legal.min()} legal action(s)"
    assert np.isfinite(d["r64"]["metrics"]).all() and bool(d["r64"]["grads"].isfinite().all())


# ------------------------------------------------------------------ CPU tests
def test_config_mirrors_match_c_sizes():
    """ctypes.sizeof of the Python mirrors of rlgpu_ppo_config / rlgpu_learner_config equals the library's sizeof."""
    from rlgpu import learner, ppo
    assert ctypes.sizeof(ppo._Cfg) == ppo._bind().rlgpu_ppo_config_size()
    assert ctypes.sizeof(learner._CConfig) == learner._bind().rlgpu_learner_config_size()
    assert ppo._Cfg._fields_[-2:] == [("policy_temperature", ctypes.c_float), ("mask_entropy", ctypes.c_int32)]
    assert learner._CConfig._fields_[-2:] == [("policy_temperature", ctypes.c_float), ("mask_entropy", ctypes.c_int32)]


def _small_cfg():
    from rlgpu.ppo import _Cfg
    cfg = _Cfg()
    cfg.obs_size, cfg.num_actions, cfg.max_rows = 167, 90, 64
    cfg.n_policy_layers = cfg.n_critic_layers = 1
    cfg.policy_layers[0] = cfg.critic_layers[0] = 64
    return cfg


@pytest.mark.parametrize("field,value", [("policy_temperature", -1.0), ("policy_temperature", float("nan")),
                                         ("policy_temperature", float("inf")), ("mask_entropy", 2)])
def test_create_rejects_bad_options(field, value):
    """rlgpu_ppo_create names a negative, NaN or infinite policy_temperature and a mask_entropy outside {0, 1}
    before it allocates anything (no GPU needed), with RLGPU_ERR_INVALID_ARG."""
    from rlgpu.ppo import _bind
    L = _bind()
    L.rlgpu_last_error.restype = ctypes.c_char_p
    cfg = _small_cfg()
    setattr(cfg, field, value)
    h = ctypes.c_void_p()
    assert L.rlgpu_ppo_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and not h.value  # RLGPU_ERR_INVALID_ARG
    assert field.encode() in L.rlgpu_last_error()


def test_create_accepts_zeroed_options():
    """policy_temperature = 0 (a zero-initialised config) means 1: create does not reject it (without a GPU it
    fails later, on its first allocation, not on the field)."""
    from rlgpu.ppo import _bind
    L = _bind()
    L.rlgpu_last_error.restype = ctypes.c_char_p
    cfg = _small_cfg()
    assert cfg.policy_temperature == 0.0 and cfg.mask_entropy == 0
    h = ctypes.c_void_p()
    if L.rlgpu_ppo_create(ctypes.byref(cfg), ctypes.byref(h)) == 0:
        assert L.rlgpu_ppo_destroy(h) == 0
    else:
        err = L.rlgpu_last_error()
        assert b"policy_temperature" not in err and b"mask_entropy" not in err


def test_learner_default_config_options():
    """rlgpu_learner_default_config writes the reference's defaults: temperature 1, maskEntropy off."""
    from rlgpu import learner
    L = learner._bind()
    c = learner._CConfig()
    L.rlgpu_learner_default_config.argtypes = [ctypes.POINTER(learner._CConfig)]
    assert L.rlgpu_learner_default_config(ctypes.byref(c)) == 0
    assert c.policy_temperature == 1.0 and c.mask_entropy == 0 and c.collect_groups == 0 and c.world == 1
    assert learner.LearnerConfig().policy_temperature == 1.0 and learner.LearnerConfig().mask_entropy is False


@pytest.mark.parametrize("name", list(OPTION_CASES))
def test_reference_matches_golden(name):
    """The float64 reference of every option case against tests/golden/ppo_reference.npz (ppo_reference.check_golden)."""
    check_golden(f"option/{name}", option_data(name))


def test_reference_options_change_the_result():
    """The two options move the reference: the temperature every policy gradient, maskEntropy the entropy (larger:
    every row has fewer legal actions than A) and through it the policy gradient."""
    d = option_data("rows37_t2.5_me")
    c, b = d["case"], d["batch"]
    assert (b["masks"][d["rows"]].sum(1) < c.A).all()
    r_t, _ = run_refs(c, d["mods"], b, temperature=2.5, mask_entropy=False)
    base, _ = run_refs(c, d["mods"], b, temperature=1.0, mask_entropy=False)
    assert d["r64"]["metrics"][0] > r_t["metrics"][0] > 0
    npol = sum(q.numel() for q in d["mods"][0].parameters())
    for a, w in ((d["r64"], r_t), (r_t, base)):
        assert float((a["grads"][:npol] - w["grads"][:npol]).norm()) > 1e-6 * float(w["grads"][:npol].norm())
        assert bool((a["grads"][npol:] == w["grads"][npol:]).all())  # the critic sees neither option


@pytest.mark.parametrize("name", list(OPTION_CASES))
def test_option_side_conditions_hold(name):
    """Every case's kink, clamp and clip margins and legal-action counts, by the float64 reference alone; 0.3 - 0.7 of
    the rows' ratios inside the clip range wherever there are enough rows to count."""
    d = option_data(name)
    assert_option_side_conditions(d)
    c = d["case"]
    if c.n >= 31:
        assert 0.3 <= d["r64"]["metrics"][5] <= 0.7, d["r64"]["metrics"][5]
    if d["mask_entropy"]:
        assert (d["batch"]["masks"][d["rows"]].sum(1) < c.A).any()  # the divisor differs from log A


# ------------------------------------------------------------------ GPU: gradients and metrics
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(OPTION_CASES))
def test_minibatch_with_options(gpu, name, mode):
    """One minibatch from zero_grad per case of OPTION_CASES and GEMM mode on an engine built with the case's
    policy_temperature / mask_entropy: gradients and the six metrics against minibatch_ref in float64 under
    ppo_reference's rules, the fp32 forward (raw logits: rlgpu_ppo_forward applies no temperature) as there."""
    d = option_data(name)
    assert_option_side_conditions(d)
    run_engine_case(gpu, d, mode, f"{name}/{MODE_IDS[mode]}",
                    engine_kw=dict(policy_temperature=d["temperature"], mask_entropy=d["mask_entropy"]))


# ------------------------------------------------------------------ GPU: the sampler
N_ROWS, N_ACT = 203, 90  # no multiple of the fused kernel's 8-row wave groups or of the layered kernel's 4-row blocks
STEPS = (0, 77, 2**40 + 5)
OBS_SEED = 7


def sampler_inputs():
    from test_ppo import make_batch
    obs, masks, *_ = make_batch(np.random.default_rng(OBS_SEED), N_ROWS)
    masks[::29] = 0
    masks[::29, 11] = 1  # rows with one legal action
    return obs, masks


def exact_logits(p, o, fp32=False):
    """The policy's logits as the sampler reads them, as f32: the 16-bit values exactly (forward(half=True)), or the
    fp32 inference's."""
    f = p.forward(0, o, half=not fp32).cpu().numpy()
    assert f.dtype == np.float32
    return f


def assert_division_is_told_apart(logits, masks, temperature, seed):
    """CPU precondition: the oracle's log probs on logits * (1 / T) differ from those on logits / T in at least one
    row, so a sampler that multiplied by the reciprocal would fail the comparison below."""
    t = np.float32(temperature)
    _, lp_div = oracle.sample_actions(logits / t, masks, False, seed, 0, 0)
    _, lp_mul = oracle.sample_actions(logits * (np.float32(1) / t), masks, False, seed, 0, 0)
    assert (lp_div.view(np.uint32) != lp_mul.view(np.uint32)).any()


def check_sampler(p, o, m, logits, masks, temperature, rows=None, infer=None):
    """p's actions and log probs over STEPS and both deterministic values against the oracle on logits / T (rows:
    the rows to compare, all by default; infer: the call, p.infer_actions by default)."""
    t = np.float32(temperature)
    rows = np.arange(len(masks)) if rows is None else rows
    infer = p.infer_actions if infer is None else infer
    for det in (True, False):
        for step in STEPS:
            a, lp = infer(o, m, step=step, deterministic=det)
            wa, wlp = oracle.sample_actions(logits / t, masks, det, p.cfg.seed, step, 0)
            ga, glp = a.cpu().numpy(), lp.cpu().numpy()
            bad = rows[ga[rows] != wa[rows]]
            assert bad.size == 0, (step, det, bad[:5], ga[bad[:5]], wa[bad[:5]])
            yield det, step, ga, glp, wlp


@pytest.mark.gpu
@pytest.mark.parametrize("temperature", [0.7, 3.0])
@pytest.mark.parametrize("kw,fused", [
    (dict(), True),
    (dict(), False),
    (dict(policy_layers=(256, 256), infer_fp16=True), True),
    (dict(infer_fp16=2), True),
    (dict(max_rows=96), True)],
    ids=["bf16-fused", "bf16-layer", "fp16-fused", "fp32", "chunked"])
def test_tempered_sampler_bit_exact_vs_oracle(gpu, monkeypatch, kw, fused, temperature):
    """203 rows, A = 90, every 29th row with one legal action, on each inference path: actions and log-prob bits
    equal the oracle sampler's on the fp32 division logits / T."""
    import torch
    from rlgpu.ppo import PPO
    if not fused:
        monkeypatch.setenv("RLGPU_FUSED_INFER", "0")
    kw = dict(dict(max_rows=N_ROWS), **kw)
    p = PPO(seed=31, policy_temperature=temperature, **kw)
    obs, masks = sampler_inputs()
    o, m = torch.from_numpy(obs).to(gpu), torch.from_numpy(masks).to(gpu)
    R = p.max_rows
    logits = np.concatenate([exact_logits(p, o[i:i + R], kw.get("infer_fp16") == 2) for i in range(0, N_ROWS, R)])
    assert_division_is_told_apart(logits, masks, temperature, p.cfg.seed)
    for det, step, ga, glp, wlp in check_sampler(p, o, m, logits, masks, temperature):
        np.testing.assert_array_equal(glp.view(np.uint32), wlp.view(np.uint32))
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("temperature", [0.7, 3.0])
def test_tempered_mixed_sampler_bit_exact_vs_oracle(gpu, temperature):
    """infer_actions_mixed: every third row acts with an old version (set_version) at the handle's temperature --
    its actions equal the oracle's on the old version's logits (from a second handle holding those parameters); the
    other rows' actions and log probs equal the oracle's on the current policy's."""
    import torch
    from rlgpu.ppo import PPO
    p = PPO(max_rows=N_ROWS, seed=31, policy_temperature=temperature)
    q = PPO(max_rows=N_ROWS, seed=31, init=False)
    q.init_params(97)  # the old version: another initialisation
    p.set_version(q.policy_version())
    obs, masks = sampler_inputs()
    o, m = torch.from_numpy(obs).to(gpu), torch.from_numpy(masks).to(gpu)
    old = np.zeros(N_ROWS, np.uint8)
    old[::3] = 1
    old_rows = torch.from_numpy(old).to(gpu)
    cur_logits, old_logits = exact_logits(p, o), exact_logits(q, o)
    assert not np.array_equal(cur_logits, old_logits)
    assert_division_is_told_apart(cur_logits, masks, temperature, p.cfg.seed)
    infer = lambda o, m, **k: p.infer_actions_mixed(o, m, old_rows, **k)  # noqa: E731
    cur, oldr = np.nonzero(old == 0)[0], np.nonzero(old)[0]
    for det, step, ga, glp, wlp in check_sampler(p, o, m, cur_logits, masks, temperature, rows=cur, infer=infer):
        np.testing.assert_array_equal(glp[cur].view(np.uint32), wlp[cur].view(np.uint32))
        wa, _ = oracle.sample_actions(old_logits / np.float32(temperature), masks, det, p.cfg.seed, step, 0)
        bad = oldr[ga[oldr] != wa[oldr]]
        assert bad.size == 0, (step, det, bad[:5])
    p.close()
    q.close()


@pytest.mark.gpu
def test_default_options_are_todays_sampler(gpu):
    """A handle built without the options, one with policy_temperature = 1.0 / mask_entropy = False and one whose raw
    config field is 0 return bit-identical actions and log probs -- which are the oracle's on the untempered logits;
    at T = 3 the non-deterministic actions differ from them on at least one row (the field is not ignored)."""
    import torch
    from rlgpu.ppo import PPO
    obs, masks = sampler_inputs()
    o, m = torch.from_numpy(obs).to(gpu), torch.from_numpy(masks).to(gpu)
    ps = [PPO(max_rows=N_ROWS, seed=31), PPO(max_rows=N_ROWS, seed=31, policy_temperature=1.0, mask_entropy=False),
          PPO(max_rows=N_ROWS, seed=31, policy_temperature=0.0)]
    assert ps[2].cfg.policy_temperature == 0.0 and ps[0].cfg.policy_temperature == 1.0
    hot = PPO(max_rows=N_ROWS, seed=31, policy_temperature=3.0)
    logits = exact_logits(ps[0], o)
    bits = (logits.view(np.uint32) >> 16).astype(np.uint16)
    differs = False
    for det in (True, False):
        for step in STEPS:
            res = [tuple(t.cpu().numpy() for t in p.infer_actions(o, m, step=step, deterministic=det)) for p in ps]
            wa, wlp = oracle.sample_actions(bits, masks, det, 31, step, 0)
            for a, lp in res:
                np.testing.assert_array_equal(a, wa)
                np.testing.assert_array_equal(lp.view(np.uint32), wlp.view(np.uint32))
            if not det:
                a3, _ = hot.infer_actions(o, m, step=step, deterministic=False)
                differs = differs or bool((a3.cpu().numpy() != res[0][0]).any())
    assert differs
    for p in ps + [hot]:
        p.close()

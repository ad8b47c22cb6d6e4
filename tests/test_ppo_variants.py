"""Every leaf of the dispatch tree behind rlgpu_ppo_minibatch against a float64 reference.

The reference (minibatch_ref) is the PyTorch restatement of PPOLearner::Learn's minibatch body that
test_ppo.ref_minibatch is, generic in the dtype: run on float64 copies of the modules it is the reference, run
on the fp32 modules it is the yardstick -- the engine must be as close to float64 as torch's own fp32 is:

    per parameter tensor   ||g - g64|| <= F * ||g32 - g64|| + 1e-7 * ||g64||            (F = 4, see below)
                           ||g - g64|| <= 1e-4 * ||g64||                                 (the kink-free contract)
                           |g - g64|   <= 1e-3 * |g64| + 1e-4 * max |g64|  elementwise   (now at slope 0.01 too)
    forward outputs        the first rule on the logits and the values of every row of the batch
    one-element results    |m - m64| <= F * |m32 - m64| + K(n) * 2^-24 * S      (the six metrics, and the rank-1
                           head's bias gradient, a one-element tensor, on top of its tensor rule's floor)

The 4 and the 1e-7 are test_gemm_modes_fp32_class_accuracy's.  A one-element fp32 result has no usable
one-element yardstick: torch's own fp32 scalar lands within a fraction of an ulp of float64 as often as not (measured
here: 5e-10 relative on a clip fraction, 4e-9 on the head's bias gradient, where the engine was one ulp off), so a
scalar also gets a floor in units of u S, u = 2^-24:
  * S is what one rounding of a term's inputs moves the mean by: with z the legal logits, zmax their largest
    magnitude and c = 1 + |z_action| + zmax + |old log prob|, ratio: mean(ratio c); KL: mean((ratio + 1) c); policy
    loss: mean(|adv| ratio c); entropy: mean(sum_k p_k (|log p_k| + 1)(1 + |z_k| + zmax)) / log A; critic loss:
    mean(2 |v - t| (|v| + |t|) + (v - t)^2) bsr; clip fraction: 1; head bias gradient: 2 bsr / n sum(|v| + |t|).
  * K(n) = 4 + sqrt(ceil(n / 32)), never more than 1e-4 / u: 4 roundings of a term and its mean, and one fp32 add per
    32-row block (the loss kernel's atomic adds, in any order), whose roundings add up like a random walk --
    0.17 sqrt(blocks) u S expected, so sqrt(blocks) is 6 sigma.  Not the worst case, which grows like n and would
    let a dropped block through.
  * Measured on an MI355X over two runs, the engine's largest error in units of u S (the loss kernel is the same in
    every mode; the order of its atomic adds is not): 37 rows and fewer (K = 5.0 .. 5.4) 2.4 on a metric and 2.9 on the
    head's bias gradient; 8161 rows (K = 20) 3.3; 32771 rows (K = 36) 5.0 and 9.1, on the clip fraction, which K
    allows 2.1e-6 where one row on the wrong side moves it by 1 / n = 3.1e-5.  Largest err / floor per mode
    (x6 / f32 / h3): 0.14 / 0.38 / 0.58 at 37 rows and fewer, 0.14 / 0.17 / 0.25 at 8161 and 32771 rows.

Cases are built on the CPU from numpy streams (Linear: U(+-1/sqrt(fan_in)) like the engine's init; LayerNorm weight
1 + 0.2 N(0,1), bias 0.2 N(0,1), so that a wrong column map of gamma / beta shows), loaded with
load_torch_module and read back with torch_module (asserted bit-equal), so the side conditions below are
evaluated by the reference alone, here on the CPU for every case (test_side_conditions_hold) and again inside
each GPU test:

  * kink margin: with a LeakyReLU slope other than 1 every float64 pre-activation has |h| >= DELTA.  Measured on
    the CPU over the case table: the largest |h32 - h64| of a torch fp32 forward is 3.2e-6 (test_delta_covers_fp32
    recomputes it), 10 x that is 3.2e-5, rounded up to DELTA = 4.5e-5.
  * no legal action's float64 probability within 0.1 % of the 1e-11 clamp; no ratio within 1e-4 of 1 +- clip.
The seeds in the table were searched on the CPU until every case passes.

The error ratios measured on an MI355X are written at factor() below.  The optimizer test's share of coordinates
outside the tight band is written at OPT_SHARE: 0 between torch fp32 and float64 on the CPU, 1e-4 allowed (the engine
measured 0 in every mode, largest parameter difference 1.0e-6; its grad-norm metrics were within 2.4e-7 relative of
the float64 norms, against a bound of about 1e-6).
"""
import copy
import functools
import math
from typing import NamedTuple

import numpy as np
import pytest

from tests_util import random_actions

CLIP, ENT_SCALE = 0.2, 0.035
DELTA = 4.5e-5  # kink margin, see the module docstring
MODES = [0, 1, 2]
MODE_IDS = ["x6", "f32", "h3"]
# The yardstick factor (4: test_gemm_modes_fp32_class_accuracy's).  Measured on an MI355X, the largest
# (err - floor) / (torch fp32 err) over this file, gradients / forward outputs: x6 1.52 / 0.63, f32 3.25 / 2.21,
# h3 4.57 / 1.30 (the metrics: module docstring).  The one excess is h3 on the one-row minibatch (critic.3.weight
# 4.15, critic.4.bias 4.57; 1.61 on every other case): with one row nothing averages, every element of the critic's
# gradient is a per-row factor times the one dv = 2 (v - t) bsr, so each tensor's error is v's error amplified by
# |v| / |v - t|, and v comes from H3's 22-bit products (2^-22 per product against fp32's 2^-24).  For that mode and
# that case the factor is twice the measured ratio; the 1e-4 normwise ceiling holds everywhere.
def factor(mode, n):
    return 9.2 if (mode == 2 and n == 1) else 4.0


class Case(NamedTuple):
    name: str
    obs: int
    A: int
    pol: tuple
    crit: tuple
    seed: int = 0
    ln: bool = True
    slope: float = 0.01
    n: int = 37
    extra: int = 27          # rows of the batch beyond the minibatch's (index / start pick n of n + extra)
    first_scale: float = 1.0  # the first Linear's weight and bias, both models
    obs_scale: float = 1.0
    out_scale: float = 1.0    # the policy's output Linear (logit range)
    edge: bool = False        # the loss kernel's edge rows


# Kernel reached per case.  fwd<M> / bwd<M> = ln_act_fwd_f32<M> / ln_act_bwd<M, false>, +head = the critic's last
# layer (fused rank-1 head: ln_act_fwd_f32<M> with head_w, ln_act_bwd<M, true>), v / s = float4 / scalar path
# (float4 needs H % 4 == 0 and M % 4 == 0, so M = 1 and M = 2 only have the scalar path), wide<NV> =
# ln_act_fwd_wide<NV> / ln_act_bwd_wide<NV>, loss<K> = policy_loss<K>, ldd = dlogits row stride.
# M = 16 / 32 take the float4 path only under the head (the wide kernels take every other multiple of 4).
SWEEP = [
    # 33: fwd/bwd<1> s; 65: <2> s; 130: <4> s; 64: <1> +head;   loss<1>, ldd 2 -> 4; obs 167 -> 168
    Case("a2", 167, 2, (33, 65), (130, 64), seed=0),
    # 64: <1> s; 128: <2> s; 65: <2> s; 33: <1> +head (odd);    loss<2>, ldd 17 -> 20; obs 168 unpadded
    Case("b17", 168, 17, (64, 128), (65, 33), seed=1),
    # 130: <4> s; 255: <4> s; 33: <1>; 128: <2> +head;          loss<1>, ldd 16 unpadded
    Case("c16", 167, 16, (130, 255), (33, 128), seed=1),
    # 256: <4> v; 257: <8> s; 128: <2>; 65: <2> +head (odd);    loss<4>, ldd 64
    Case("d64", 168, 64, (256, 257), (128, 65), seed=0),
    # 510: <8> s; 512: <8> v; 257: <8> s; 256: <4> v +head;     loss<7>, ldd 100
    Case("e100", 167, 100, (510, 512), (257, 256), seed=8),
    # 255: <4> s; 512: <8> v; 255: <4> s +head (odd);           loss<8>, ldd 113 -> 116
    Case("f113", 167, 113, (255,), (512, 255), seed=2),
    # 516, 1024: wide<1>; 256: <4> v; 512: <8> v +head;         loss<8>, ldd 128 unpadded
    Case("g128", 168, 128, (516, 1024), (256, 512), seed=75),
    # 1028, 2048: wide<2>; 510: <8> s; 257: <8> s +head (odd);  loss<6>, ldd 90 -> 92
    Case("h90", 167, 90, (1028, 2048), (510, 257), seed=254),
    # 1023: <16> s; 2047: <32> s; 1024: <16> v +head
    Case("i16", 167, 16, (1023,), (2047, 1024), seed=350),
    # 2047: <32> s; 1024: wide<1> (critic, non-last); 1023: <16> s +head (odd)
    Case("j17", 167, 17, (2047,), (1024, 1023), seed=32),
    # 1028: wide<2>; 1023: <16> s; 2048: <32> v +head
    Case("k2", 168, 2, (1028,), (1023, 2048), seed=379),
    # 516: wide<1>; 2048: wide<2> (critic, non-last); 2047: <32> s +head (odd)
    Case("l64", 167, 64, (516,), (2048, 2047), seed=81),
    # layer_norm = 0, narrow: 65: <2>; 256: <4> v; 130: <4> s; 33: <1> +head -- the use_ln = 0 branches
    Case("noln", 167, 90, (65, 256), (130, 33), seed=7, ln=False),
    # layer_norm = 0 above 512 columns: 516: wide<1>; 33: <1>; 1023: <16> s +head
    Case("noln_wide", 167, 90, (516, 33), (1023,), seed=2, ln=False),
    # 8 hidden layers in both models: 18 (policy) / 17 (critic) Reducer jobs > kRedJobs = 16: the mid-pass flush
    Case("deep8", 167, 90, (40, 33, 64, 48, 36, 65, 44, 52), (36, 64, 33, 52, 40, 65, 48, 44), seed=3),
    # first Linear x 1e-3, obs x 4: pre-norm row variance ~ 5e-6 against eps = 1e-5 (eps placement, biased variance)
    Case("smallvar", 167, 90, (130, 64), (65, 128), seed=3, first_scale=1e-3, obs_scale=4.0),
] + [
    # row-count edges on a narrow model (16-row forward, 32-row backward and loss blocks); adv_stats from n + 27 rows
    Case(f"rows{n}", 167, 90, (96, 33), (40, 64), seed=0, n=n) for n in (1, 31, 32, 33)
]
# The LeakyReLU kink cannot be avoided at these row counts: slope 1.0.  The subject is the reductions -- 8161 rows:
# 256 blocks of the 32-row LayerNorm backward and of the loss kernel, the first two-level Reducer job (G = 16), with
# a one-row last block; 32771 rows: split-K weight gradients at the kMaxSplits = 256 cap -- and the gather's
# grid-stride loop (more than 2048 x 256 elements).
MANY = [Case("rows8161", 167, 90, (64, 36), (64, 36), seed=0, slope=1.0, n=8161, extra=100),
        Case("rows32771", 167, 90, (64, 36), (64, 36), seed=0, slope=1.0, n=32771, extra=100)]
# loss-kernel edge rows on a default-width policy, logits spanning about +-60
EDGE = Case("edge", 167, 90, (512, 512), (64,), seed=20, n=64, out_scale=50.0, edge=True)
# the optimizer runs: slope 1.0 (after the first step the two trajectories differ in the last bits, so a kink
# margin chosen for the reference's parameters says nothing about the engine's)
OPTIM = Case("optim", 167, 90, (130, 64), (65, 128), seed=0, slope=1.0, n=64)
CASES = {c.name: c for c in SWEEP + MANY + [EDGE]}


# ------------------------------------------------------------------ the reference
def run_seq(seq, x):
    """seq(x) and the input of every LeakyReLU."""
    import torch
    pre = []
    for mod in seq:
        if isinstance(mod, torch.nn.LeakyReLU):
            pre.append(x.detach())
        x = mod(x)
    return x, pre


def masked_probs(logits, masks):
    """InferPolicyProbsFromModels: (unclamped, clamped) masked softmax."""
    import torch
    raw = torch.softmax(logits + -1e10 * masks.bool().logical_not(), -1)
    return raw, raw.clamp(1e-11, 1.0)


def minibatch_ref(pol, crit, obs, masks, acts, old_logp, adv, target, batch_size, clip=CLIP, ent_scale=ENT_SCALE):
    """PPOLearner::Learn's minibatch body (PPOLearner.cpp:341-498) in the dtype of the modules and inputs; from
    zeroed gradients.  Returns the flat gradients (policy, then critic: the engine's order), the six metrics
    (entropy, KL, policy loss, critic loss, mean ratio, clip fraction; KL = mean(exp(lr) - 1 - lr), clip fraction
    = mean(|ratio - 1| > clip), PPOLearner.cpp:484-489), the rounding scale of each metric (module docstring),
    every pre-activation, the outputs, the unclamped probabilities and the ratios."""
    import torch
    for m in (pol, crit):
        m.zero_grad(set_to_none=True)
    n = obs.shape[0]
    bsr = n / float(batch_size)
    logits, pre_p = run_seq(pol, obs)
    raw, probs = masked_probs(logits, masks)
    logp = probs.gather(-1, acts.long().unsqueeze(-1)).squeeze(-1).log()
    ent = (-(probs.log() * probs).sum(-1) / math.log(probs.shape[1])).mean()
    lr = logp - old_logp
    ratio = lr.exp()
    clipped = ratio.clamp(1 - clip, 1 + clip)
    terms = torch.min(ratio * adv, clipped * adv)
    pl = -terms.mean()
    vals, pre_c = run_seq(crit, obs)
    vals = vals.flatten()
    closs = torch.nn.functional.mse_loss(vals, target) * bsr
    ((pl - ent * ent_scale) * bsr + closs).backward()
    kl = (lr.exp() - 1 - lr).mean()
    frac = ((ratio - 1).abs() > clip).to(obs.dtype).mean()
    f = lambda t: float(t.detach().double())  # noqa: E731
    # what one rounding of the inputs of each metric's terms moves the metric by (module docstring)
    with torch.no_grad():
        z = logits + -1e10 * masks.bool().logical_not()
        zm = z.max(-1).values.abs()
        ai = acts.long().unsqueeze(-1)
        legal_a = masks.bool().gather(-1, ai).squeeze(-1)  # a masked action's log prob is log(1e-11) exactly
        lcond = 1 + (logits.gather(-1, ai).squeeze(-1).abs() + zm) * legal_a + old_logp.abs()
        zc = 1 + logits.abs() * masks.bool() + zm.unsqueeze(-1)
        s_ent = ((probs * (probs.log().abs() + 1) * zc).sum(-1) / math.log(probs.shape[1])).mean()
        s_crit = ((2 * (vals - target).abs() * (vals.abs() + target.abs()) + (vals - target) ** 2).mean()) * bsr
        s_head = 2 * bsr / n * (vals.abs() + target.abs()).sum()
    return {"grads": torch.cat([p.grad.reshape(-1) for m in (pol, crit) for p in m.parameters()]).clone(),
            "metrics": np.array([f(ent), f(kl), f(pl), f(closs), f(ratio.mean()), f(frac)]),
            "scales": np.array([f(s_ent), f(((ratio + 1) * lcond).mean()), f((adv.abs() * ratio * lcond).mean()),
                                f(s_crit), f((ratio * lcond).mean()), 1.0]),
            "head_bias_scale": f(s_head),
            "pre": pre_p + pre_c, "logits": logits.detach(), "values": vals.detach(), "raw_probs": raw.detach(),
            "ratio": ratio.detach()}


def side_conditions(c, ref, masks):
    """The conditions under which a float64 reference decides an fp32 result (module docstring); None or a reason."""
    if c.slope != 1.0:
        h = min(float(p.abs().min()) for p in ref["pre"])
        if h < DELTA:
            return f"pre-activation {h:.2e} inside the kink margin {DELTA:.0e}"
    legal = ref["raw_probs"][masks.bool()]
    near = ((legal / 1e-11 - 1).abs() < 1e-3).sum().item()
    if near:
        return f"{near} legal probabilities within 0.1 % of the clamp"
    r = ref["ratio"]
    d = min(float((r - (1 - CLIP)).abs().min()), float((r - (1 + CLIP)).abs().min()))
    if d < 1e-4:
        return f"a ratio {d:.1e} from the clip range's end"
    return None


# ------------------------------------------------------------------ the cases
def build_modules(c, seed=None):
    """(policy, critic) fp32 torch modules of case c, filled from a numpy stream."""
    import torch
    from rlgpu.ppo import make_sequential
    rng = np.random.default_rng(1000 + (c.seed if seed is None else seed))
    mods = [make_sequential(c.obs, c.A, c.pol, c.ln, c.slope), make_sequential(c.obs, 1, c.crit, c.ln, c.slope)]
    with torch.no_grad():
        for mi, seq in enumerate(mods):
            linears = [m for m in seq if isinstance(m, torch.nn.Linear)]
            for m in seq:
                if isinstance(m, torch.nn.Linear):
                    bound = 1.0 / math.sqrt(m.in_features)
                    s = c.first_scale if m is linears[0] else (c.out_scale if (mi == 0 and m is linears[-1]) else 1.0)
                    m.weight.copy_(torch.from_numpy((rng.uniform(-bound, bound, m.weight.shape) * s).astype(np.float32)))
                    m.bias.copy_(torch.from_numpy((rng.uniform(-bound, bound, m.bias.shape) * s).astype(np.float32)))
                elif isinstance(m, torch.nn.LayerNorm):
                    m.weight.copy_(torch.from_numpy((1 + 0.2 * rng.standard_normal(m.weight.shape)).astype(np.float32)))
                    m.bias.copy_(torch.from_numpy((0.2 * rng.standard_normal(m.bias.shape)).astype(np.float32)))
    return mods


def build_batch(c, pol64, seed=None):
    """A batch of n + extra rows, of which index[start : start + n] is the minibatch.  The old log probs are the
    float64 policy's own plus noise, so the ratios straddle the clip range."""
    import torch
    rng = np.random.default_rng(7919 * (c.seed if seed is None else seed) + 17)
    B, A = c.n + c.extra, c.A
    obs = (rng.standard_normal((B, c.obs)) * c.obs_scale).astype(np.float32)
    masks = (rng.random((B, A)) < 0.6).astype(np.uint8)
    masks[np.arange(B), rng.integers(A, size=B)] = 1
    acts = random_actions(masks, rng)
    # log ratios inside the clip range, above it and below it, none near its ends (log 0.8 = -0.223, log 1.2 = 0.182)
    which = rng.random(B)
    noise = np.where(which < 0.5, rng.uniform(-0.15, 0.12, B),
                     np.where(which < 0.75, rng.uniform(0.25, 0.6, B), rng.uniform(-0.6, -0.3, B)))
    index = rng.permutation(B).astype(np.int32)
    start = c.extra // 3
    if c.edge:
        rows = index[start:start + c.n]
        one, off = rows[:8], rows[8:20]
        masks[one] = 0
        masks[one, rng.integers(A, size=len(one))] = 1  # a single legal action
        acts[one] = masks[one].argmax(1)
        masks[off, 0] = 0
        masks[off, 1] = 1
        acts[off] = 0                                    # the stored action is masked: the clamped 1e-11 is gathered
        noise = np.where(rng.random(B) < 0.5, 0.7, -0.7) * (rng.random(B) < 0.6) + rng.uniform(-0.1, 0.1, B)
    with torch.no_grad():
        _, probs = masked_probs(pol64(torch.from_numpy(obs).double()), torch.from_numpy(masks))
        lp = probs.gather(-1, torch.from_numpy(acts).long().unsqueeze(-1)).squeeze(-1).log().numpy()
    old = (lp + noise).astype(np.float32)
    adv = rng.standard_normal(B).astype(np.float32)
    tgt = rng.standard_normal(B).astype(np.float32)
    return {"obs": obs, "masks": masks, "acts": acts, "old": old, "adv": adv, "tgt": tgt, "index": index,
            "start": start, "batch_size": c.n + 13}


def run_refs(c, mods, b):
    """(float64 reference, torch fp32 yardstick) of the minibatch of batch b on fp32 modules mods (left untouched)."""
    import torch
    rows = b["index"][b["start"]:b["start"] + c.n].astype(np.int64)
    adv64 = b["adv"].astype(np.float64)
    advn64 = (adv64 - adv64.mean()) / (adv64.std(ddof=1) + 1e-8)  # over the whole batch, like adv_stats
    advn32 = ((b["adv"] - b["adv"].mean()) / (b["adv"].std(ddof=1) + np.float32(1e-8))).astype(np.float32)
    T = torch.from_numpy
    out = []
    for dt, advn in ((torch.float64, advn64), (torch.float32, advn32)):
        pol, crit = (copy.deepcopy(m).to(dt) for m in mods)
        out.append(minibatch_ref(pol, crit, T(b["obs"][rows]).to(dt), T(b["masks"][rows]), T(b["acts"][rows]),
                                 T(b["old"][rows]).to(dt), T(advn[rows]).to(dt), T(b["tgt"][rows]).to(dt),
                                 b["batch_size"]))
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def case_data(name, seed=None):
    c = CASES[name]
    mods = build_modules(c, seed)
    b = build_batch(c, copy.deepcopy(mods[0]).double(), seed)
    r64, r32 = run_refs(c, mods, b)
    rows = b["index"][b["start"]:b["start"] + c.n]
    return {"case": c, "mods": mods, "batch": b, "r64": r64, "r32": r32, "rows": rows}


def assert_side_conditions(d):
    import torch
    why = side_conditions(d["case"], d["r64"], torch.from_numpy(d["batch"]["masks"][d["rows"]]))
    assert why is None, f"case {d['case'].name}: {why}"


# ------------------------------------------------------------------ CPU self-tests
def test_float64_reference_agrees_with_fp32_restatement():
    """minibatch_ref in float64 against test_ppo.ref_minibatch (fp32) on one default-shape batch, at fp32 accuracy:
    gradients normwise 1e-5 per tensor, the four shared metrics 1e-5."""
    import torch
    from test_ppo import flat_grads, make_batch, ref_minibatch
    from rlgpu.ppo import make_sequential
    torch.manual_seed(3)
    pol, crit = make_sequential(167, 90, (512, 512), True, 1.0), make_sequential(167, 1, (512, 512), True, 1.0)
    n = 300
    obs, masks, acts, old, adv, tgt = make_batch(np.random.default_rng(5), n)
    advn = ((adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)).astype(np.float32)
    T = torch.from_numpy
    p64, c64 = copy.deepcopy(pol).double(), copy.deepcopy(crit).double()
    want = ref_minibatch(pol, crit, T(obs), T(masks), T(acts), T(old), T(advn), T(tgt), 2 * n)
    g32 = flat_grads(pol, crit).double()
    ref = minibatch_ref(p64, c64, T(obs).double(), T(masks), T(acts), T(old).double(), T(advn).double(),
                        T(tgt).double(), 2 * n)
    o = 0
    for m in (pol, crit):
        for name, prm in m.named_parameters():
            a, b = ref["grads"][o:o + prm.numel()], g32[o:o + prm.numel()]
            o += prm.numel()
            assert (a - b).norm() <= 1e-5 * a.norm(), name
    assert o == ref["grads"].numel()
    for k, key in ((0, "entropy"), (2, "policy_loss"), (3, "critic_loss"), (4, "ratio")):
        assert abs(ref["metrics"][k] - want[key]) <= 1e-5 * max(1.0, abs(want[key])), key
    assert ref["metrics"][1] >= 0 and 0 <= ref["metrics"][5] <= 1
    assert len(ref["pre"]) == 4 and ref["pre"][0].shape == (n, 512)


@pytest.mark.parametrize("name", list(CASES))
def test_side_conditions_hold(name):
    """Every case's kink, clamp and clip margins, by the float64 reference alone; the sweep's features are present."""
    d = case_data(name)
    assert_side_conditions(d)
    c, b = d["case"], d["batch"]
    assert not np.array_equal(d["rows"], np.arange(c.n)) and b["start"] > 0 and b["batch_size"] != c.n
    m = d["r64"]["metrics"]
    if c.n >= 31:  # both clipped and unclipped rows
        assert 0 < m[5] < 1, m[5]
    if c.edge:
        rows, r = d["rows"], d["r64"]["ratio"]
        assert (b["masks"][rows[:8]].sum(1) == 1).all()
        assert (b["masks"][rows[8:20], b["acts"][rows[8:20]]] == 0).all()
        assert float(r.min()) < 0.6 and float(r.max()) > 1.8
        lg = d["r64"]["logits"]
        assert float(lg.max()) > 45 and float(lg.min()) < -45
        advr = b["adv"][rows]
        assert (advr > 0).any() and (advr < 0).any()
        legal = d["r64"]["raw_probs"][np.asarray(b["masks"][rows], bool)]
        assert (legal < 1e-11).any()  # the clamp engages on legal actions too
    if c.name == "smallvar":
        assert 1e-6 < first_linear_variance(d) < 1e-5  # against LayerNorm's eps = 1e-5


def first_linear_variance(d):
    """Mean over the minibatch rows of the biased variance of the policy's first Linear output (LayerNorm's input)."""
    import torch
    lin = d["mods"][0][0]
    with torch.no_grad():
        z = lin(torch.from_numpy(d["batch"]["obs"][d["rows"].astype(np.int64)]))
    return float(z.double().var(1, unbiased=False).mean())


def test_delta_covers_fp32():
    """DELTA is at least 10 x the largest pre-activation difference between the torch fp32 and the float64 forward
    over the case table (the kink cases: slope != 1)."""
    worst = 0.0
    for name, c in CASES.items():
        if c.slope == 1.0:
            continue
        d = case_data(name)
        worst = max(worst, max(float((a.double() - b).abs().max()) for a, b in zip(d["r32"]["pre"], d["r64"]["pre"])))
    assert 10 * worst <= DELTA, worst


def test_create_rejects_one_action():
    """num_actions = 1 has no distribution to learn and an infinite 1 / log(A): rlgpu_ppo_create names it, and
    accepts 2 (without a GPU that create fails later, on its first allocation, not on num_actions)."""
    import ctypes
    from rlgpu.ppo import _Cfg, _bind
    L = _bind()
    L.rlgpu_last_error.restype = ctypes.c_char_p
    cfg = _Cfg()
    cfg.obs_size, cfg.num_actions, cfg.max_rows = 167, 1, 64
    cfg.n_policy_layers = cfg.n_critic_layers = 1
    cfg.policy_layers[0] = cfg.critic_layers[0] = 64
    h = ctypes.c_void_p()
    assert L.rlgpu_ppo_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
    assert b"num_actions must be in [2, 128]" in L.rlgpu_last_error()
    cfg.num_actions = 2
    if L.rlgpu_ppo_create(ctypes.byref(cfg), ctypes.byref(h)) == 0:
        assert L.rlgpu_ppo_destroy(h) == 0
    else:
        assert b"num_actions" not in L.rlgpu_last_error()


@pytest.mark.parametrize("field", ["n_policy_layers", "n_critic_layers"])
def test_create_rejects_model_without_hidden_layers(field):
    """Every model has at least one hidden layer: rlgpu_ppo_create names a zero layer count, for the policy and for
    the critic (the training passes have no path for an output layer that reads the model input), before it
    allocates anything -- so this needs no GPU."""
    import ctypes
    from rlgpu.ppo import _Cfg, _bind
    L = _bind()
    L.rlgpu_last_error.restype = ctypes.c_char_p
    cfg = _Cfg()
    cfg.obs_size, cfg.num_actions, cfg.max_rows = 167, 90, 64
    cfg.n_policy_layers = cfg.n_critic_layers = 1
    cfg.policy_layers[0] = cfg.critic_layers[0] = 64
    setattr(cfg, field, 0)
    h = ctypes.c_void_p()
    assert L.rlgpu_ppo_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
    assert b"1..8 hidden layers per model" in L.rlgpu_last_error()


def test_scalar_floor_is_small():
    """No scalar is allowed more than 1e-4 of its scale, and the clip fraction less than half a row, at every n."""
    for c in list(CASES.values()) + [OPTIM]:
        assert scalar_floor(c.n, 1.0) < min(1e-4, 0.5 / c.n), c.name
    assert scalar_floor(10 ** 12, 1.0) == 1e-4


# ------------------------------------------------------------------ GPU
def ratio_of(err, floor, yard):
    """(err - floor) / yardstick, for a failure message."""
    return max(err - floor, 0.0) / yard if yard > 0 else (0.0 if err <= floor else float("inf"))


def make_engine(gpu, c, mods, mode, **kw):
    """A PPO of case c holding mods' parameters; torch_module gives them back bit for bit."""
    import torch
    from rlgpu.ppo import PPO
    p = PPO(obs_size=c.obs, num_actions=c.A, policy_layers=c.pol, critic_layers=c.crit, layer_norm=c.ln,
            leaky_slope=c.slope, clip_range=CLIP, entropy_scale=ENT_SCALE, max_rows=c.n + c.extra, seed=1, init=False,
            train_gemm=mode, device=gpu, **kw)
    for m in (0, 1):
        p.load_torch_module(m, mods[m])
        for a, b in zip(p.torch_module(m).parameters(), mods[m].parameters()):
            assert torch.equal(a, b)
    return p


def engine_minibatch(gpu, p, c, b):
    import torch
    D = {k: torch.from_numpy(b[k]).to(gpu) for k in ("obs", "masks", "acts", "old", "adv", "tgt", "index")}
    p.adv_normalizer(D["adv"])
    p.minibatch(D["obs"], D["masks"], D["acts"], D["old"], D["adv"], D["tgt"], D["index"], b["start"], c.n,
                b["batch_size"])
    torch.cuda.synchronize()
    return D


def check_grads(got, r64, r32, mods, mode, tag, n):
    o, bad = 0, []
    g64, g32 = r64["grads"], r32["grads"].double()
    for mi, m in enumerate(mods):
        for name, prm in m.named_parameters():
            k = prm.numel()
            g, w, t = got[o:o + k].double(), g64[o:o + k], g32[o:o + k]
            o += k
            err, yard, wn = float((g - w).norm()), float((t - w).norm()), float(w.norm())
            floor = 1e-7 * wn
            if k == 1:  # the rank-1 head's bias: a scalar, the sum of the rows' dv
                assert mi == 1 and name.endswith("bias")
                floor += scalar_floor(n, r64["head_bias_scale"])
            r = ratio_of(err, floor, yard)
            within = bool(((g - w).abs() <= 1e-3 * w.abs() + 1e-4 * w.abs().max()).all())
            if not (err <= factor(mode, n) * yard + floor and err <= 1e-4 * wn and within):
                bad.append(f"{('policy', 'critic')[mi]}.{name}: rel {err / (wn + 1e-300):.2e}, torch fp32 "
                           f"{yard / (wn + 1e-300):.2e}, ratio {r:.2f}, elementwise {within}")
    assert o == got.numel() == g64.numel()
    assert not bad, f"{tag}: " + "; ".join(bad)


def scalar_floor(n, scale):
    """K(n) * 2^-24 * S of a one-element result over n rows (module docstring)."""
    return min((4 + math.sqrt((n + 31) // 32)) * 2.0 ** -24, 1e-4) * abs(scale)


def check_metrics(p, r64, r32, mode, tag, n):
    got = p.metrics.cpu().double().numpy()[:6]
    names = ("entropy", "kl", "policy_loss", "critic_loss", "ratio", "clip_fraction")
    bad = []
    for k, nm in enumerate(names):
        err, yard = abs(got[k] - r64["metrics"][k]), abs(r32["metrics"][k] - r64["metrics"][k])
        floor = scalar_floor(n, r64["scales"][k])
        if not err <= factor(mode, n) * yard + floor:
            bad.append(f"{nm}: {got[k]:.9g} vs {r64['metrics'][k]:.9g}, err {err:.2e}, torch fp32 {yard:.2e}, floor "
                       f"{floor:.2e}, ratio {ratio_of(err, floor, yard):.2f}")
    assert not bad, f"{tag}: " + "; ".join(bad)


def check_forward(gpu, p, d, mode, tag):
    import torch
    obs = torch.from_numpy(d["batch"]["obs"])
    x = obs.to(gpu)
    bad = []
    for m, key in ((0, "logits"), (1, "values")):
        with torch.no_grad():
            w, t = copy.deepcopy(d["mods"][m]).double()(obs.double()), d["mods"][m](obs).double()
        got = p.forward(m, x).cpu().double()
        err, yard, wn = float((got - w).norm()), float((t - w).norm()), float(w.norm())
        if not err <= 4.0 * yard + 1e-7 * wn:
            bad.append(f"{key}: rel {err / wn:.2e}, torch fp32 {yard / wn:.2e}, ratio {ratio_of(err, 1e-7 * wn, yard):.2f}")
    assert not bad, f"{tag}: " + "; ".join(bad)


def run_case(gpu, name, mode):
    d = case_data(name)
    c = d["case"]
    assert_side_conditions(d)
    p = make_engine(gpu, c, d["mods"], mode)
    p.zero_grad()
    engine_minibatch(gpu, p, c, d["batch"])
    tag = f"{name}/{MODE_IDS[mode]}"
    errs = []
    for fn in (lambda: check_grads(p.flat(grads=True).cpu(), d["r64"], d["r32"], d["mods"], mode, tag, c.n),
               lambda: check_metrics(p, d["r64"], d["r32"], mode, tag, c.n),
               lambda: check_forward(gpu, p, d, mode, tag)):
        try:
            fn()
        except AssertionError as e:  # report every failing part of the case, not the first
            errs.append(str(e))
    p.close()
    assert not errs, "\n".join(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", [c.name for c in SWEEP])
def test_width_and_topology_sweep(gpu, name, mode):
    """One minibatch from zero_grad per case of SWEEP (the table's comments name the kernels) and GEMM mode: 37 rows
    (two blocks of the 16- and 32-row kernels with a ragged tail, more than two of the wide kernels' 4-row groups)
    through a non-identity index with a non-zero start into a batch of 64, batch_size != n; gradients, the six
    metrics and the fp32 forward of both models against float64."""
    run_case(gpu, name, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", [c.name for c in MANY])
def test_many_row_reductions(gpu, name, mode):
    """The two-level reduction (8161 rows) and the split-K cap (32771 rows), max_rows = n; slope 1.0 (see MANY)."""
    run_case(gpu, name, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_loss_kernel_edge_rows(gpu, mode):
    """64 rows with logits over about +-60: rows with a single legal action, rows whose stored action is masked (the
    clamped 1e-11 is gathered and passes no gradient), ratios near 0.5 and 2, advantages of both signs, legal
    actions under the clamp (test_side_conditions_hold asserts the batch has them)."""
    run_case(gpu, "edge", mode)


OPT = dict(policy_lr=1e-3, critic_lr=3e-4, weight_decay=0.05)
# Coordinates outside the tight band |d| <= 1e-4 |w| + 2e-6 (test_optimizer_step_matches_torch_adamw's): measured
# between torch fp32 and float64 AdamW on the CPU (test_optimizer_share_on_cpu) the share is 0 in both runs; the
# engine is allowed one coordinate in 10^4, that test's share, and no coordinate further than 0.1 lr.
OPT_SHARE = 1e-4


def optimizer_reference(max_norm, steps=2):
    """Two AdamW steps after clip_grad_norm_ in float64 and in torch fp32: per step the batches, the gradient norms
    (policy, critic) and the fp32 gradient error; the final flat parameters of both."""
    import torch
    c = OPTIM
    mods = build_modules(c)
    tr = {}
    for dt in (torch.float64, torch.float32):
        ms = [copy.deepcopy(m).to(dt) for m in mods]
        opts = [torch.optim.AdamW(ms[0].parameters(), lr=OPT["policy_lr"], weight_decay=OPT["weight_decay"]),
                torch.optim.AdamW(ms[1].parameters(), lr=OPT["critic_lr"], weight_decay=OPT["weight_decay"])]
        norms, grads, batches = [], [], []
        for it in range(steps):
            b = build_batch(c, copy.deepcopy(mods[0]).double(), seed=100 + it)
            rows = b["index"][b["start"]:b["start"] + c.n].astype(np.int64)
            adv = b["adv"].astype(np.float64)
            advn = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
            T = torch.from_numpy
            r = minibatch_ref(ms[0], ms[1], T(b["obs"][rows]).to(dt), T(b["masks"][rows]), T(b["acts"][rows]),
                              T(b["old"][rows]).to(dt), T(advn[rows]).to(dt), T(b["tgt"][rows]).to(dt), b["batch_size"])
            if dt == torch.float64:  # the clamp and clip margins of the batches these tests run (slope 1: no kink)
                why = side_conditions(c, r, T(b["masks"][rows]))
                assert why is None, f"optimizer step {it}: {why}"
            grads.append(r["grads"].double())
            norms.append([float(torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm)) for m in ms])
            for o in opts:
                o.step()
            batches.append(b)
        flat = torch.cat([q.detach().reshape(-1).double() for m in ms for q in m.parameters()])
        tr[dt] = {"norms": norms, "grads": grads, "flat": flat, "batches": batches}
    return mods, tr[torch.float64], tr[torch.float32]


def band(got, want):
    diff = (got - want).abs()
    return float((diff <= 1e-4 * want.abs() + 2e-6).double().mean()), float(diff.max())


@pytest.mark.parametrize("max_norm", [1e-3, 1e3])
def test_optimizer_share_on_cpu(max_norm):
    """The reference side of the optimizer test: max_grad_norm far below / far above the float64 gradient norms, and
    the share of coordinates where torch fp32 AdamW leaves the tight band around float64."""
    _, r64, r32 = optimizer_reference(max_norm)
    for pair in r64["norms"]:
        for nrm in pair:
            assert (nrm > 10 * max_norm) if max_norm < 1 else (nrm < 0.1 * max_norm), (nrm, max_norm)
    tight, worst = band(r32["flat"], r64["flat"])
    assert 1 - tight <= OPT_SHARE / 4 and worst < 0.1 * OPT["critic_lr"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("max_norm", [1e-3, 1e3])
def test_optimizer_clip_and_adamw(gpu, max_norm, mode):
    """Two optimizer steps with weight_decay 0.05 and learning rates 1e-3 / 3e-4, once with clip_grad_norm_ engaged
    (max_grad_norm 1e-3, far below the norms: the update then depends on Adam's eps) and once idle (1e3), against
    float64 torch.optim.AdamW + clip_grad_norm_.  The grad-norm metrics against the float64 norms: by the reverse
    triangle inequality within the gradient's own bound, plus 7e-7 for the fp32 sum of squares (its last level
    adds 512 partials in sequence, a random walk of sqrt(512) x 2^-24, halved by the square root; measured: 2.4e-7 at most)."""
    import torch
    mods, r64, r32 = optimizer_reference(max_norm)
    c = OPTIM
    for pair in r64["norms"]:
        for nrm in pair:
            assert (nrm > 10 * max_norm) if max_norm < 1 else (nrm < 0.1 * max_norm), (nrm, max_norm)
    p = make_engine(gpu, c, mods, mode, max_grad_norm=max_norm, **OPT)
    sizes = [sum(q.numel() for q in m.parameters()) for m in mods]
    for it, b in enumerate(r64["batches"]):
        engine_minibatch(gpu, p, c, b)
        p.optimizer_step()
        got = p.metrics.cpu().double().numpy()[7:9]
        g64, g32 = r64["grads"][it], r32["grads"][it]
        for m in (0, 1):
            sl = slice(0, sizes[0]) if m == 0 else slice(sizes[0], sizes[0] + sizes[1])
            want = r64["norms"][it][m]
            assert abs(float(g64[sl].norm()) - want) <= 1e-12 * want
            tol = 4.0 * float((g32[sl] - g64[sl]).norm()) + (1e-7 + 7e-7) * want
            assert abs(got[m] - want) <= tol, (it, m, got[m], want, tol)
    assert float(p.grads.abs().max()) == 0.0  # the step zeroes the gradients
    tight, worst = band(p.flat().cpu().double(), r64["flat"])
    assert 1 - tight <= OPT_SHARE, tight
    assert worst < 0.1 * OPT["critic_lr"], worst
    moved = (r64["flat"] - torch.cat([q.detach().reshape(-1).double() for m in mods for q in m.parameters()])).abs()
    assert float(moved.max()) > 1e-4  # the band is around parameters that moved
    p.close()

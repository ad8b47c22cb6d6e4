"""The float64 reference of rlgpu_ppo_minibatch and the rules an engine result is held to against it: one copy,
shared by test_ppo_variants, test_policy_options, test_guiding_policy and test_activations (which own their case
tables; the tables' comments name the kernels each case reaches).

The reference (minibatch_ref) is the PyTorch restatement of PPOLearner::Learn's minibatch body that
test_ppo.ref_minibatch is, generic in the dtype: run on float64 copies of the modules it is the reference, run
on the fp32 modules it is the yardstick -- the engine must be as close to float64 as torch's own fp32 is:

    per parameter tensor   ||g - g64|| <= F * ||g32 - g64|| + 1e-7 * ||g64||            (F = 4, see below)
                           ||g - g64|| <= 1e-4 * ||g64||                                 (the kink-free contract)
                           |g - g64|   <= 1e-3 * |g64| + 1e-4 * max |g64|  elementwise   (now at slope 0.01 too)
    forward outputs        the first rule on the logits and the values of every row of the batch
    one-element results    |m - m64| <= F * |m32 - m64| + K(n) * 2^-24 * S      (the six metrics, the guiding loss,
                           and the rank-1 head's bias gradient, a one-element tensor, on top of its tensor rule's floor)

The 4 and the 1e-7 are test_gemm_modes_fp32_class_accuracy's.  A one-element fp32 result has no usable
one-element yardstick: torch's own fp32 scalar lands within a fraction of an ulp of float64 as often as not (measured
here: 5e-10 relative on a clip fraction, 4e-9 on the head's bias gradient, where the engine was one ulp off), so a
scalar also gets a floor in units of u S, u = 2^-24:
  * S is what one rounding of a term's inputs moves the mean by: with z the legal (tempered) logits, zmax their
    largest magnitude and c = 1 + |z_action| + zmax + |old log prob|, ratio: mean(ratio c); KL: mean((ratio + 1) c);
    policy loss: mean(|adv| ratio c); entropy: mean(sum_k p_k (|log p_k| + 1)(1 + |z_k| + zmax)) / log A (per row
    log(legal count) with mask_entropy); critic loss: mean(2 |v - t| (|v| + |t|) + (v - t)^2) bsr; clip fraction: 1;
    head bias gradient: 2 bsr / n sum(|v| + |t|); guiding loss: mean over (row, action) of
    c_k (1 + |z_k| + zmax) + g_k (1 + |zg_k| + zgmax).
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
evaluated by the reference alone, on the CPU for every case (the *_side_conditions_hold tests) and again inside
each GPU test:

  * kink margin: with a LeakyReLU slope other than 1 every float64 pre-activation has |h| >= DELTA.  Measured on
    the CPU over test_ppo_variants' case table: the largest |h32 - h64| of a torch fp32 forward is 3.2e-6
    (test_delta_covers_fp32 recomputes it), 10 x that is 3.2e-5, rounded up to DELTA = 4.5e-5.
  * no legal action's float64 probability within 0.1 % of the 1e-11 clamp; no ratio within 1e-4 of 1 +- clip.
The seeds in the tables were searched on the CPU until every case passes.

The error ratios measured on an MI355X are written at factor() below.

The reference itself is pinned by tests/golden/ppo_reference.npz (check_golden): the float64 metrics, scales and
per parameter tensor ||g|| and g . u of every case, recorded from the three separate statements of the reference
(plain, with temperature / mask_entropy, with the guide) that minibatch_ref replaced.

This is a helper module: pytest does not rewrite its asserts, so every assert here carries its message.
"""
import copy
import functools
import math
import os
from typing import NamedTuple

import numpy as np

from tests_util import random_actions

CLIP, ENT_SCALE = 0.2, 0.035
DELTA = 4.5e-5  # kink margin, see the module docstring
MODES = [0, 1, 2]
MODE_IDS = ["x6", "f32", "h3"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_reference.npz")
GOLDEN_RTOL = 1e-10  # 10^5 x the float64 summation-order noise (4.8e-16), 1000 x below the tightest GPU floor (1e-7)


# The yardstick factor (4: test_gemm_modes_fp32_class_accuracy's).  Measured on an MI355X, the largest
# (err - floor) / (torch fp32 err) over test_ppo_variants, gradients / forward outputs: x6 1.52 / 0.63, f32 3.25 / 2.21,
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


def minibatch_ref(pol, crit, obs, masks, acts, old_logp, adv, target, batch_size, *, temperature=1.0,
                  mask_entropy=False, guide_logits=None, strength=0.0, clip=CLIP, ent_scale=ENT_SCALE):
    """PPOLearner::Learn's minibatch body (PPOLearner.cpp:341-498) in the dtype of the modules and inputs; from
    zeroed gradients.  With PPOLearnerConfig::policyTemperature (:411-415: the softmax runs on logits / temperature),
    maskEntropy (:426-438: each row's entropy over log(the row's legal actions) instead of log A) and, where
    guide_logits [n, A] (in the dtype of obs) is given, the guiding term strength * mean |g - c| (:458-468) with g the
    guide's clamped masked softmax of (guide logits / temperature) and c the trained policy's clamped probabilities.
    Returns the flat gradients (policy, then critic: the engine's order), the six metrics (entropy, KL, policy loss,
    critic loss, mean ratio, clip fraction; KL = mean(exp(lr) - 1 - lr), clip fraction = mean(|ratio - 1| > clip),
    :484-489), the rounding scale of each metric (module docstring), every pre-activation, the outputs, the
    unclamped probabilities and the ratios; with a guide also the guiding loss and its rounding scale, c, g and g
    unclamped."""
    import torch
    for m in (pol, crit):
        m.zero_grad(set_to_none=True)
    n = obs.shape[0]
    bsr = n / float(batch_size)
    logits, pre_p = run_seq(pol, obs)
    tl = logits / temperature
    raw, probs = masked_probs(tl, masks)
    logp = probs.gather(-1, acts.long().unsqueeze(-1)).squeeze(-1).log()
    # the entropy's divisor: log A, or per row log(legal actions) (no guard: log 1 = 0 as in the reference)
    log_cnt = masks.to(obs.dtype).sum(-1).log() if mask_entropy else math.log(probs.shape[1])
    ent = (-(probs.log() * probs).sum(-1) / log_cnt).mean()
    lr = logp - old_logp
    ratio = lr.exp()
    clipped = ratio.clamp(1 - clip, 1 + clip)
    terms = torch.min(ratio * adv, clipped * adv)
    pl = -terms.mean()
    vals, pre_c = run_seq(crit, obs)
    vals = vals.flatten()
    closs = torch.nn.functional.mse_loss(vals, target) * bsr
    ppo_loss = (pl - ent * ent_scale) * bsr
    if guide_logits is not None:
        with torch.no_grad():  # the guide: no gradient (PPOLearner.cpp:459 runs it under NoGradGuard)
            gl = guide_logits / temperature
            graw, gprobs = masked_probs(gl, masks)
        guiding = (gprobs - probs).abs().mean()
        # ppoLoss += guidingLoss * guidingStrength after the batch-size-ratio scaling (PPOLearner.cpp:466-468)
        ppo_loss = ppo_loss + guiding * strength
    (ppo_loss + closs).backward()
    kl = (lr.exp() - 1 - lr).mean()
    frac = ((ratio - 1).abs() > clip).to(obs.dtype).mean()
    f = lambda t: float(t.detach().double())  # noqa: E731
    # what one rounding of the inputs of each metric's terms moves the metric by (module docstring)
    with torch.no_grad():
        tl = tl.detach()
        legal = masks.bool()
        z = tl + -1e10 * legal.logical_not()
        zm = z.max(-1).values.abs()
        ai = acts.long().unsqueeze(-1)
        legal_a = legal.gather(-1, ai).squeeze(-1)  # a masked action's log prob is log(1e-11) exactly
        lcond = 1 + (tl.gather(-1, ai).squeeze(-1).abs() + zm) * legal_a + old_logp.abs()
        zc = 1 + tl.abs() * legal + zm.unsqueeze(-1)
        s_ent = ((probs * (probs.log().abs() + 1) * zc).sum(-1) / log_cnt).mean()
        s_crit = ((2 * (vals - target).abs() * (vals.abs() + target.abs()) + (vals - target) ** 2).mean()) * bsr
        s_head = 2 * bsr / n * (vals.abs() + target.abs()).sum()
    out = {"grads": torch.cat([p.grad.reshape(-1) for m in (pol, crit) for p in m.parameters()]).clone(),
           "metrics": np.array([f(ent), f(kl), f(pl), f(closs), f(ratio.mean()), f(frac)]),
           "scales": np.array([f(s_ent), f(((ratio + 1) * lcond).mean()), f((adv.abs() * ratio * lcond).mean()),
                               f(s_crit), f((ratio * lcond).mean()), 1.0]),
           "head_bias_scale": f(s_head),
           "pre": pre_p + pre_c, "logits": logits.detach(), "values": vals.detach(), "raw_probs": raw.detach(),
           "ratio": ratio.detach()}
    if guide_logits is not None:
        with torch.no_grad():
            zgm = (gl + -1e10 * legal.logical_not()).max(-1).values.abs()
            zgc = 1 + gl.abs() * legal + zgm.unsqueeze(-1)
            s_guide = (probs * zc + gprobs * zgc).mean()
        out.update(guiding=f(guiding), guide_scale=f(s_guide), probs=probs.detach(), gprobs=gprobs.detach(),
                   graw=graw.detach())
    return out


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


def swap_activation(seq, act):
    """seq with every LeakyReLU replaced by Sigmoid / Tanh (the parameters untouched)."""
    import torch
    new = {"sigmoid": torch.nn.Sigmoid, "tanh": torch.nn.Tanh}[act]
    return torch.nn.Sequential(*[new() if isinstance(m, torch.nn.LeakyReLU) else m for m in seq])


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


def build_option_batch(c, pol64, temperature):
    """build_batch, then (1) every row with a single legal action gets a second one (the next column), and (2) the
    old log probs are rebuilt as the tempered float64 log prob plus build_batch's noise (recovered as its old log
    prob minus its float64 log prob), so the ratios still straddle the clip range."""
    import torch
    b = build_batch(c, pol64)
    with torch.no_grad():
        logits = pol64(torch.from_numpy(b["obs"]).double())
        ai = torch.from_numpy(b["acts"]).long().unsqueeze(-1)
        _, probs = masked_probs(logits, torch.from_numpy(b["masks"]))
        noise = b["old"].astype(np.float64) - probs.gather(-1, ai).squeeze(-1).log().numpy()
        one = np.nonzero(b["masks"].sum(1) == 1)[0]
        b["masks"][one, (b["masks"][one].argmax(1) + 1) % c.A] = 1
        _, probs = masked_probs(logits / temperature, torch.from_numpy(b["masks"]))
        lp = probs.gather(-1, ai).squeeze(-1).log().numpy()
    b["old"] = (lp + noise).astype(np.float32)
    return b


def guide_stream(c, gscale, fp16, seed_offset=0):
    """(bits uint16 [B, A], values f32 [B, A]) of the case's guide logits: N(0, 1) * gscale from the stream
    4242 + c.seed, rounded to nearest even into bf16 (fp16: numpy's own rounding)."""
    rng = np.random.default_rng(4242 + c.seed + seed_offset)
    x = (rng.standard_normal((c.n + c.extra, c.A)) * gscale).astype(np.float32)
    if fp16:
        h = x.astype(np.float16)
        return h.view(np.uint16).copy(), h.astype(np.float32)
    u = x.view(np.uint32)
    bits = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return bits, (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def minibatch_rows(c, b):
    """The batch rows of the minibatch, in its order."""
    return b["index"][b["start"]:b["start"] + c.n]


def run_refs(c, mods, b, *, guide_logits=None, **options):
    """(float64 reference, torch fp32 yardstick) of the minibatch of batch b on fp32 modules mods (left untouched);
    options: minibatch_ref's.  guide_logits: the whole batch's f32 [B, A] array, of which the minibatch's rows are
    taken."""
    import torch
    rows = minibatch_rows(c, b).astype(np.int64)
    adv64 = b["adv"].astype(np.float64)
    advn64 = (adv64 - adv64.mean()) / (adv64.std(ddof=1) + 1e-8)  # over the whole batch, like adv_stats
    advn32 = ((b["adv"] - b["adv"].mean()) / (b["adv"].std(ddof=1) + np.float32(1e-8))).astype(np.float32)
    T = torch.from_numpy
    out = []
    for dt, advn in ((torch.float64, advn64), (torch.float32, advn32)):
        pol, crit = (copy.deepcopy(m).to(dt) for m in mods)
        if guide_logits is not None:
            options["guide_logits"] = T(guide_logits[rows]).to(dt)
        out.append(minibatch_ref(pol, crit, T(b["obs"][rows]).to(dt), T(b["masks"][rows]), T(b["acts"][rows]),
                                 T(b["old"][rows]).to(dt), T(advn[rows]).to(dt), T(b["tgt"][rows]).to(dt),
                                 b["batch_size"], **options))
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def build_case(c, *, seed=None, act=None, temperature=1.0, mask_entropy=False, guide=None):
    """Case c's modules (act: every LeakyReLU swapped for "sigmoid" / "tanh"), batch, float64 reference and torch fp32
    yardstick, computed once and shared: treat the result as read-only.  Without the options the batch is
    build_batch's and keeps its rows with a single legal action; with a temperature or mask_entropy it is
    build_option_batch's (every row has two legal actions: mask_entropy divides by log(legal); the old log probs are
    the tempered ones).  guide = (gscale, fp16, strength): guide_stream's logits enter the reference at that strength."""
    mods = build_modules(c, seed)
    if act is not None:
        mods = [swap_activation(m, act) for m in mods]
    pol64 = copy.deepcopy(mods[0]).double()
    plain = temperature == 1.0 and not mask_entropy
    b = build_batch(c, pol64, seed) if plain else build_option_batch(c, pol64, temperature)
    d = {"case": c, "mods": mods, "batch": b, "rows": minibatch_rows(c, b), "temperature": temperature,
         "mask_entropy": mask_entropy}
    options = dict(temperature=temperature, mask_entropy=mask_entropy)
    if guide is not None:
        gscale, fp16, strength = guide
        d["bits"], d["gvals"] = guide_stream(c, gscale, fp16)
        options.update(guide_logits=d["gvals"], strength=strength)
    d["r64"], d["r32"] = run_refs(c, mods, b, **options)
    return d


def param_tensors(mods):
    """(label, offset into the flat gradient, numel) of every parameter tensor, policy then critic."""
    o, out = 0, []
    for mi, m in enumerate(mods):
        for name, prm in m.named_parameters():
            out.append((f"{('policy', 'critic')[mi]}.{name}", o, prm.numel()))
            o += prm.numel()
    return out


# ------------------------------------------------------------------ the golden pin of the reference
def golden_record(r64, mods):
    """What tests/golden/ppo_reference.npz keeps of a float64 reference result: the scalars, and per parameter tensor
    ||g|| and g . u with u a unit vector from np.random.default_rng(31337 + tensor index)."""
    rec = {"metrics": r64["metrics"], "scales": r64["scales"], "head_bias_scale": np.float64(r64["head_bias_scale"])}
    if "guiding" in r64:
        rec.update(guiding=np.float64(r64["guiding"]), guide_scale=np.float64(r64["guide_scale"]))
    g = r64["grads"].numpy()
    assert g.dtype == np.float64, f"the golden record is of the float64 reference, not {g.dtype}"
    norms, projs = [], []
    for i, (_, o, k) in enumerate(param_tensors(mods)):
        u = np.random.default_rng(31337 + i).standard_normal(k)
        norms.append(np.linalg.norm(g[o:o + k]))
        projs.append(g[o:o + k] @ (u / np.linalg.norm(u)))
    rec.update(grad_norm=np.array(norms), grad_proj=np.array(projs))
    return rec


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def check_golden(key, d):
    """The float64 reference of case data d against its record `key` in the golden file: every scalar within
    1e-10 * max(|value|, its rounding scale), the clip fraction exactly, every tensor's norm and projection within
    1e-10 * ||g||."""
    want = {k[len(key) + 1:]: v for k, v in _golden().items() if k.startswith(key + ":")}
    got = golden_record(d["r64"], d["mods"])
    assert want and set(got) == set(want), f"{key}: recorded {sorted(want)}, computed {sorted(got)}"
    bad = []

    def close(name, a, w, scale):
        if not abs(a - w) <= GOLDEN_RTOL * max(abs(w), scale):
            bad.append(f"{name}: {a!r} vs recorded {w!r}")

    names = ("entropy", "kl", "policy_loss", "critic_loss", "ratio")
    for k, nm in enumerate(names):
        close(nm, got["metrics"][k], want["metrics"][k], want["scales"][k])
    if got["metrics"][5] != want["metrics"][5]:
        bad.append(f"clip_fraction: {got['metrics'][5]!r} vs recorded {want['metrics'][5]!r}")
    for k, nm in enumerate(names + ("clip_fraction",)):
        close(f"scale of {nm}", got["scales"][k], want["scales"][k], want["scales"][k])
    close("head_bias_scale", got["head_bias_scale"], want["head_bias_scale"], want["head_bias_scale"])
    if "guiding" in want:
        close("guiding", got["guiding"], want["guiding"], want["guide_scale"])
        close("guide_scale", got["guide_scale"], want["guide_scale"], want["guide_scale"])
    tensors = param_tensors(d["mods"])
    assert len(tensors) == len(want["grad_norm"]) == len(got["grad_norm"]), f"{key}: parameter tensor count"
    for i, (label, _, _) in enumerate(tensors):
        for what in ("grad_norm", "grad_proj"):
            if not abs(got[what][i] - want[what][i]) <= GOLDEN_RTOL * want["grad_norm"][i]:
                bad.append(f"{label} {what}: {got[what][i]!r} vs recorded {want[what][i]!r}")
    assert not bad, f"{key}: " + "; ".join(bad)


# ------------------------------------------------------------------ the engine side
def make_engine(gpu, c, mods, mode, **kw):
    """A PPO of case c holding mods' parameters; torch_module gives them back bit for bit."""
    import torch
    from rlgpu.ppo import PPO
    p = PPO(obs_size=c.obs, num_actions=c.A, policy_layers=c.pol, critic_layers=c.crit, layer_norm=c.ln,
            leaky_slope=c.slope, clip_range=CLIP, entropy_scale=ENT_SCALE, max_rows=c.n + c.extra, seed=1, init=False,
            train_gemm=mode, device=gpu, **kw)
    for m in (0, 1):
        p.load_torch_module(m, mods[m])
        for (name, a), b in zip(p.torch_module(m).named_parameters(), mods[m].parameters()):
            assert torch.equal(a, b), f"model {m}: {name} read back from the engine differs from what was loaded"
    return p


def engine_minibatch(gpu, p, c, b, guide=None, strength=0.0):
    """adv_normalizer and one minibatch of batch b on engine p (guide: the 16-bit guide logits of the whole batch, on
    the device); the batch's device tensors."""
    import torch
    D = {k: torch.from_numpy(b[k]).to(gpu) for k in ("obs", "masks", "acts", "old", "adv", "tgt", "index")}
    kw = {} if guide is None else dict(guide_logits=guide, guiding_strength=strength)
    p.adv_normalizer(D["adv"])
    p.minibatch(D["obs"], D["masks"], D["acts"], D["old"], D["adv"], D["tgt"], D["index"], b["start"], c.n,
                b["batch_size"], **kw)
    torch.cuda.synchronize()
    return D


# ------------------------------------------------------------------ the rules
def ratio_of(err, floor, yard):
    """(err - floor) / yardstick, for a failure message."""
    return max(err - floor, 0.0) / yard if yard > 0 else (0.0 if err <= floor else float("inf"))


def scalar_floor(n, scale):
    """K(n) * 2^-24 * S of a one-element result over n rows (module docstring)."""
    return min((4 + math.sqrt((n + 31) // 32)) * 2.0 ** -24, 1e-4) * abs(scale)


def one_element(name, got, want64, want32, scale, mode, n):
    """The one-element rule |m - m64| <= F |m32 - m64| + K(n) 2^-24 S: (whether it holds, the figures)."""
    err, yard = abs(got - want64), abs(want32 - want64)
    floor = scalar_floor(n, scale)
    return err <= factor(mode, n) * yard + floor, (
        f"{name}: {got:.9g} vs {want64:.9g}, err {err:.2e}, torch fp32 {yard:.2e}, floor {floor:.2e}, ratio "
        f"{ratio_of(err, floor, yard):.2f}")


def check_grads(got, r64, r32, mods, mode, tag, n, grad_factor=None):
    """The three per-tensor rules; grad_factor: the first rule's F for this case instead of factor(mode, n)."""
    F = factor(mode, n) if grad_factor is None else grad_factor
    bad = []
    g64, g32 = r64["grads"], r32["grads"].double()
    tensors = param_tensors(mods)
    for label, o, k in tensors:
        g, w, t = got[o:o + k].double(), g64[o:o + k], g32[o:o + k]
        err, yard, wn = float((g - w).norm()), float((t - w).norm()), float(w.norm())
        floor = 1e-7 * wn
        if k == 1:  # the rank-1 head's bias: a scalar, the sum of the rows' dv
            assert label.startswith("critic.") and label.endswith("bias"), f"{tag}: one-element tensor {label}"
            floor += scalar_floor(n, r64["head_bias_scale"])
        r = ratio_of(err, floor, yard)
        within = bool(((g - w).abs() <= 1e-3 * w.abs() + 1e-4 * w.abs().max()).all())
        if not (err <= F * yard + floor and err <= 1e-4 * wn and within):
            bad.append(f"{label}: rel {err / (wn + 1e-300):.2e}, torch fp32 {yard / (wn + 1e-300):.2e}, ratio {r:.2f}, "
                       f"elementwise {within}")
    end = tensors[-1][1] + tensors[-1][2]
    assert end == got.numel() == g64.numel(), f"{tag}: {end} parameters, {got.numel()} gradients, {g64.numel()} expected"
    assert not bad, f"{tag}: " + "; ".join(bad)


def check_metrics(p, r64, r32, mode, tag, n):
    got = p.metrics.cpu().double().numpy()[:6]
    names = ("entropy", "kl", "policy_loss", "critic_loss", "ratio", "clip_fraction")
    res = [one_element(nm, got[k], r64["metrics"][k], r32["metrics"][k], r64["scales"][k], mode, n)
           for k, nm in enumerate(names)]
    assert all(ok for ok, _ in res), f"{tag}: " + "; ".join(figures for ok, figures in res if not ok)


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


def run_engine_case(gpu, d, mode, tag, *, engine_kw=(), guide=None, grad_factor=None, extra_checks=(),
                    around_minibatch=None):
    """One minibatch from zero_grad of case data d on an engine in GEMM mode `mode` (engine_kw: further PPO arguments;
    guide: (16-bit guide logits on the device, guiding strength)), then check_grads (grad_factor: its factor for this
    case; the metric and forward rules keep factor(mode, n)), check_metrics, check_forward and every extra_checks(p),
    reporting every failing part of the case, not the first.  around_minibatch(p, "before" / "after") brackets the
    minibatch."""
    c = d["case"]
    p = make_engine(gpu, c, d["mods"], mode, **dict(engine_kw))
    p.zero_grad()
    if around_minibatch:
        around_minibatch(p, "before")
    engine_minibatch(gpu, p, c, d["batch"], *(guide or ()))
    if around_minibatch:
        around_minibatch(p, "after")
    errs = []
    for fn in (lambda p: check_grads(p.flat(grads=True).cpu(), d["r64"], d["r32"], d["mods"], mode, tag, c.n, grad_factor),
               lambda p: check_metrics(p, d["r64"], d["r32"], mode, tag, c.n),
               lambda p: check_forward(gpu, p, d, mode, tag), *extra_checks):
        try:
            fn(p)
        except AssertionError as e:
            errs.append(str(e))
    p.close()
    assert not errs, "\n".join(errs)

"""The float64 reference of transfer learning (Learner::StartTransferLearn) and its case table: PPOLearner::TransferLearn
(PPOLearner.cpp:583-637) with InferPolicyProbsFromModels (:78-114) and ComputeEntropy (:253-276), restated in torch and
generic in the dtype -- on float64 copies of the modules it is the reference, on the fp32 modules the yardstick, under
ppo_reference's rules (check_grads, one_element) unchanged.  Modules, batches, the engine and the rules come from
ppo_reference; nothing there is changed.

What the reference takes as given: the teacher's logits.  The engine runs the teacher's forward on its inference path
(16-bit by default), so a float64 forward of the teacher would differ from it at the 1e-2 level; the teacher's output
enters transfer_ref as logits that are exact values of the handle's 16-bit format (guide_stream's rounding), either a
numpy stream or -- the case with a teacher of other widths -- the fp32 forward of a CPU teacher module rounded to
bf16.  Everything after the forward (temperature, mask, softmax, clamp, entropy, gather, argmax, the loss, its
backward, the optimiser) is the reference's.

transfer_ref's metrics are the four the reference reports from epoch 0: loss, accuracy, the student's entropy, the
teacher's entropy.  Their rounding scales S for the one-element rule, each "what one rounding of a term's inputs moves
the mean by" as in ppo_reference: with zc = 1 + |z_k| + zmax of the student's legal tempered logits and zo the same of
the teacher's (gathered),
    loss       loss_scale * mean(e t^(e-1) dt + t^e), dt = c zc + o zo   (L1)
                                                      dt = (|log(o / c)| + 1) o zo + o zc   (KL: d t = |log| do + o (do / o + dc / c))
    entropies  mean over rows of sum_k p_k (|log p_k| + 1) zc / log(count)   (minibatch_ref's entropy scale)
    accuracy   1; the tests hold it exactly.

Golden record: tests/golden/transfer_reference.npz (tests/golden/make_transfer_reference_golden.py), checked at
ppo_reference.GOLDEN_RTOL.

This is a helper module: pytest does not rewrite its asserts, so every assert here carries its message.
"""
import copy
import functools
import math
import os
from typing import NamedTuple, Optional

import numpy as np

from ppo_reference import GOLDEN_RTOL, Case, build_modules, masked_probs, run_seq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transfer_reference.npz")
CLAMP, CLAMP_MARGIN = 1e-11, 1e-3  # ACTION_MIN_PROB and side_conditions' 0.1 % distance from it


class TCase(NamedTuple):
    case: Case                  # the student: obs, A, policy widths, rows (crit: the unused critic)
    temperature: float = 1.0
    mask_entropy: bool = False
    use_kl: bool = False
    exponent: float = 1.0
    loss_scale: float = 1.0
    fp16: bool = False          # the handles' 16-bit format (the teacher's logits are rounded to it)
    shared: tuple = ()          # the student's shared head
    gscale: float = 1.0         # the teacher logit stream's scale
    a_old: Optional[int] = None  # the teacher's action count with an action map (None: A, no map)
    teacher: tuple = ()         # widths of a CPU teacher module whose bf16-rounded forward gives the logits
    max_rows: Optional[int] = None  # the engine's max_rows when the batch is to run in chunks
    two_legal: bool = False     # every row gets at least two legal actions (mask_entropy divides by log(legal))


_ROWS = dict(obs=167, A=90, pol=(96, 33), crit=(16,), seed=0, extra=0)
CASES = {
    # loss<1>, ldd 2 -> 4: rows with one legal action (c = o = 1 exactly); L1, e = 1
    "a2": TCase(Case("a2", 167, 2, (33, 65), (16,), seed=0, extra=0), gscale=8.0),
    # loss<2>, ldd 17 -> 20; KL, e = 2, T < 1
    "b17": TCase(Case("b17", 168, 17, (64, 128), (16,), seed=1, extra=0), temperature=0.7, use_kl=True, exponent=2.0),
    # loss<6>, ldd 90 -> 92: the 1-row and 33-row block edges and two blocks with a ragged tail
    "rows1": TCase(Case("rows1", n=1, **_ROWS), temperature=0.7, use_kl=True, gscale=4.0),
    "rows33": TCase(Case("rows33", n=33, **_ROWS), temperature=2.5, exponent=2.0, loss_scale=3.0),
    "rows37": TCase(Case("rows37", n=37, **_ROWS), temperature=2.5, mask_entropy=True, two_legal=True, use_kl=True,
                    exponent=2.0, loss_scale=0.5),
    # loss<8>, ldd 128 unpadded; mask_entropy
    "a128": TCase(Case("a128", 168, 128, (130, 64), (16,), seed=0, extra=0), temperature=2.5, mask_entropy=True,
                  two_legal=True, exponent=2.0),
    # an fp16 handle: the teacher's logits are fp16 values
    "rows37_f16": TCase(Case("rows37", n=37, **_ROWS), temperature=0.7, fp16=True, gscale=4.0),
    # a shared-head student: the head's backward from the policy's input gradient alone
    "shared": TCase(Case("shared", 167, 90, (96, 33), (16,), seed=9, n=37, extra=0), shared=(64,), use_kl=True),
    # a teacher of other widths: a CPU module [48] whose bf16-rounded forward is the teacher's logits
    "teacher48": TCase(Case("teacher48", 167, 90, (32, 32), (16,), seed=3, n=37, extra=0), teacher=(48,), temperature=0.7),
    # an action map, A_old = 23 -> A = 17, permuted with repeats
    "map23": TCase(Case("map23", 168, 17, (64, 128), (16,), seed=4, extra=0), a_old=23, temperature=0.7, exponent=2.0,
                   two_legal=True),
    # 70 rows through max_rows = 32: three chunks that must sum to the whole-batch gradient
    "chunked": TCase(Case("chunked", n=70, **dict(_ROWS, seed=5)), max_rows=32, temperature=2.5, use_kl=True),
}


# ------------------------------------------------------------------ the reference
def compute_entropy(probs, masks, mask_entropy):
    """ComputeEntropy (PPOLearner.cpp:253-276): mean over rows of -(log p * p).sum / log A, or / log(legal actions)."""
    ent = -(probs.log() * probs).sum(-1)
    div = masks.to(probs.dtype).sum(-1).log() if mask_entropy else math.log(masks.shape[-1])
    return (ent / div).mean()


def _entropy_scale(probs, tl, masks, mask_entropy):
    """minibatch_ref's rounding scale of an entropy metric."""
    legal = masks.bool()
    z = tl + -1e10 * legal.logical_not()
    zc = 1 + tl.abs() * legal + z.max(-1).values.abs().unsqueeze(-1)
    div = masks.to(probs.dtype).sum(-1).log() if mask_entropy else math.log(masks.shape[-1])
    return ((probs * (probs.log().abs() + 1) * zc).sum(-1) / div).mean(), zc


def transfer_ref(pol, shared, obs, masks, old_logits, old_masks, action_map, *, temperature=1.0, mask_entropy=False,
                 use_kl=False, loss_scale=1.0, exponent=1.0):
    """Epoch 0 of PPOLearner::TransferLearn in the dtype of the modules and inputs, from zeroed gradients: the teacher's
    clamped probabilities from old_logits [n, A_old] (no gradient), their entropy, the gather by action_map (int64
    [n, A] or None), the student's probabilities through shared (or None) and pol, the loss, backward().  Returns the
    flat gradients (policy, then the shared head's), the metrics (loss, accuracy, entropy, old entropy) and their
    scales, every pre-activation, and the probabilities of both sides (clamped and raw; the teacher's gathered)."""
    import torch
    mods = [m for m in (pol, shared) if m is not None]
    for m in mods:
        m.zero_grad(set_to_none=True)
    pre = []
    with torch.no_grad():
        otl = old_logits / temperature
        oraw, oprobs = masked_probs(otl, old_masks)
        old_ent = compute_entropy(oprobs, old_masks, mask_entropy)
        s_old, ozc = _entropy_scale(oprobs, otl, old_masks, mask_entropy)
        if action_map is not None:
            oprobs, oraw, ozc = oprobs.gather(1, action_map), oraw.gather(1, action_map), ozc.gather(1, action_map)
    x = obs
    if shared is not None:
        x, p0 = run_seq(shared, x)
        pre += p0
    logits, p1 = run_seq(pol, x)
    pre += p1
    tl = logits / temperature
    raw, probs = masked_probs(tl, masks)
    if use_kl:
        t = (oprobs * torch.log(oprobs / probs)).abs()
    else:
        t = (oprobs - probs).abs()
    loss = t.pow(exponent).mean() * loss_scale
    with torch.no_grad():
        acc = (probs.argmax(-1) == oprobs.argmax(-1)).to(obs.dtype).mean()
        ent = compute_entropy(probs, masks, mask_entropy)
        s_ent, zc = _entropy_scale(probs, tl.detach(), masks, mask_entropy)
        td = t.detach()
        if use_kl:
            dt = (torch.log(oprobs / probs).abs() + 1) * oprobs * ozc + oprobs * zc
        else:
            dt = probs * zc + oprobs * ozc
        s_loss = abs(loss_scale) * (exponent * td.pow(exponent - 1) * dt + td.pow(exponent)).mean()
    loss.backward()
    f = lambda v: float(v.detach().double())  # noqa: E731
    return {"grads": torch.cat([p.grad.reshape(-1) for m in mods for p in m.parameters()]).clone(),
            "metrics": np.array([f(loss), f(acc), f(ent), f(old_ent)]),
            "scales": np.array([f(s_loss), 1.0, f(s_ent), f(s_old)]),
            "pre": pre, "logits": logits.detach(), "raw_probs": raw.detach(), "probs": probs.detach(),
            "oprobs": oprobs, "oraw": oraw, "ratio": torch.ones(1, dtype=obs.dtype), "head_bias_scale": 0.0}


def transfer_epochs_ref(pol, shared, obs, masks, old_logits, old_masks, action_map, *, epochs, lr, betas=(0.9, 0.999),
                        eps=1e-8, weight_decay=1e-2, start_step=0, **options):
    """The epoch loop with StepOptims (AdamW at tlConfig.lr on the policy and the shared head, zero_grad after the
    step, no gradient clipping), in place on the modules.  start_step: the optimisers' step count before the first
    epoch, with zero moments (an engine whose count was set).  Returns the loss of every epoch."""
    import torch
    mods = [m for m in (pol, shared) if m is not None]
    opts = [torch.optim.AdamW(m.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay) for m in mods]
    if start_step:
        for o in opts:
            for q in o.param_groups[0]["params"]:
                o.state[q] = {"step": torch.tensor(float(start_step)), "exp_avg": torch.zeros_like(q),
                              "exp_avg_sq": torch.zeros_like(q)}
    losses = []
    for _ in range(epochs):
        r = transfer_ref(pol, shared, obs, masks, old_logits, old_masks, action_map, **options)
        losses.append(r["metrics"][0])
        for o in opts:
            o.step()
            o.zero_grad(set_to_none=True)
    return losses


# ------------------------------------------------------------------ the cases
def round16(x, fp16):
    """x (f32) rounded to the nearest value of the 16-bit format, as f32 (bf16: ties to even, guide_stream's rule)."""
    x = np.ascontiguousarray(x, np.float32)
    if fp16:
        return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32)
    bits = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint32)
    return (bits << np.uint32(16)).view(np.float32)


def build_transfer_batch(t):
    """obs, the student's masks, the teacher's logits and masks, and the action map of case t (numpy; every row of the
    batch is trained: there is no index).  With a map the student's masks are the gathered teacher's, so a masked
    column is masked on both sides."""
    import torch
    c = t.case
    rng = np.random.default_rng(104729 * c.seed + 31 + c.n)
    n, A = c.n, c.A
    a_old = t.a_old or A
    obs = (rng.standard_normal((n, c.obs)) * c.obs_scale).astype(np.float32)
    old_masks = (rng.random((n, a_old)) < 0.6).astype(np.uint8)
    old_masks[np.arange(n), rng.integers(a_old, size=n)] = 1
    amap = None
    if t.a_old:
        amap = np.stack([rng.permutation(a_old)[:A] for _ in range(n)]).astype(np.int32)
        rep = rng.integers(A, size=(n, 3))  # repeats: three columns of every row copy another column's source
        for k in range(3):
            amap[np.arange(n), rep[:, k]] = amap[np.arange(n), (rep[:, k] + 1 + k) % A]
        for i in range(n):  # at least two legal gathered columns
            while old_masks[i][amap[i]].sum() < 2:
                old_masks[i, amap[i, rng.integers(A)]] = 1
        masks = np.take_along_axis(old_masks, amap.astype(np.int64), 1)
    else:
        if t.two_legal:
            one = np.nonzero(old_masks.sum(1) == 1)[0]
            old_masks[one, (old_masks[one].argmax(1) + 1) % a_old] = 1
        masks = old_masks.copy()
    if t.teacher:
        tc = Case(c.name + "_teacher", c.obs, a_old, t.teacher, (16,), seed=c.seed + 50, ln=c.ln, slope=c.slope)
        with torch.no_grad():
            lg = build_modules(tc)[0](torch.from_numpy(obs)).numpy()
    else:
        lg = (rng.standard_normal((n, a_old)) * t.gscale).astype(np.float32)
    return {"obs": obs, "masks": masks, "old_masks": old_masks, "old_logits": round16(lg, t.fp16), "map": amap}


def build_student(t):
    """(policy, shared head or None) fp32 modules of case t: behind a shared head the policy reads its last width."""
    c = t.case
    if not t.shared:
        return build_modules(c)[0], None
    pol = build_modules(c._replace(obs=t.shared[-1]))[0]
    # the head: hidden layers only (make_sequential with out=None), filled like build_modules' layers
    import torch
    from rlgpu.ppo import make_sequential
    rng = np.random.default_rng(2000 + c.seed)
    head = make_sequential(c.obs, None, t.shared, c.ln, c.slope)
    with torch.no_grad():
        for m in head:
            if isinstance(m, torch.nn.Linear):
                bound = 1.0 / math.sqrt(m.in_features)
                m.weight.copy_(torch.from_numpy(rng.uniform(-bound, bound, m.weight.shape).astype(np.float32)))
                m.bias.copy_(torch.from_numpy(rng.uniform(-bound, bound, m.bias.shape).astype(np.float32)))
            elif isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(torch.from_numpy((1 + 0.2 * rng.standard_normal(m.weight.shape)).astype(np.float32)))
                m.bias.copy_(torch.from_numpy((0.2 * rng.standard_normal(m.bias.shape)).astype(np.float32)))
    return pol, head


def options_of(t):
    return dict(temperature=t.temperature, mask_entropy=t.mask_entropy, use_kl=t.use_kl, loss_scale=t.loss_scale,
                exponent=t.exponent)


def ref_inputs(b, dt):
    """transfer_ref's tensor arguments after the modules, in dtype dt."""
    import torch
    T = torch.from_numpy
    amap = T(b["map"]).long() if b["map"] is not None else None
    return (T(b["obs"]).to(dt), T(b["masks"]), T(b["old_logits"]).to(dt), T(b["old_masks"]), amap)


@functools.lru_cache(maxsize=None)
def build_transfer_case(name):
    """Case `name`: its modules, batch, float64 reference (r64) and torch fp32 yardstick (r32), computed once and shared:
    treat the result as read-only.  mods: [policy, critic] as ppo_reference's engine helpers take them (the critic is
    there to be left alone), shared: the head or None."""
    import torch
    t = CASES[name]
    pol, shared = build_student(t)
    crit = build_modules(t.case._replace(obs=t.shared[-1] if t.shared else t.case.obs))[1]
    b = build_transfer_batch(t)
    out = []
    for dt in (torch.float64, torch.float32):
        p = copy.deepcopy(pol).to(dt)
        s = copy.deepcopy(shared).to(dt) if shared is not None else None
        out.append(transfer_ref(p, s, *ref_inputs(b, dt), **options_of(t)))
    return {"name": name, "t": t, "case": t.case, "mods": [pol, crit], "shared": shared, "batch": b, "r64": out[0],
            "r32": out[1]}


def student_tensors(d):
    """(label, offset, numel) of the reference's flat gradient: the policy's tensors, then the shared head's."""
    o, out = 0, []
    for tag, m in (("policy", d["mods"][0]), ("shared_head", d["shared"])):
        if m is None:
            continue
        for pname, prm in m.named_parameters():
            out.append((f"{tag}.{pname}", o, prm.numel()))
            o += prm.numel()
    return out


# ------------------------------------------------------------------ side conditions
def gap_margin(d):
    """Over the legal (row, action) pairs of case data d, without those where o = c exactly in any precision (rows with
    one legal action on an unmapped case: 1 = 1; both raw probabilities under the clamp: 1e-11 = 1e-11): the smallest
    |o - c| / max(o, c) by float64, and the fp32 yardstick's largest |(o32 - c32) - (o64 - c64)| / max(o64, c64)."""
    b, r64, r32 = d["batch"], d["r64"], d["r32"]
    legal = b["masks"].astype(bool)
    o, c = r64["oprobs"].numpy(), r64["probs"].numpy()
    both = (r64["raw_probs"].numpy() < CLAMP * (1 - CLAMP_MARGIN)) & (r64["oraw"].numpy() < CLAMP * (1 - CLAMP_MARGIN))
    assert (o[legal & both] == c[legal & both]).all(), f"{d['name']}: elements under the clamp on both sides differ"
    single = (legal.sum(1, keepdims=True) == 1) & (b["map"] is None)
    if b["map"] is None:
        assert (o[legal & single] == c[legal & single]).all(), f"{d['name']}: a single-legal row differs"
    sel = legal & ~single & ~both
    err = np.abs((r32["oprobs"].double().numpy() - r32["probs"].double().numpy()) - (o - c)) / np.maximum(o, c)
    gap = (np.abs(o - c) / np.maximum(o, c))[sel]
    return (float(gap.min()) if gap.size else float("inf")), float(err.max()), int(sel.sum())


def top_two_margin(d):
    """The smallest relative separation (top1 - top2) / top1 of the two largest entries of every row of o and of c by
    float64, not counting a runner-up of o gathered from the same source as the top (an exact tie in any precision,
    decided by the first index)."""
    b, r64 = d["batch"], d["r64"]
    out = float("inf")
    for key, mapped in (("oprobs", True), ("probs", False)):
        p = r64[key].numpy()
        for i in range(p.shape[0]):
            order = np.argsort(-p[i], kind="stable")
            top = order[0]
            for k in order[1:]:
                if mapped and b["map"] is not None and b["map"][i, k] == b["map"][i, top]:
                    continue
                out = min(out, float((p[i, top] - p[i, k]) / p[i, top]))
                break
    return out


# ------------------------------------------------------------------ the golden pin of the reference
def golden_record(d):
    """What tests/golden/transfer_reference.npz keeps of a case's float64 reference: the metrics, their scales, and per
    parameter tensor ||g|| and g . u with u a unit vector from np.random.default_rng(31337 + tensor index)."""
    r64 = d["r64"]
    g = r64["grads"].numpy()
    assert g.dtype == np.float64, f"the golden record is of the float64 reference, not {g.dtype}"
    norms, projs = [], []
    for i, (_, o, k) in enumerate(student_tensors(d)):
        u = np.random.default_rng(31337 + i).standard_normal(k)
        norms.append(np.linalg.norm(g[o:o + k]))
        projs.append(g[o:o + k] @ (u / np.linalg.norm(u)))
    return {"metrics": r64["metrics"], "scales": r64["scales"], "grad_norm": np.array(norms), "grad_proj": np.array(projs)}


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def check_golden(d):
    """Case data d's float64 reference against its record: every metric and scale within GOLDEN_RTOL * max(|value|, its
    scale), the accuracy exactly, every tensor's norm and projection within GOLDEN_RTOL * ||g||."""
    key = d["name"]
    want = {k[len(key) + 1:]: v for k, v in _golden().items() if k.startswith(key + ":")}
    got = golden_record(d)
    assert want and set(got) == set(want), f"{key}: recorded {sorted(want)}, computed {sorted(got)}"
    bad = []
    for k, nm in enumerate(("loss", "accuracy", "entropy", "old_entropy")):
        for what in ("metrics", "scales"):
            a, w = got[what][k], want[what][k]
            tol = 0.0 if (nm == "accuracy") else GOLDEN_RTOL * max(abs(w), want["scales"][k])
            if not abs(a - w) <= tol:
                bad.append(f"{nm} {what}: {a!r} vs recorded {w!r}")
    assert len(want["grad_norm"]) == len(got["grad_norm"]), f"{key}: parameter tensor count"
    for i, (label, _, _) in enumerate(student_tensors(d)):
        for what in ("grad_norm", "grad_proj"):
            if not abs(got[what][i] - want[what][i]) <= GOLDEN_RTOL * want["grad_norm"][i]:
                bad.append(f"{label} {what}: {got[what][i]!r} vs recorded {want[what][i]!r}")
    assert not bad, f"{key}: " + "; ".join(bad)


# ------------------------------------------------------------------ the engine side
def make_student_engine(gpu, d, mode, max_rows=None):
    """A PPO holding case d's student (policy, critic and, if any, shared head), read back bit for bit."""
    import torch
    from rlgpu.ppo import PPO
    from ppo_reference import CLIP, ENT_SCALE
    t, c = d["t"], d["case"]
    p = PPO(obs_size=c.obs, num_actions=c.A, policy_layers=c.pol, critic_layers=c.crit, layer_norm=c.ln,
            leaky_slope=c.slope, clip_range=CLIP, entropy_scale=ENT_SCALE, max_rows=max_rows or t.max_rows or c.n, seed=1,
            init=False, train_gemm=mode, device=gpu, shared_layers=t.shared, policy_temperature=t.temperature,
            mask_entropy=t.mask_entropy, infer_fp16=t.fp16)
    mods = {0: d["mods"][0], 1: d["mods"][1]}
    if d["shared"] is not None:
        mods[2] = d["shared"]
    for m, seq in mods.items():
        p.load_torch_module(m, seq)
        for (name, a), b in zip(p.torch_module(m).named_parameters(), seq.parameters()):
            assert torch.equal(a, b), f"model {m}: {name} read back from the engine differs from what was loaded"
    return p


def engine_epoch0(gpu, p, d):
    """The teacher's probabilities from the case's logits (rlgpu_teacher_probs_from_logits) and every chunk of the batch
    on engine p, from zeroed gradients and metrics.  Returns (target probs, target argmax) on the device."""
    import torch
    from rlgpu.ppo import teacher_probs_from_logits
    t, b = d["t"], d["batch"]
    D = {k: torch.from_numpy(b[k]).to(gpu) for k in ("obs", "masks", "old_logits", "old_masks")}
    amap = torch.from_numpy(b["map"]).to(gpu) if b["map"] is not None else None
    p.zero_grad()
    p.metrics.zero_()
    probs, arg = teacher_probs_from_logits(D["old_logits"], D["old_masks"], t.temperature, t.mask_entropy, amap, p.metrics)
    n = d["case"].n
    for s0 in range(0, n, p.max_rows):
        p.transfer_chunk(D["obs"], D["masks"], probs, arg, None, s0, min(p.max_rows, n - s0), n, t.use_kl, t.loss_scale,
                         t.exponent)
    torch.cuda.synchronize()
    return probs, arg

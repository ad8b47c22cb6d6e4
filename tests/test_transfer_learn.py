"""Transfer learning at the kernel and C-ABI level (rlgpu_ppo_teacher_probs, rlgpu_teacher_probs_from_logits,
rlgpu_ppo_transfer_chunk, rlgpu_ppo_transfer_step, the per-model optimiser step count) against
transfer_reference.transfer_ref in float64, under ppo_reference's rules unchanged: check_grads on the policy's and the
shared head's gradients, one_element on the loss and the two entropies, the accuracy exactly (the number of matching
rows: the slot sums each chunk's count / n in fp32, so slot * n is the integer count to well within 1e-4), the critic's
gradients exactly zero.

Side conditions, decided by the float64 reference alone and asserted on the CPU for every case
(test_transfer_side_conditions_hold), again before each GPU case:
  * ppo_reference.side_conditions (kink margin, legal probabilities away from the clamp);
  * the sign margin: d |o - c| / d c = sign(c - o) (and the KL form's sign(log(o / c))) is decided by float64 only where
    the gap is well above fp32's error, so every legal element has |o - c| >= TL_DELTA * max(o, c).  Exempt are only
    elements equal in any precision: masked columns (1e-11 on both sides; with an action map the student's masks are
    the gathered teacher's), rows with a single legal action (1 = 1; unmapped cases only -- the mapped case has two
    legal actions in every row) and elements whose raw probabilities are both under the clamp;
  * the argmax margin: the top two of o and of c in every row are separated by TL_DELTA relative to the top, unless the
    two are gathered from the same source (an exact tie, the first index on both sides).
TL_DELTA is 10 x the fp32 yardstick's largest |(o32 - c32) - (o64 - c64)| / max(o64, c64) over the case table
(test_delta_covers_fp32 recomputes it).  Measured on the CPU over CASES: largest fp32 error 9.0e-7 (rows37_f16),
10 x that rounded up is TL_DELTA = 1e-5; smallest gap 7.5e-5 (rows37), smallest top-two separation 2.9e-4 (chunked).
The seeds in transfer_reference.CASES were searched on the CPU until the table passes.

The teacher's 16-bit forward is not the reference's business (transfer_reference's docstring): it is pinned by
test_teacher_handle, where rlgpu_ppo_teacher_probs on a teacher handle of other widths equals, bit for bit,
rlgpu_teacher_probs_from_logits on that handle's own inference forward, chunk edges included, and by the elementwise
bound that test_transfer_chunk puts on the kernel's probabilities (check_teacher_outputs): with u = 2^-24 and z the
tempered masked logits, a probability e^(z - zmax) / sum
carries one rounding of z = logit / T (relative u, moving the exponent by |z| u), one of the subtraction
(|z - zmax| u <= (|z| + zmax) u), expf's own error (2 ulp), the sum's (A terms of one sign, pairwise: log2(A) + 1
roundings <= 8 u) and the division's (u): |o - o64| <= (2 |z| + zmax + 12) u o64, asserted with a factor 2 on top.

The optimiser (test_transfer_step_three_epochs): three epochs on the fixed batch of case "shared" at lr = 3e-4, AdamW
without clipping on the policy and the shared head, every model's step count starting at 2 (so "not advanced" and
"reset" differ for the critic); per parameter tensor the change of the three steps against float64
AdamW, ||d - d64|| <= OPT_F * ||d32 - d64|| + 1e-7 * ||d64|| with d32 torch's own fp32 run of the same three steps and
OPT_F = 4 (check_grads' factor).  Measured on the CPU: the yardstick's error ||d32 - d64|| / ||d64|| over the tensors
is 6.7e-6 .. 1.8e-4 (test_optimiser_yardstick_on_cpu prints it).  Measured on an MI355X (h3 mode): the engine's error is
6.8e-6 .. 1.8e-4, per tensor 0.98 .. 1.07 of the yardstick's.  Over test_transfer_chunk's 33 cases the largest
(err - floor) / yardstick of a metric was 1.01 and the teacher probabilities' largest error was 0.48 of their bound.
"""
import copy
import ctypes

import numpy as np
import pytest

import transfer_reference as tr
from ppo_reference import MODE_IDS, MODES, check_grads, one_element, side_conditions

TL_DELTA = 1e-5  # sign / argmax margin, see the module docstring
OPT_F = 4.0      # the optimiser test's yardstick factor
M_ENTROPY, M_TL_LOSS, M_TL_ACCURACY, M_TL_OLD_ENTROPY = 0, 11, 12, 13
NAMES = list(tr.CASES)


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", NAMES)
def test_reference_matches_golden(name):
    """The float64 reference of every case against tests/golden/transfer_reference.npz."""
    tr.check_golden(tr.build_transfer_case(name))


@pytest.mark.parametrize("name", ["a2", "b17", "rows33", "rows37", "shared", "map23"])
def test_reference_against_autograd_of_the_written_gradient(name):
    """transfer_ref's gradient is torch autograd's of the literal loss; here the logit gradient the issue writes down --
    g e t^(e-1) sign(c - o) [o / c], the clamp gate, the masked softmax's backward, 1 / T -- is evaluated by hand in
    float64 and pushed through the network with autograd from the logits on: the two flat gradients agree to 1e-12 of
    each tensor's norm, and the L1 / KL, exponent, temperature and map branches are the same function on both sides."""
    import torch
    d = tr.build_transfer_case(name)
    t, b = d["t"], d["batch"]
    pol = copy.deepcopy(d["mods"][0]).double()
    shared = copy.deepcopy(d["shared"]).double() if d["shared"] is not None else None
    obs, masks, old_logits, old_masks, amap = tr.ref_inputs(b, torch.float64)
    x = shared(obs) if shared is not None else obs
    logits = pol(x)
    r = d["r64"]
    o, c, p = r["oprobs"], r["probs"], r["raw_probs"]
    n, A = c.shape
    g = t.loss_scale / (n * A)
    sg = torch.sign(c - o)
    tt = (o * torch.log(o / c)).abs() if t.use_kl else (o - c).abs()
    dc = g * t.exponent * (tt.pow(t.exponent - 1) if t.exponent != 1 else 1.0) * sg * (o / c if t.use_kl else 1.0)
    dc = torch.where((p >= 1e-11) & (p <= 1.0), dc, torch.zeros_like(dc))
    dlogits = p * (dc - (dc * p).sum(-1, keepdim=True)) / t.temperature
    mods = [m for m in (pol, shared) if m is not None]
    for m in mods:
        m.zero_grad(set_to_none=True)
    logits.backward(dlogits)
    got = torch.cat([q.grad.reshape(-1) for m in mods for q in m.parameters()])
    for label, off, k in tr.student_tensors(d):
        a, w = got[off:off + k], r["grads"][off:off + k]
        assert float((a - w).norm()) <= 1e-12 * float(w.norm()), (name, label)
    assert float(r["grads"].abs().max()) > 0


def test_new_names_exist():
    """The C ABI's new symbols are declared in the header and bound in Python, the metric slots are the issue's, and
    the Python surface has its new names."""
    import os
    from rlgpu import ppo
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rlgpu_ppo.h")).read()
    for sym in ("rlgpu_ppo_teacher_probs", "rlgpu_teacher_probs_from_logits", "rlgpu_ppo_transfer_chunk",
                "rlgpu_ppo_transfer_step", "rlgpu_ppo_model_optimizer_step", "rlgpu_ppo_set_model_optimizer_step",
                "rlgpu_diff_norm", "RLGPU_M_TL_LOSS = 11", "RLGPU_M_TL_ACCURACY = 12", "RLGPU_M_TL_OLD_ENTROPY = 13",
                "RLGPU_NUM_METRICS = 16"):
        assert sym in header, sym
    assert (ppo.M_TL_LOSS, ppo.M_TL_ACCURACY, ppo.M_TL_OLD_ENTROPY, ppo.NUM_METRICS) == (11, 12, 13, 16)
    for attr in ("teacher_probs", "transfer_chunk", "transfer_step", "transfer_learn", "model_optimizer_step",
                 "set_model_optimizer_step"):
        assert callable(getattr(ppo.PPO, attr)), attr
    assert callable(ppo.teacher_probs_from_logits) and callable(ppo.diff_norm)
    kernels = open(os.path.join(root, "reinforcement-learning_amd", "csrc", "transfer_kernels.hpp")).read()
    for k in ("teacher_probs", "transfer_loss", "adam_models"):
        assert f" {k}(" in kernels, k


def assert_side_conditions(d):
    import torch
    why = side_conditions(d["case"], d["r64"], torch.from_numpy(d["batch"]["masks"]))
    assert why is None, f"{d['name']}: {why}"
    near = int(((np.abs(d["r64"]["oraw"].numpy() / tr.CLAMP - 1) < tr.CLAMP_MARGIN) & d["batch"]["masks"].astype(bool)).sum())
    assert near == 0, f"{d['name']}: {near} legal teacher probabilities within 0.1 % of the clamp"
    if d["t"].mask_entropy:
        assert d["batch"]["masks"].sum(1).min() >= 2 and d["batch"]["old_masks"].sum(1).min() >= 2
    gap, _, count = tr.gap_margin(d)
    assert gap >= TL_DELTA, f"{d['name']}: a legal element {gap:.2e} inside the sign margin"
    assert count > 0 or d["case"].A == 2
    top = tr.top_two_margin(d)
    assert top >= TL_DELTA, f"{d['name']}: the top two of a row are {top:.2e} apart"
    off = ~d["batch"]["masks"].astype(bool)
    assert (d["r64"]["oprobs"].numpy()[off] == d["r64"]["probs"].numpy()[off]).all(), "masked columns differ"
    assert np.isfinite(d["r64"]["metrics"]).all() and bool(d["r64"]["grads"].isfinite().all())
    assert d["r64"]["metrics"][0] > 0


@pytest.mark.parametrize("name", NAMES)
def test_transfer_side_conditions_hold(name):
    d = tr.build_transfer_case(name)
    assert_side_conditions(d)
    if name == "a2":  # its rows with a single legal action: c = o = 1 exactly
        assert (d["batch"]["masks"].sum(1) == 1).any()
    if name == "map23":  # permuted, with repeats, and masks that follow the map
        m = d["batch"]["map"]
        assert m.shape == (d["case"].n, 17) and m.max() < 23 and all(len(set(r)) < 17 for r in m.tolist())


def test_delta_covers_fp32():
    """TL_DELTA is at least 10 x the yardstick's largest relative error of o - c over the case table and at most the
    smallest gap and top-two separation; the yardstick has float64's signs and argmax everywhere."""
    worst, small, top = 0.0, float("inf"), float("inf")
    for name in NAMES:
        d = tr.build_transfer_case(name)
        gap, err, _ = tr.gap_margin(d)
        worst, small, top = max(worst, err), min(small, gap), min(top, tr.top_two_margin(d))
        o64, c64 = d["r64"]["oprobs"].numpy(), d["r64"]["probs"].numpy()
        o32, c32 = d["r32"]["oprobs"].double().numpy(), d["r32"]["probs"].double().numpy()
        assert (np.sign(c32 - o32) == np.sign(c64 - o64)).all(), name
        assert (o32.argmax(1) == o64.argmax(1)).all() and (c32.argmax(1) == c64.argmax(1)).all(), name
        assert np.float32(d["r32"]["metrics"][1]) == np.float32(d["r64"]["metrics"][1]), name
    print(f"largest fp32 error of o - c {worst:.2e}, smallest gap {small:.2e}, smallest top-two separation {top:.2e}")
    assert 10 * worst <= TL_DELTA <= min(small, top), (worst, small, top)


def test_optimiser_yardstick_on_cpu():
    """The fp32 yardstick of the optimiser test against float64 over its three steps, per tensor (the figures of the
    module docstring), and the loss falls over the epochs."""
    d = tr.build_transfer_case("shared")
    d64, d32, losses = _three_epochs_refs(d)
    rel = [float((a - w).norm() / w.norm()) for a, w in zip(d32, d64)]
    print("yardstick error per tensor:", " ".join(f"{x:.1e}" for x in rel))
    assert max(rel) < 1e-3 and min(float(w.norm()) for w in d64) > 0
    assert losses[-1] < losses[0]


START_STEP = 2  # the optimiser test's step count before the epochs, every model (zero moments)


def _three_epochs_refs(d, epochs=3, lr=3e-4):
    """Per parameter tensor (policy, then shared head) the change over the epochs in float64 and in torch fp32, the
    optimisers starting at step count START_STEP with zero moments."""
    import torch
    t, b = d["t"], d["batch"]
    out, losses = [], None
    for dt in (torch.float64, torch.float32):
        pol = copy.deepcopy(d["mods"][0]).to(dt)
        shared = copy.deepcopy(d["shared"]).to(dt) if d["shared"] is not None else None
        before = [q.detach().clone() for m in (pol, shared) if m is not None for q in m.parameters()]
        ls = tr.transfer_epochs_ref(pol, shared, *tr.ref_inputs(b, dt), epochs=epochs, lr=lr, start_step=START_STEP, **tr.options_of(t))
        after = [q.detach() for m in (pol, shared) if m is not None for q in m.parameters()]
        out.append([(a - w).double() for a, w in zip(after, before)])
        losses = losses or ls
    return out[0], out[1], losses


# ------------------------------------------------------------------ GPU
def check_transfer_metrics(p, d, mode, tag):
    got = p.metrics.cpu().double().numpy()
    r64, r32, n = d["r64"], d["r32"], d["case"].n
    bad = []
    for k, (nm, slot) in enumerate((("tl_loss", M_TL_LOSS), ("tl_accuracy", M_TL_ACCURACY), ("entropy", M_ENTROPY),
                                    ("old_entropy", M_TL_OLD_ENTROPY))):
        ok, figures = one_element(nm, got[slot], r64["metrics"][k], r32["metrics"][k], r64["scales"][k], mode, n)
        print(f"{tag}: {figures}")
        if nm == "tl_accuracy":  # exact: the number of matching rows (the slot holds the chunks' counts / n, summed)
            ok = abs(got[slot] * n - round(r64["metrics"][k] * n)) <= 1e-4
        if not ok:
            bad.append(figures)
    assert not bad, f"{tag}: " + "; ".join(bad)


def check_transfer_grads(p, d, mode, tag):
    import torch
    r64, r32, n = d["r64"], d["r32"], d["case"].n
    npol = sum(q.numel() for q in d["mods"][0].parameters())
    ncrit = sum(q.numel() for q in d["mods"][1].parameters())
    crit = p.model_slice(1, grads=True).cpu()
    assert crit.numel() == ncrit and not bool(crit.any()), f"{tag}: the critic's gradients are not exactly zero"
    z64, z32 = torch.zeros(ncrit, dtype=torch.float64), torch.zeros(ncrit)
    ext = lambda r, z: {"grads": torch.cat([r["grads"][:npol], z.to(r["grads"].dtype)]), "head_bias_scale": 0.0}  # noqa: E731
    got = torch.cat([p.model_slice(0, grads=True), p.model_slice(1, grads=True)]).cpu()
    check_grads(got, ext(r64, z64), ext(r32, z32), d["mods"], mode, tag, n)
    if d["shared"] is not None:
        part = lambda r: {"grads": r["grads"][npol:], "head_bias_scale": 0.0}  # noqa: E731
        check_grads(p.model_slice(2, grads=True).cpu(), part(r64), part(r32), [d["shared"]], mode, tag + "/shared-head", n)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_transfer_chunk(gpu, name, mode):
    """Epoch 0 of every case and GEMM mode from zeroed gradients: the teacher's probabilities from the case's logits,
    every chunk of the batch, then the gradients and the four metrics against the float64 reference."""
    d = tr.build_transfer_case(name)
    assert_side_conditions(d)
    tag = f"{name}/{MODE_IDS[mode]}"
    p = tr.make_student_engine(gpu, d, mode)
    probs, arg = tr.engine_epoch0(gpu, p, d)
    errs = []
    for fn in (lambda: check_transfer_grads(p, d, mode, tag), lambda: check_transfer_metrics(p, d, mode, tag),
               lambda: check_teacher_outputs(probs, arg, d, tag)):
        try:
            fn()
        except AssertionError as e:
            errs.append(str(e))
    p.close()
    assert not errs, "\n".join(errs)


def teacher_bound(d):
    """(o64, the elementwise bound 2 (2 |z| + zmax + 12) 2^-24 o64) of the gathered teacher probabilities (module
    docstring); clamped elements are exact."""
    import torch
    t, b = d["t"], d["batch"]
    z = torch.from_numpy(b["old_logits"]).double() / t.temperature
    legal = torch.from_numpy(b["old_masks"]).bool()
    zm = (z + -1e10 * legal.logical_not()).max(-1).values.abs().unsqueeze(-1)
    k = 2 * z.abs() * legal + zm + 12
    if b["map"] is not None:
        k = k.gather(1, torch.from_numpy(b["map"]).long())
    o64 = d["r64"]["oprobs"]
    return o64, 2 * k * 2.0 ** -24 * o64


def check_teacher_outputs(probs, arg, d, tag):
    import torch
    o64, bound = teacher_bound(d)
    got = probs.cpu().double()
    under = d["r64"]["oraw"] < tr.CLAMP
    assert bool((got[under] == np.float32(1e-11)).all()), f"{tag}: a clamped teacher probability is not 1e-11"
    err = (got - o64).abs()
    worst = float((err / bound)[~under].max()) if bool((~under).any()) else 0.0
    print(f"{tag}: teacher probabilities, largest error / bound {worst:.2f}")
    assert bool((err <= bound)[~under].all()), f"{tag}: teacher probabilities off by {worst:.2f} x the bound"
    assert torch.equal(arg.cpu().long(), o64.argmax(-1)), f"{tag}: teacher argmax"


@pytest.mark.gpu
@pytest.mark.parametrize("fp16,shared,fused", [(0, (), True), (1, (32,), True), (0, (), False), (2, (), True)],
                         ids=["bf16", "fp16-shared", "bf16-layer", "fp32"])
def test_teacher_handle(gpu, monkeypatch, fp16, shared, fused):
    """rlgpu_ppo_teacher_probs on a teacher handle of its own architecture ([48], 23 actions, obs 150; LayerNorm off on
    the fp32 handle) equals rlgpu_teacher_probs_from_logits on the handle's own inference forward, bit for bit, in
    probabilities, argmax and the entropy metric's value: n = 1, 37 and max_rows + 3 (the chunk edge) on max_rows =
    40, without a map and with one (23 -> 17)."""
    import torch
    from rlgpu.ppo import NUM_METRICS, PPO, teacher_probs_from_logits
    if not fused:
        monkeypatch.setenv("RLGPU_FUSED_INFER", "0")
    rng = np.random.default_rng(5)
    T = PPO(obs_size=150, num_actions=23, policy_layers=(48,), critic_layers=(8,), shared_layers=shared, max_rows=40, seed=9,
            infer_fp16=fp16, policy_temperature=0.7, mask_entropy=True, layer_norm=fp16 != 2)
    for n in (1, 37, 43):
        obs = torch.from_numpy(rng.standard_normal((n, 150)).astype(np.float32)).to(gpu)
        masks = (rng.random((n, 23)) < 0.6).astype(np.uint8)
        masks[:, :2] = 1
        masks = torch.from_numpy(masks).to(gpu)
        amap = torch.from_numpy(rng.integers(23, size=(n, 17)).astype(np.int32)).to(gpu)
        logits = torch.cat([T.forward(0, obs[i:i + 40], half=fp16 != 2) for i in range(0, n, 40)])
        for m in (None, amap):
            want_m = torch.zeros(NUM_METRICS, device=gpu)
            got_m = torch.zeros(NUM_METRICS, device=gpu)
            want = teacher_probs_from_logits(logits, masks, 0.7, True, m, want_m)
            got = T.teacher_probs(obs, masks, m, metrics=got_m)
            assert got[0].shape == (n, 23 if m is None else 17)
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (n, m is None)
            assert torch.equal(got[1], want[1]), (n, m is None)
            assert float(want_m[M_TL_OLD_ENTROPY]) > 0
            # the entropy sum's atomic order is free: equal to a few ulp
            assert abs(float(got_m[M_TL_OLD_ENTROPY]) - float(want_m[M_TL_OLD_ENTROPY])) <= 4e-7 * float(want_m[M_TL_OLD_ENTROPY])
            assert not bool(got_m[:M_TL_OLD_ENTROPY].any())
    T.close()


@pytest.mark.gpu
def test_transfer_step_three_epochs(gpu):
    """Three epochs on the fixed batch of case "shared" at lr = 3e-4: the change of every policy and shared-head tensor
    against float64 AdamW under the yardstick rule of the module docstring; the critic's parameters, moments and step
    count byte-identical before and after; the per-model step counts read back and set."""
    import torch
    from rlgpu.ppo import teacher_probs_from_logits
    d = tr.build_transfer_case("shared")
    t, b, n = d["t"], d["batch"], d["case"].n
    d64, d32, _ = _three_epochs_refs(d)
    p = tr.make_student_engine(gpu, d, 2)
    # a history: a step count of START_STEP on every model, and non-zero critic moments
    p.set_optimizer_step(START_STEP)
    step0, m, v = p.optimizer_state()
    o1, c1 = p.model_range(1)
    m[o1:o1 + c1].normal_()
    v[o1:o1 + c1].uniform_()
    crit_before = [x[o1:o1 + c1].clone() for x in (p.params, m, v)]
    before = [p.model_slice(mi).clone() for mi in (0, 2)]
    D = {k: torch.from_numpy(b[k]).to(gpu) for k in ("obs", "masks", "old_logits", "old_masks")}
    probs, arg = teacher_probs_from_logits(D["old_logits"], D["old_masks"], t.temperature, t.mask_entropy)
    p.zero_grad()
    for _ in range(3):
        p.transfer_chunk(D["obs"], D["masks"], probs, arg, None, 0, n, n, t.use_kl, t.loss_scale, t.exponent)
        p.transfer_step(3e-4)
    torch.cuda.synchronize()
    assert [p.model_optimizer_step(mi) for mi in (0, 1, 2)] == [5, 2, 5]  # the critic's: not advanced, not reset
    assert p.optimizer_state()[0] == 5
    for x, w in zip((p.params, m, v), crit_before):
        assert torch.equal(x[o1:o1 + c1].view(torch.int32), w.view(torch.int32)), "the critic moved"
    assert not bool(p.grads.any()), "transfer_step leaves gradients behind"
    got = torch.cat([(p.model_slice(mi) - w).cpu().double() for mi, w in zip((0, 2), before)])
    bad, o = [], 0
    for (label, _, k), w, y in zip(tr.student_tensors(d), d64, d32):
        g = got[o:o + k]
        o += k
        err, yard, wn = float((g - w.reshape(-1)).norm()), float((y - w).norm()), float(w.norm())
        print(f"{label}: rel {err / wn:.2e}, torch fp32 {yard / wn:.2e}, ratio {max(err - 1e-7 * wn, 0) / yard:.2f}")
        if not err <= OPT_F * yard + 1e-7 * wn:
            bad.append(label)
    assert not bad, bad
    # the 16-bit copy follows the step: the inference forward sees the new parameters
    q = tr.make_student_engine(gpu, d, 2)
    for mi in (0, 2):
        q.model_slice(mi).copy_(p.model_slice(mi))
    q.refresh_half()
    assert torch.equal(p.forward(0, D["obs"], half=True), q.forward(0, D["obs"], half=True))
    # set / get per model; set_optimizer_step sets all; an ordinary step advances all
    p.set_model_optimizer_step(1, 7)
    assert [p.model_optimizer_step(mi) for mi in (0, 1, 2)] == [5, 7, 5]
    p.optimizer_step()
    assert [p.model_optimizer_step(mi) for mi in (0, 1, 2)] == [6, 8, 6]
    p.set_optimizer_step(5)
    assert [p.model_optimizer_step(mi) for mi in (0, 1, 2)] == [5, 5, 5]
    p.close()
    q.close()


@pytest.mark.gpu
def test_transfer_chunk_rejects_bad_arguments(gpu):
    """loss_exponent 0.5 (and NaN) is RLGPU_ERR_INVALID_ARG with the reason; so are more rows than max_rows and a
    non-finite loss_scale; a teacher without a map needs equal action counts."""
    import torch
    from rlgpu import _lib
    from rlgpu.ppo import teacher_probs_from_logits
    d = tr.build_transfer_case("b17")
    t, b, n = d["t"], d["batch"], d["case"].n
    p = tr.make_student_engine(gpu, d, 2)
    D = {k: torch.from_numpy(b[k]).to(gpu) for k in ("obs", "masks", "old_logits", "old_masks")}
    probs, arg = teacher_probs_from_logits(D["old_logits"], D["old_masks"], t.temperature, t.mask_entropy)
    p.zero_grad()
    args = (D["obs"], D["masks"], probs, arg, None, 0)
    for e in (0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.RLGPUError, match=r"\(-1\).*loss_exponent.*NaN"):
            p.transfer_chunk(*args, n, n, False, 1.0, e)
    with pytest.raises(_lib.RLGPUError, match=r"\(-1\).*max_rows"):
        p.transfer_chunk(*args, n + 1, n + 1)
    with pytest.raises(_lib.RLGPUError, match=r"\(-1\).*loss_scale"):
        p.transfer_chunk(*args, n, n, False, float("inf"), 1.0)
    assert not bool(p.grads.any())
    L = _lib.lib()
    out, a = torch.empty((n, 16), device=gpu), torch.empty(n, dtype=torch.int32, device=gpu)
    st = L.rlgpu_teacher_probs_from_logits(_lib.ptr(D["old_logits"]), _lib.ptr(D["old_masks"]), n, 17, None, 16,
                                           ctypes.c_float(1.0), 0, _lib.ptr(out), _lib.ptr(a), None, _lib.stream_ptr())
    assert st == -1 and "action map" in _lib.last_error()
    p.close()


@pytest.mark.gpu
def test_transfer_learn_report(gpu):
    """PPO.transfer_learn with a teacher handle of other widths: the report has the reference's five entries, the loss
    of a second call is below the first's (the student moves toward the teacher), and "Policy Update Magnitude" is the
    norm of the policy model's change."""
    import torch
    from rlgpu.learner import TransferLearnConfig
    from rlgpu.ppo import PPO
    rng = np.random.default_rng(8)
    n = 70
    S = PPO(policy_layers=(32, 32), critic_layers=(8,), max_rows=32, seed=5)
    T = PPO(policy_layers=(48,), critic_layers=(8,), max_rows=64, seed=77)
    obs = torch.from_numpy(rng.standard_normal((n, 167)).astype(np.float32)).to(gpu)
    masks = (rng.random((n, 90)) < 0.6).astype(np.uint8)
    masks[:, 0] = 1
    masks = torch.from_numpy(masks).to(gpu)
    cfg = TransferLearnConfig(lr=1e-3, epochs=5)
    before = S.model_slice(0).clone()
    crit = S.model_slice(1).clone()
    r1 = S.transfer_learn(T, obs, masks, cfg)
    mag = float((S.model_slice(0) - before).double().norm())
    r2 = S.transfer_learn(T, obs, masks, cfg)
    print(r1, r2)
    assert set(r1) == {"Old Policy Entropy", "Transfer Learn Accuracy", "Transfer Learn Loss", "Policy Entropy",
                       "Policy Update Magnitude"}
    assert all(np.isfinite(list(r1.values()))) and 0 <= r1["Transfer Learn Accuracy"] <= 1
    assert r2["Transfer Learn Loss"] < r1["Transfer Learn Loss"]
    # the same teacher over the same rows; the entropy sum's atomic order is free: equal to a few ulp
    assert r1["Old Policy Entropy"] > 0 and abs(r1["Old Policy Entropy"] - r2["Old Policy Entropy"]) <= 4e-7 * r1["Old Policy Entropy"]
    assert abs(r1["Policy Update Magnitude"] - mag) <= 1e-5 * mag
    assert torch.equal(S.model_slice(1), crit)
    assert [S.model_optimizer_step(mi) for mi in (0, 1)] == [10, 0]
    S.close()
    T.close()

"""Adagrad, RMSprop and MagSGD (ModelConfig::optimType; rlgpu_ppo_set_optimizer) against float64.

The three steps as the engine states them (include/rlgpu_ppo.h), with gr = grad * clip coefficient:
    adagrad   sum += gr^2;                 p -= lr * gr / (sqrt(sum) + 1e-10)
    rmsprop   sq = 0.99 sq + 0.01 gr^2;    p -= lr * gr / (sqrt(sq) + 1e-8)
    magsgd    p -= lr * gr / ||gr||        (||gr|| over the model's own parameters: a step of length lr)
restated here in float64 (restated_step) and held to torch.optim.Adagrad / RMSprop / SGD on float64 tensors.

The fixture is test_ppo_variants' OPTIM case and its learning rates; the reference runs (optim_reference) are
optimizer_reference's loop with the optimizer swapped.  Two kinds of engine check:

  band cases (adagrad at both max_norm, rmsprop at max_norm 1e-3): test_optimizer_clip_and_adamw's rules -- the share of
  coordinates outside band() at most OPT_SHARE, four times what the CPU test grants torch fp32, and no coordinate
  further from float64 than 0.1 x the largest float64 move.

  update-error cases (rmsprop at max_norm 1e3, magsgd at both): per model ||D - D64|| / ||D64||, D = parameters after -
  before, at most UPDATE_F = 4 times the same quantity of torch fp32 (the factor the suite grants its fp32-class GEMM
  modes over torch fp32).  RMSprop with the clip idle is no band case: a coordinate whose gradient is near zero moves by
  10 lr sign(g) in its first step, and torch fp32 alone leaves the band on 7.1e-5 of the coordinates.  MagSGD's update
  error is the rounding of the parameters themselves (a step of length lr spread over the model's 30 000 / 20 000
  coordinates is a few ulp of a weight per coordinate).
"""
import copy
import functools

import numpy as np
import pytest

from ppo_reference import MODE_IDS, MODES, build_batch, build_modules, engine_minibatch, make_engine, minibatch_ref, side_conditions
from test_ppo_variants import OPT, OPT_SHARE, OPTIM, band

KINDS = ("adagrad", "rmsprop", "magsgd")
LRS = (OPT["policy_lr"], OPT["critic_lr"])
BAND_CASES = [("adagrad", 1e-3), ("adagrad", 1e3), ("rmsprop", 1e-3)]
UPDATE_CASES = [("rmsprop", 1e3), ("magsgd", 1e-3), ("magsgd", 1e3)]
UPDATE_F = 4.0


# ------------------------------------------------------------------ the float64 restatement
def clip_coef(grads, max_norm):
    """clip_grad_norm_'s coefficient of one model's gradients (a list of tensors): min(max_norm / (||g|| + 1e-6), 1)."""
    import torch
    norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
    return min(float(max_norm / (norm + 1e-6)), 1.0) if max_norm is not None else 1.0


def restated_step(kind, params, grads, state, lr, max_norm):
    """One step of optimizer `kind` on one model in float64: params / grads / state lists of tensors (state: adagrad's
    sum or rmsprop's square_avg per parameter, updated in place like params; untouched by magsgd).  max_norm None: no
    clip (the transfer step)."""
    import torch
    coef = clip_coef(grads, max_norm)
    gr = [g * coef for g in grads]
    mag = torch.sqrt(sum((g ** 2).sum() for g in gr))
    for p, g, v in zip(params, gr, state):
        if kind == "adagrad":
            v += g * g
            p += -lr * (g / (v.sqrt() + 1e-10))
        elif kind == "rmsprop":
            v.mul_(0.99).add_(0.01 * g * g)
            p += -lr * (g / (v.sqrt() + 1e-8))
        else:
            assert kind == "magsgd", kind
            p += -lr * (g / mag)


def magsgd_normalize(params):
    """MagSGD::step's own part (Util/MagSGD.h) on one model: a float accumulator over the parameters' sums of squares
    (float64 on float64 parameters: the reference arithmetic, exact to double), sqrtf, grad /= the magnitude."""
    import torch
    f32 = params[0].dtype == torch.float32
    mag = np.float32(0) if f32 else 0.0
    for p in params:
        s = p.grad.detach().square().sum().item()
        mag = np.float32(mag + np.float32(s)) if f32 else mag + s
    mag = float(np.sqrt(mag))
    for p in params:
        p.grad /= mag


def torch_optimizer(kind, params, lr):
    """MakeOptimizer(type, params, lr) (Util/Models.h): the class's defaults with nothing but lr set."""
    import torch
    cls = {"adagrad": torch.optim.Adagrad, "rmsprop": torch.optim.RMSprop, "magsgd": torch.optim.SGD}[kind]
    return cls(params, lr=lr)


def torch_step(kind, params, opt, max_norm):
    """clip_grad_norm_ (max_norm None: none), MagSGD's normalisation, the optimizer's step; the unclipped norm."""
    import torch
    norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm)) if max_norm is not None else None
    if kind == "magsgd":
        magsgd_normalize(params)
    opt.step()
    return norm


def flat_of(ms):
    import torch
    return torch.cat([q.detach().reshape(-1).double() for m in ms for q in m.parameters()])


@functools.lru_cache(maxsize=None)
def optim_reference(kind, max_norm, steps=2):
    """test_ppo_variants.optimizer_reference with optimizer `kind` in AdamW's place: `steps` steps after clip_grad_norm_
    in float64 and in torch fp32; per step the batches, the gradient norms (policy, critic), the gradients and the flat
    parameters after the step ("flats"), with "start" the parameters before the first.  Shared: read-only."""
    import torch
    c = OPTIM
    mods = build_modules(c)
    tr = {}
    for dt in (torch.float64, torch.float32):
        ms = [copy.deepcopy(m).to(dt) for m in mods]
        ps = [list(m.parameters()) for m in ms]
        opts = [torch_optimizer(kind, ps[k], LRS[k]) for k in (0, 1)]
        norms, grads, batches, flats = [], [], [], []
        for it in range(steps):
            b = build_batch(c, copy.deepcopy(mods[0]).double(), seed=100 + it)
            rows = b["index"][b["start"]:b["start"] + c.n].astype(np.int64)
            adv = b["adv"].astype(np.float64)
            advn = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
            T = torch.from_numpy
            r = minibatch_ref(ms[0], ms[1], T(b["obs"][rows]).to(dt), T(b["masks"][rows]), T(b["acts"][rows]),
                              T(b["old"][rows]).to(dt), T(advn[rows]).to(dt), T(b["tgt"][rows]).to(dt), b["batch_size"])
            if dt == torch.float64:
                why = side_conditions(c, r, T(b["masks"][rows]))
                assert why is None, f"optimizer step {it}: {why}"
            grads.append(r["grads"].double())
            norms.append([torch_step(kind, ps[k], opts[k], max_norm) for k in (0, 1)])
            batches.append(b)
            flats.append(flat_of(ms))
        tr[dt] = {"norms": norms, "grads": grads, "flat": flats[-1], "flats": flats, "batches": batches,
                  "start": flat_of(mods)}
    return mods, tr[torch.float64], tr[torch.float32]


def model_slices(mods):
    sizes = [sum(q.numel() for q in m.parameters()) for m in mods]
    return [slice(0, sizes[0]), slice(sizes[0], sizes[0] + sizes[1])]


def update_error(flat, r64, sl, step=-1):
    """||D - D64|| / ||D64|| of one model, D = parameters after `step` - before the first."""
    d64 = r64["flats"][step][sl] - r64["start"][sl]
    return float(((flat[sl] - r64["start"][sl]) - d64).norm() / d64.norm())


def assert_clip_side(r64, max_norm):
    for pair in r64["norms"]:
        for nrm in pair:
            assert (nrm > 10 * max_norm) if max_norm < 1 else (nrm < 0.1 * max_norm), (nrm, max_norm)


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("max_norm", [1e-3, 1e3, None])
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_torch_float64(kind, max_norm):
    """restated_step against torch.optim.Adagrad / RMSprop / SGD (MagSGD: SGD on gradients divided by their norm) on
    float64 tensors over three steps, with the clip engaged, idle and absent: 1e-12 relative."""
    import torch
    g = torch.Generator().manual_seed(5)
    shapes = [(7, 5), (7,), (3, 7), (3,)]
    mine = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    theirs = [p.clone().requires_grad_() for p in mine]
    state = [torch.zeros_like(p) for p in mine]
    opt = torch_optimizer(kind, theirs, 3e-3)
    for _ in range(3):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) * 0.3 for s in shapes]
        for p, gr in zip(theirs, grads):
            p.grad = gr.clone()
        torch_step(kind, theirs, opt, max_norm)
        restated_step(kind, mine, grads, state, 3e-3, max_norm)
        for a, b in zip(mine, theirs):
            assert float((a - b.detach()).abs().max()) <= 1e-12 * float(b.detach().abs().max())
    for v, p in zip(state, theirs):
        if kind == "adagrad":
            assert float((v - opt.state[p]["sum"]).abs().max()) <= 1e-12 * float(v.abs().max())
        elif kind == "rmsprop":
            assert float((v - opt.state[p]["square_avg"]).abs().max()) <= 1e-12 * float(v.abs().max())
        else:
            assert not bool(v.any())


@pytest.mark.parametrize("max_norm", [1e-3, 1e3])
@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_share_on_cpu(kind, max_norm):
    """The reference's own share: two steps of torch fp32 against float64 on the OPTIM fixture.  Measured here:
        adagrad 1e-3: share outside band 0, worst 2.7e-6, largest move 2.0e-3, update error <= 6.6e-5
        adagrad 1e3:  0, 1.1e-7, 2.0e-3, <= 1.4e-5
        rmsprop 1e-3: 0, 4.4e-7, 2.0e-2, <= 1.5e-6
        rmsprop 1e3:  7.1e-5 (above OPT_SHARE / 4: not a band case), 5.1e-5, 2.0e-2, 1.2e-4 (critic)
        magsgd both:  0, 1.2e-7, ||D64|| = lr after step 1, 4.6e-4 (policy) / 1.5e-3 (critic).
    The band cases hold torch fp32 to OPT_SHARE / 4, as test_ppo_variants.test_optimizer_share_on_cpu does for AdamW;
    every case has a torch fp32 update error above zero (the engine tests' yardstick) and the clip on the side it is
    meant to be; MagSGD's first float64 update has length lr."""
    mods, r64, r32 = optim_reference(kind, max_norm)
    assert_clip_side(r64, max_norm)
    tight, worst = band(r32["flat"], r64["flat"])
    moved = float((r64["flat"] - r64["start"]).abs().max())
    errs = [update_error(r32["flat"], r64, sl) for sl in model_slices(mods)]
    print(f"{kind} {max_norm:g}: share {1 - tight:.2e}, worst {worst:.2e}, largest move {moved:.2e}, update error "
          f"{errs[0]:.2e} / {errs[1]:.2e}")
    if (kind, max_norm) in BAND_CASES:
        assert 1 - tight <= OPT_SHARE / 4 and worst < 0.1 * moved
        assert moved > 1e-4
    assert all(0 < e < 1e-2 for e in errs), errs
    if kind == "magsgd":
        for sl, lr in zip(model_slices(mods), LRS):
            assert abs(float((r64["flats"][0][sl] - r64["start"][sl]).norm()) / lr - 1) <= 1e-12


def test_unknown_optimizer_is_refused():
    """An unknown name is refused by PPO(optimizer=...) and by LearnerConfig before anything is built (no GPU needed)."""
    from rlgpu.learner import LearnerConfig
    from rlgpu.ppo import OPTIMIZERS, PPO
    assert OPTIMIZERS == {"adamw": 0, "adam": 1, "adagrad": 2, "rmsprop": 3, "magsgd": 4}
    with pytest.raises(ValueError, match="optimizer must be one of.*'sgd'"):
        PPO(optimizer="sgd")
    with pytest.raises(ValueError, match="optimizer must be one of.*'lion'"):
        LearnerConfig(optimizer="lion")
    for name in OPTIMIZERS:
        assert LearnerConfig(optimizer=name).optimizer == name


# ------------------------------------------------------------------ GPU
def run_engine(gpu, kind, max_norm, mode, r64, mods, check_norms=None):
    """`len(r64["batches"])` rounds of engine_minibatch + optimizer_step on a fresh engine; (engine, flat parameters)."""
    p = make_engine(gpu, OPTIM, mods, mode, max_grad_norm=max_norm, optimizer=kind, **OPT)
    for it, b in enumerate(r64["batches"]):
        engine_minibatch(gpu, p, OPTIM, b)
        p.optimizer_step()
        if check_norms is not None:
            check_norms(it, p.metrics.cpu().double().numpy()[7:9])
    assert float(p.grads.abs().max()) == 0.0  # the step zeroes the gradients
    return p, p.flat().cpu().double()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind,max_norm", BAND_CASES)
def test_optimizer_band(gpu, kind, max_norm, mode):
    """Two minibatch + optimizer_step rounds against float64 torch under test_optimizer_clip_and_adamw's rules: the
    share outside band at most OPT_SHARE, no coordinate further from float64 than 0.1 x the largest float64 move (which
    is above 1e-4), gradients zero afterwards, the grad-norm metrics within that test's bound of the float64 norms.
    Measured on an MI355X: share 0 in every case and mode; worst coordinate 1.0e-6 .. 2.1e-6 (adagrad 1e-3), 1.1e-7
    (adagrad 1e3), 4.6e-7 .. 7.3e-7 (rmsprop 1e-3) against largest moves of 2.0e-3, 2.0e-3 and 2.0e-2."""
    mods, r64, r32 = optim_reference(kind, max_norm)
    assert_clip_side(r64, max_norm)
    sls = model_slices(mods)

    def check_norms(it, got):
        g64, g32 = r64["grads"][it], r32["grads"][it]
        for m in (0, 1):
            want = r64["norms"][it][m]
            assert abs(float(g64[sls[m]].norm()) - want) <= 1e-12 * want
            tol = 4.0 * float((g32[sls[m]] - g64[sls[m]]).norm()) + (1e-7 + 7e-7) * want
            assert abs(got[m] - want) <= tol, (it, m, got[m], want, tol)

    p, flat = run_engine(gpu, kind, max_norm, mode, r64, mods, check_norms)
    tight, worst = band(flat, r64["flat"])
    moved = float((r64["flat"] - r64["start"]).abs().max())
    print(f"{kind} {max_norm:g} mode {mode}: share {1 - tight:.2e}, worst {worst:.2e}, largest move {moved:.2e}")
    assert 1 - tight <= OPT_SHARE, tight
    assert worst < 0.1 * moved, (worst, moved)
    assert moved > 1e-4
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind,max_norm", UPDATE_CASES)
def test_optimizer_update_error(gpu, kind, max_norm, mode):
    """Two rounds; per model the engine's ||D - D64|| / ||D64|| against UPDATE_F = 4 times torch fp32's, which is
    computed here from the reference runs alone.  Measured on an MI355X, engine in the modes x6 / f32 / H3 against torch
    fp32 on that host (no mode needs more than 1.0 x torch fp32's error, against the 4 x allowed):
        rmsprop 1e3   policy 5.7e-6 / 1.2e-5 / 8.1e-6 against 2.1e-5    critic 3.5e-5 / 3.9e-5 / 4.4e-5 against 1.1e-4
        magsgd, both  policy 4.51e-4 in every mode against 4.51e-4      critic 1.35e-3 in every mode against 1.35e-3
    (MagSGD's error is the parameters' own rounding, the same for the engine and torch: ratio 1.00.)"""
    mods, r64, r32 = optim_reference(kind, max_norm)
    assert_clip_side(r64, max_norm)
    p, flat = run_engine(gpu, kind, max_norm, mode, r64, mods)
    bad = []
    for name, sl in zip(("policy", "critic"), model_slices(mods)):
        err, yard = update_error(flat, r64, sl), update_error(r32["flat"], r64, sl)
        print(f"{kind} {max_norm:g} mode {mode} {name}: engine {err:.3e}, torch fp32 {yard:.3e}, ratio {err / yard:.2f}")
        if not err <= UPDATE_F * yard:
            bad.append((name, err, yard))
    assert not bad, bad
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("max_norm", [1e-3, 1e3])
def test_magsgd_update_has_length_lr(gpu, max_norm, mode):
    """After one MagSGD step each model's ||D|| is its lr, with the clip engaged and idle (the normalisation cancels the
    clip): | ||D|| / lr - 1 | at most four times torch fp32 MagSGD's on the CPU.  A kernel that forgot a division would
    give lr * coef * ||g|| (none at all), lr * ||g|| (by the coefficient alone) or lr * coef (by the unclipped norm):
    ||D|| / lr is further than the bound from each of them -- from coef only where the clip is engaged, since an idle
    clip's coefficient is 1 exactly and lr * coef is lr itself.  exp_avg and exp_avg_sq are not touched.  Measured on an
    MI355X: | ||D|| / lr - 1 | between 6.7e-7 and 1.4e-6 over the modes, models and both max_norm, torch fp32 0.99e-6 to
    1.07e-6 (so at most 1.4 x torch fp32's against the 4 x allowed); coef 4.5e-4 / 1.1e-4, ||g|| 2.2 / 9.2."""
    import torch
    mods, r64, r32 = optim_reference("magsgd", max_norm, 1)
    sls = model_slices(mods)
    p = make_engine(gpu, OPTIM, mods, mode, max_grad_norm=max_norm, optimizer="magsgd", **OPT)
    _, m, v = p.optimizer_state()
    m.normal_()
    v.uniform_()
    m0, v0 = m.clone(), v.clone()
    engine_minibatch(gpu, p, OPTIM, r64["batches"][0])
    p.optimizer_step()
    flat = p.flat().cpu().double()
    assert torch.equal(m.view(torch.int32), m0.view(torch.int32)) and torch.equal(v.view(torch.int32), v0.view(torch.int32))
    for k, (sl, lr) in enumerate(zip(sls, LRS)):
        yard = abs(float((r32["flat"][sl] - r32["start"][sl]).norm()) / lr - 1)
        bound = 4.0 * yard
        got = float((flat[sl] - r64["start"][sl]).norm()) / lr
        norm = r64["norms"][0][k]
        coef = min(max_norm / (norm + 1e-6), 1.0)
        print(f"magsgd {max_norm:g} mode {mode} model {k}: ||D|| / lr - 1 = {got - 1:.3e}, torch fp32 {yard:.3e}, "
              f"coef {coef:.3e}, ||g|| {norm:.3e}")
        assert 0 < yard < 1e-3, yard
        assert abs(got - 1) <= bound, (k, got, bound)
        wrong = [norm, coef * norm] + ([coef] if coef < 1.0 else [])
        for w in wrong:
            assert abs(got - w) > bound, (k, got, w, bound)
    p.close()


@pytest.mark.gpu
def test_adagrad_state_placement_and_late_setter(gpu):
    """Two Adagrad steps: exp_avg_sq holds the sum of gr^2 and exp_avg stays zero.  gr is formed from the engine's own
    gradient (read before each step) in float64; the tolerance per coordinate is 2e-6 of the sum: the fp32 clip
    coefficient is within 7e-7 + 3 x 2^-24 of the float64 one (the sum of squares' bound of
    test_optimizer_clip_and_adamw, a square root, a division, an add), gr one rounding more, its square twice that
    plus a rounding, the sum one more.  Then: the setter after a step is RLGPU_ERR_INVALID_ARG, by name."""
    import torch
    from rlgpu import _lib
    max_norm = 1e-3
    mods, r64, _ = optim_reference("adagrad", max_norm)
    p = make_engine(gpu, OPTIM, mods, 2, max_grad_norm=max_norm, optimizer="adagrad", **OPT)
    assert [p.get_optimizer(mi) for mi in (0, 1)] == ["adagrad", "adagrad"]
    _, m, v = p.optimizer_state()
    want = [torch.zeros(p.model_range(mi)[1], dtype=torch.float64) for mi in (0, 1)]
    for b in r64["batches"]:
        engine_minibatch(gpu, p, OPTIM, b)
        for mi in (0, 1):
            g = p.model_slice(mi, grads=True).cpu().double()
            want[mi] += (g * clip_coef([g], max_norm)) ** 2
        p.optimizer_step()
    torch.cuda.synchronize()
    for mi in (0, 1):
        o, c = p.model_range(mi)
        got = v[o:o + c].cpu().double()
        assert bool((want[mi] > 0).any())
        assert bool(((got - want[mi]).abs() <= 2e-6 * want[mi]).all()), float(((got - want[mi]).abs() / want[mi]).max())
        assert not bool(m[o:o + c].any()), "exp_avg is not Adagrad's"
    for model in (-1, 0, 1):
        with pytest.raises(_lib.RLGPUError, match=r"\(-1\).*already stepped"):
            p.set_optimizer(model, "rmsprop")
    assert p.get_optimizer(0) == "adagrad"
    p.close()


@pytest.mark.gpu
def test_per_model_setter_leaves_the_other_model(gpu):
    """set_optimizer(1, rmsprop): the policy's update is bit-identical to an all-AdamW handle's, the critic's is not;
    the types read back per model."""
    import torch
    mods, r64, _ = optim_reference("rmsprop", 1e-3)
    flats = []
    for mixed in (False, True):
        p = make_engine(gpu, OPTIM, mods, 2, max_grad_norm=1e-3, **OPT)
        if mixed:
            p.set_optimizer(1, "rmsprop")
        assert [p.get_optimizer(mi) for mi in (0, 1)] == ["adamw", "rmsprop" if mixed else "adamw"]
        for b in r64["batches"]:
            engine_minibatch(gpu, p, OPTIM, b)
            p.optimizer_step()
        flats.append([p.model_slice(mi).clone() for mi in (0, 1)])
        p.close()
    assert torch.equal(flats[0][0].view(torch.int32), flats[1][0].view(torch.int32))
    assert not torch.equal(flats[0][1], flats[1][1])


@pytest.mark.gpu
def test_default_is_adamw_byte_for_byte(gpu):
    """A handle that never calls the setter and one that calls set_optimizer(-1, adamw): after two steps the parameters
    and both moments are byte-identical."""
    import torch
    mods, r64, _ = optim_reference("adagrad", 1e3)  # the batches; the optimizer here is the handles' AdamW
    out = []
    for explicit in (False, True):
        p = make_engine(gpu, OPTIM, mods, 2, max_grad_norm=1e3, **OPT)
        if explicit:
            p.set_optimizer(-1, "adamw")
        for b in r64["batches"]:
            engine_minibatch(gpu, p, OPTIM, b)
            p.optimizer_step()
        step, m, v = p.optimizer_state()
        assert step == 2
        out.append([x.clone().view(torch.int32) for x in (p.params, m, v)])
        p.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert bool(out[0][1].any()) and bool(out[0][2].any())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_transfer_step_optimizers(gpu, kind):
    """One transfer_chunk + transfer_step(3e-4) of transfer_reference's case "shared" -- its smallest case that has both
    models the step touches, the policy and a shared head -- with each optimizer: per model the update error against the
    float64 step without a clip, at most UPDATE_F times torch fp32's (the float64 torch step is itself held to
    restated_step at 1e-12); the critic's parameters, moments and step count bit-unchanged.  Measured on an MI355X
    (policy, shared head), engine against torch fp32:
        adagrad  1.47e-5 against 1.46e-5, 1.10e-5 against 1.10e-5
        rmsprop  2.4e-6 against 3.3e-6,   2.2e-6 against 2.6e-6
        magsgd   1.32e-3 against 1.32e-3, 8.36e-4 against 8.36e-4"""
    import torch
    import transfer_reference as tr
    from rlgpu.ppo import teacher_probs_from_logits
    lr = 3e-4
    d = tr.build_transfer_case("shared")
    t, b, n = d["t"], d["batch"], d["case"].n
    deltas = {}
    for dt in (torch.float64, torch.float32):
        ms = [copy.deepcopy(x).to(dt) for x in (d["mods"][0], d["shared"])]
        tr.transfer_ref(ms[0], ms[1], *tr.ref_inputs(b, dt), **tr.options_of(t))
        before = [[q.detach().clone() for q in x.parameters()] for x in ms]
        grads = [[q.grad.detach().clone() for q in x.parameters()] for x in ms]
        for x in ms:
            ps = list(x.parameters())
            torch_step(kind, ps, torch_optimizer(kind, ps, lr), None)
        deltas[dt] = [torch.cat([(q.detach().double() - w.double()).reshape(-1) for q, w in zip(x.parameters(), ws)])
                      for x, ws in zip(ms, before)]
        if dt == torch.float64:  # the restatement, unclipped, says the same
            for x, ws, gs in zip(ms, before, grads):
                mine = [w.clone() for w in ws]
                restated_step(kind, mine, gs, [torch.zeros_like(w) for w in ws], lr, None)
                for a, q in zip(mine, x.parameters()):
                    assert float((a - q.detach()).abs().max()) <= 1e-12 * float(q.detach().abs().max())
    p = tr.make_student_engine(gpu, d, 2)
    p.set_optimizer(-1, kind)
    step0, m, v = p.optimizer_state()
    o1, c1 = p.model_range(1)
    m[o1:o1 + c1].normal_()
    v[o1:o1 + c1].uniform_()
    crit_before = [x[o1:o1 + c1].clone() for x in (p.params, m, v)]
    before = [p.model_slice(mi).clone() for mi in (0, 2)]
    D = {k: torch.from_numpy(b[k]).to(gpu) for k in ("obs", "masks", "old_logits", "old_masks")}
    probs, arg = teacher_probs_from_logits(D["old_logits"], D["old_masks"], t.temperature, t.mask_entropy)
    p.zero_grad()
    p.transfer_chunk(D["obs"], D["masks"], probs, arg, None, 0, n, n, t.use_kl, t.loss_scale, t.exponent)
    p.transfer_step(lr)
    torch.cuda.synchronize()
    assert [p.model_optimizer_step(mi) for mi in (0, 1, 2)] == [1, 0, 1]
    for x, w in zip((p.params, m, v), crit_before):
        assert torch.equal(x[o1:o1 + c1].view(torch.int32), w.view(torch.int32)), "the critic moved"
    assert not bool(p.grads.any()), "transfer_step leaves gradients behind"
    bad = []
    for name, mi, w, d64, d32 in zip(("policy", "shared_head"), (0, 2), before, deltas[torch.float64], deltas[torch.float32]):
        got = p.model_slice(mi).cpu().double() - w.cpu().double()
        err, yard = float((got - d64).norm() / d64.norm()), float((d32 - d64).norm() / d64.norm())
        print(f"transfer {kind} {name}: engine {err:.3e}, torch fp32 {yard:.3e}, ratio {err / yard:.2f}")
        if not err <= UPDATE_F * yard:
            bad.append((name, err, yard))
        if kind == "magsgd":
            assert abs(float(got.norm()) / lr - 1) < 1e-3, (name, float(got.norm()))
    assert not bad, bad
    p.close()

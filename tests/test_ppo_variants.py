"""Every leaf of the dispatch tree behind rlgpu_ppo_minibatch against a float64 reference.

The reference (minibatch_ref), the rules an engine result is held to (F = 4, the 1e-7 floor, K(n), S per metric),
the side conditions and the numbers measured on an MI355X are stated in tests/ppo_reference.py; this file owns the
case table, whose comments name the kernel each case reaches.

The optimizer test's share of coordinates outside the tight band is written at OPT_SHARE: 0 between torch fp32 and
float64 on the CPU, 1e-4 allowed (the engine measured 0 in every mode, largest parameter difference 1.0e-6; its
grad-norm metrics were within 2.4e-7 relative of the float64 norms, against a bound of about 1e-6).
"""
import copy

import numpy as np
import pytest

from ppo_reference import (DELTA, MODE_IDS, MODES, Case, build_batch, build_case, build_modules, check_golden,
                           engine_minibatch, make_engine, minibatch_ref, run_engine_case, scalar_floor,
                           side_conditions)


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


def case_data(name, seed=None):
    return build_case(CASES[name], seed=seed)


def assert_side_conditions(d):
    import torch
    why = side_conditions(d["case"], d["r64"], torch.from_numpy(d["batch"]["masks"][d["rows"]]))
    assert why is None, f"case {d['case'].name}: {why}"


# ------------------------------------------------------------------ CPU self-tests
@pytest.mark.parametrize("name", list(CASES))
def test_reference_matches_golden(name):
    """The float64 reference of every plain case against tests/golden/ppo_reference.npz (ppo_reference.check_golden)."""
    check_golden(f"plain/{name}", case_data(name))


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
def run_case(gpu, name, mode):
    d = case_data(name)
    assert_side_conditions(d)
    run_engine_case(gpu, d, mode, f"{name}/{MODE_IDS[mode]}")


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


def adamw_optimizers(param_lists, lrs, weight_decay):
    """The AdamW statement of the optimizer tests (and of learn_reference.optimizer_step_ref): one torch.optim.AdamW
    per model with nothing but its lr and the weight decay set."""
    import torch
    return [torch.optim.AdamW(ps, lr=lr, weight_decay=weight_decay) for ps, lr in zip(param_lists, lrs)]


def optimizer_reference(max_norm, steps=2):
    """Two AdamW steps after clip_grad_norm_ in float64 and in torch fp32: per step the batches, the gradient norms
    (policy, critic) and the fp32 gradient error; the final flat parameters of both."""
    import torch
    c = OPTIM
    mods = build_modules(c)
    tr = {}
    for dt in (torch.float64, torch.float32):
        ms = [copy.deepcopy(m).to(dt) for m in mods]
        opts = adamw_optimizers([m.parameters() for m in ms], (OPT["policy_lr"], OPT["critic_lr"]), OPT["weight_decay"])
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

"""Learner::Learn (host/learner.cpp) held step by step to learn_reference's float64 restatement of PPOLearner::Learn.

Teacher-forced: a gradient hook (called after a batch's last minibatch, before clip and step, the stream synchronised)
records for every optimizer step k the parameters p_k the batch's gradient was taken at, the gradient g_k and the
optimizer state s_k; p_{k+1} is the next call's parameters or the final ones.  Every step is then judged on its own:

  schedule   the hook's (epoch, batch) sequence is learn_schedule's; the optimizer's step counter rises by one per call
  order      rlgpu.ppo.permutation(M, seed, iteration * epochs + epoch) is a permutation of range(M), differs between
             epochs and between iterations, and is the epoch's order (composed with the row map
             t * P + 2 * q + (1 - old_team), restated in numpy, while an old version holds a team): the reference
             gradient is taken over order[b0:b1], so another order, another batch or another minibatch walk fails
  gradient   g_k against batch_step at p_k on the rows snapshotted after consume(): ppo_reference.check_grads unchanged
             (per tensor F ||g32 - g64|| + 1e-7 ||g64||, the 1e-4 ||g64|| contract, the elementwise rule)
  update     p_{k+1} - p_k against optimizer_step_ref(p_k, g_k, s_k): per model ||D - D64|| / ||D64|| at most
             test_optimizers.UPDATE_F times torch fp32's own; the last step's "Policy / Critic Grad Norm" by
             test_optimizer_clip_and_adamw's rule, 4 ||g32 - g64|| + (1e-7 + 7e-7) ||g64||
  metrics    read_metrics() divides by the schedule's minibatch count; the six means against the reference's means over
             the same minibatches by ppo_reference.one_element, K(n) of the largest minibatch, S the mean of the scales
  side       every minibatch of every step: no legal probability near the 1e-11 clamp, no ratio within 1e-4 of 1 +- clip
             (asserted, nothing excluded: the share of rows or steps left out is 0).  tanh has no kink.

The float64 cases run activation="tanh".  default_kind (leaky_relu, the row-fused training path) has a kink at every
hidden unit on rows that a GPU rollout chose, so its yardstick is a twin PPO handle loaded with p_k and driven from
Python over the same schedule (adv_normalizer on the gathered batch advantages, zero_grad, minibatch per entry): 1e-5
normwise, the project's bound for that comparison in test_guiding_learner_gpu and test_dist_gpu.

max_grad_norm is the Learner's fixed 0.5 (PPOLearner.cpp:522-526).  On these cases it gives only one side: both models'
gradient norms are above 0.5 at every step of every case, so the clip is engaged throughout and never idle through
Learn (no case was bent to change that); optimizer_step_ref's idle side is exercised on the CPU
(test_optimizer_step_ref_continues_a_run), the engine's in test_ppo_variants and test_optimizers.

Out of scope here: several ranks (trajRanges and the all-reduced advantage moments need two processes:
test_dist_gpu.py); the guide (its first batch: test_guiding_learner_gpu.py); frame stacking and obs standardisation
(they change what rows Learn reads, not the loop).

Measured on an MI355X (one run; every case passed the side conditions with its first seed, so the seeds tried are the
seeds below and nothing else).  Per case: rows, optimizer steps checked, the largest gradient error over what
check_grads' normwise rules allow, the largest update error over UPDATE_F x torch fp32's, the clip:
    overbatch x6 / f32 / h3   M 240, 4 steps, gradient 0.41 / 0.41 / 0.48, update 0.24, clip engaged, seed 11
    dropped                   M 240, 4 steps, gradient 0.40, update 0.25, clip engaged, seed 11
    whole                     M 240, 2 steps, gradient 0.39, update 0.24, clip engaged, seed 11
    short                     M 240, 2 steps, gradient 0.47, update 0.24, clip engaged, seed 11
    old_team 1 / 0            M 120, 4 steps each, gradient 0.41 / 0.61, update 0.24 / 0.25, clip engaged, seed 11
    trajectory                M 1208, 4 steps, gradient 0.37, update 0.25, clip engaged, seed 5
    second_iteration          M 240, 4 + 4 steps, gradient 0.48 / 0.42, update 0.24 / 0.25, clip engaged, seed 11
    temperature               M 240, 4 steps, gradient 0.45, update 0.25, clip engaged, seed 11
    default_kind              M 240, 4 steps, largest ||g - twin|| / ||twin|| 0: bit-equal at every step; update 0.24,
                              clip engaged, seed 11
(An update ratio of 0.25 is an error equal to torch fp32's own: the move's error is the rounding of the fp32 parameters.)
Every existing bound transferred unchanged: none was re-measured or widened.
"""
import copy

import numpy as np
import pytest

import learn_reference as lr
import ppo_reference as pr
from test_optimizers import UPDATE_F

MAX_NORM = 0.5
WIDTHS = (64, 64)
BASE = dict(num_arenas=6, rollout_len=10, epochs=2, batch_size=100, mini_batch_size=50, policy_layers=WIDTHS,
            critic_layers=WIDTHS, train_against_old_versions=False, collect_groups=1, activation="tanh", layer_norm=True,
            train_gemm=2, seed=11)
TRAJECTORY = dict(BASE, num_arenas=16, rollout_len=8, experience_mode=1, ts_per_itr=1200, max_episode_duration=1.0,
                  batch_size=500, mini_batch_size=250, seed=5)
# every (M, batch_size) of the cases below (the trajectory mode's M is read at run time: a spread from 1200 on)
USED_RANGES = [(240, 100), (240, None), (240, 400), (120, 50)] + [(m, 500) for m in (1200, 1201, 1499, 1500, 1737, 2000)]


# ------------------------------------------------------------------ CPU: the restatement itself
def test_batch_ranges_equal_the_engine():
    """batch_ranges_ref, written from ExperienceBuffer.cpp on its own, against rlgpu_batch_ranges on
    test_dist.py::test_batch_ranges_match_experience_buffer's table and on every (M, batch_size) used here."""
    from rlgpu.learner import batch_ranges
    table = [(100_000, 100_000), (250, 100), (300, 100), (50, 100), (0, 100)] + USED_RANGES
    for M, b in table:
        for over in (True, False):
            assert lr.batch_ranges_ref(M, b, over) == batch_ranges(M, M if b is None else b, over), (M, b, over)
    assert lr.batch_ranges_ref(250, 100, True) == [(0, 100), (100, 250)]
    assert lr.batch_ranges_ref(250, 100, False) == [(0, 100), (100, 200)]
    assert lr.batch_ranges_ref(50, 100, True) == [(0, 50)] and lr.batch_ranges_ref(50, 100, False) == []


@pytest.mark.parametrize("M,batch", USED_RANGES + [(250, 100), (50, 100), (7, 3)])
@pytest.mark.parametrize("mini", [25, 50, 64, 250])
def test_schedule_visits_every_row_once(M, batch, mini):
    """With overbatching an epoch's minibatches tile [0, M) exactly once, in order; without it they tile
    [0, floor(M / batch) * batch) and nothing else; no minibatch is longer than mini_batch_size and only a batch's
    last one is shorter."""
    for over in (True, False):
        sched = lr.learn_schedule(M, batch, mini, over, 2)
        for epoch in (0, 1):
            entries = [e for e in sched if e[0] == epoch]
            assert [e[1] for e in entries] == list(range(len(entries)))
            seen = np.zeros(M, np.int64)
            pos = 0
            for _, _, mbs in entries:
                for s0, n in mbs:
                    assert s0 == pos and 0 < n <= mini, (s0, n, pos)
                    seen[s0:s0 + n] += 1
                    pos += n
                assert all(n == mini for _, n in mbs[:-1])
            end = M if (over or batch is None) else (M // batch) * batch
            assert (seen[:end] == 1).all() and (seen[end:] == 0).all(), (M, batch, mini, over)


@pytest.fixture(scope="module")
def synthetic():
    """240 synthetic rows on (32, 32) tanh models in float64, and the overbatched last batch (100, 240) of an order."""
    c = pr.Case("learn_cpu", 167, 90, (32, 32), (32, 32), seed=3, slope=1.0, n=140, extra=100)
    mods = [pr.swap_activation(m, "tanh") for m in pr.build_modules(c)]
    mods64 = [copy.deepcopy(m).double() for m in mods]
    b = pr.build_batch(c, mods64[0])
    data = {k: b[k] for k in ("obs", "masks", "acts", "old", "adv", "tgt")}
    order = b["index"].astype(np.int64)
    entry = lr.learn_schedule(240, 100, 50, True, 1)[1]
    assert entry == (0, 1, [(100, 50), (150, 50), (200, 40)])
    return mods64, data, order[100:240], entry


def rel(a, b):
    return float((a - b).norm() / b.norm())


def test_minibatch_walk_equals_one_call(synthetic):
    """The float64 gradient of a batch walked in minibatches 50, 50, 40 is the gradient of the same 140 rows in one
    call (every term is a sum over rows divided by the configured batch size), to float64 summation noise."""
    mods64, data, rows, entry = synthetic
    walked = lr.batch_step(mods64, data, rows, entry, 100)
    once = lr.batch_step(mods64, data, rows, (0, 1, [(100, 140)]), 100)
    assert walked["n"] == [50, 50, 40] and once["n"] == [140]
    assert rel(walked["grads"], once["grads"]) <= pr.GOLDEN_RTOL
    assert float(once["grads"].norm()) > 0


def test_reference_sees_the_loop_bugs(synthetic):
    """What the case table must be able to see, on the synthetic batch: the overbatched batch weighted by its own
    length (140) instead of the configured 100, and a dropped tail minibatch.  Each moves the float64 gradient by more
    than 1e-3 normwise (the engine's bound is 1e-4 at most)."""
    mods64, data, rows, entry = synthetic
    right = lr.batch_step(mods64, data, rows, entry, 100)["grads"]
    own_length = lr.batch_step(mods64, data, rows, entry, 140)["grads"]
    assert rel(own_length, right) > 1e-3
    no_tail = lr.batch_step(mods64, data, rows[:100], (0, 1, [(100, 50), (150, 50)]), 100)["grads"]
    assert rel(no_tail, right) > 1e-3


@pytest.mark.parametrize("kind", ["adamw", "adam", "adagrad", "rmsprop", "magsgd"])
def test_optimizer_step_ref_continues_a_run(kind):
    """optimizer_step_ref from the state a torch optimizer holds after two steps gives that optimizer's third step
    (float64, 1e-12 relative), with the clip engaged (policy, norm above 0.5) and idle (critic)."""
    import torch
    from test_optimizers import torch_optimizer, torch_step
    from test_ppo_variants import adamw_optimizers
    g = torch.Generator().manual_seed(9)
    sizes, lrs, scale = (301, 77), (2.5e-4, 1e-3), (1.0, 0.01)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g, dtype=torch.float64)) for n in sizes]
    if kind in ("adamw", "adam"):
        opts = adamw_optimizers([[p] for p in ps], lrs, 0.0 if kind == "adam" else 1e-2)
    else:
        opts = [torch_optimizer(kind, [p], lr) for p, lr in zip(ps, lrs)]
    key = {"adagrad": "sum", "rmsprop": "square_avg"}.get(kind, "exp_avg_sq")
    for step in range(3):
        grads = [torch.randn(n, generator=g, dtype=torch.float64) * s for n, s in zip(sizes, scale)]
        if step == 2:
            zero = [torch.zeros(n, dtype=torch.float64) for n in sizes]
            state = {"exp_avg": [o.state[p].get("exp_avg", z) for o, p, z in zip(opts, ps, zero)],
                     "exp_avg_sq": [o.state[p].get(key, z) for o, p, z in zip(opts, ps, zero)]}
            mine, norms, coefs = lr.optimizer_step_ref(kind, [p.detach() for p in ps], grads, state, step, lrs, MAX_NORM,
                                                       torch.float64)
            assert coefs[0] < 1.0 and coefs[1] == 1.0, coefs
        for p, gr, o in zip(ps, grads, opts):
            p.grad = gr.clone()
            torch_step(kind, [p], o, MAX_NORM)
    for a, p in zip(mine, ps):
        assert float((a - p.detach()).abs().max()) <= 1e-12 * float(p.detach().abs().max())


# ------------------------------------------------------------------ GPU: the harness
def flat_models(ppo, buf):
    """A num_params buffer (gradients, moments) without the alignment gaps between the models: PPO.flat()'s layout."""
    import torch
    return torch.cat([buf[o:o + c] for o, c in (ppo.model_range(m) for m in ppo.models)])


def snapshot(L):
    """The rows Learn trains on, cloned on the device: the rollout's [T * P] rows, or the trajectory mode's batch."""
    if L.cfg.experience_mode == 1:
        b = L.batch()
        d = {"obs": b["obs"], "masks": b["masks"], "acts": b["actions"], "old": b["logp"], "adv": b["adv"], "tgt": b["target"]}
    else:
        T, n = L.T, L.T * L.P
        d = {"obs": L.obs[:T].reshape(n, L.W), "masks": L.masks[:T].reshape(n, 90), "acts": L.actions.reshape(-1),
             "old": L.logp.reshape(-1), "adv": L.adv.reshape(-1), "tgt": L.target.reshape(-1)}
    return {k: v.clone().contiguous() for k, v in d.items()}


def run_learn(gpu, kw, iterations=1, old_team=None, prepare=None):
    """Build the Learner, then per iteration: collect, consume, snapshot, learn under the gradient hook.  Returns
    (the Learner, [per iteration: the hook's records, the snapshot, the iteration counter, the final parameters, the
    raw minibatch count and read_metrics()])."""
    import torch
    from rlgpu import _lib
    from rlgpu.learner import Learner, LearnerConfig
    L = Learner(LearnerConfig(**kw), device=gpu)
    if prepare:
        prepare(L)
    steps = []

    def hook(g, epoch, batch):
        torch.cuda.synchronize()
        step, m, v = L.ppo.optimizer_state()
        steps.append({"epoch": epoch, "batch": batch, "step": step, "params": L.ppo.flat().cpu(),
                      "grads": flat_models(L.ppo, g).cpu(), "exp_avg": flat_models(L.ppo, m).cpu(),
                      "exp_avg_sq": flat_models(L.ppo, v).cpu()})

    L.set_grad_hook(hook)
    out = []
    for it in range(iterations):
        L.collect()
        L.consume()
        torch.cuda.synchronize()
        if old_team is not None:
            _lib.check(_lib.lib().rlgpu_learner_set_old_team(L._h, old_team), "rlgpu_learner_set_old_team")
        dev = snapshot(L)
        iteration = L.iteration
        del steps[:]
        L.learn()
        torch.cuda.synchronize()
        _, count = L._metrics(False)
        out.append({"steps": list(steps), "dev": dev, "data": {k: v.cpu().numpy() for k, v in dev.items()},
                    "iteration": iteration, "final": L.ppo.flat().cpu(), "count": count, "metrics": L.ppo.read_metrics()})
        if it + 1 < iterations:
            L.finish_iteration()
    return L, out


def orders_of(gpu, L, rec, old_team):
    """The order of every epoch of one iteration (the Order checks), and its schedule."""
    from rlgpu.ppo import permutation
    cfg = L.cfg
    rows = None if old_team is None else lr.train_rows_ref(L.T, L.P, old_team)
    M = rec["data"]["adv"].size if rows is None else rows.size
    perms = {(i, e): permutation(M, cfg.seed, i * cfg.epochs + e, device=gpu).cpu().numpy().astype(np.int64)
             for i in (rec["iteration"], rec["iteration"] + 1) for e in range(cfg.epochs)}
    for key, p in perms.items():
        assert np.array_equal(np.sort(p), np.arange(M)), f"counter of {key}: not a permutation of range({M})"
    it = rec["iteration"]
    for e in range(cfg.epochs):
        assert not np.array_equal(perms[it, e], perms[it + 1, e]), f"epoch {e}: the same order in iterations {it}, {it + 1}"
        for f in range(e):
            assert not np.array_equal(perms[it, e], perms[it, f]), f"epochs {f} and {e} share an order"
    orders = [perms[it, e] if rows is None else rows[perms[it, e]] for e in range(cfg.epochs)]
    if rows is not None:
        assert all((o % 2 == 1 - old_team).all() and np.unique(o).size == M for o in orders), "the row map"
    return M, orders, lr.learn_schedule(M, cfg.batch_size, cfg.mini_batch_size, cfg.overbatching, cfg.epochs)


def check_schedule(rec, sched, first_step):
    steps = rec["steps"]
    assert [(s["epoch"], s["batch"]) for s in steps] == [(e, b) for e, b, _ in sched], \
        ([(s["epoch"], s["batch"]) for s in steps], [(e, b) for e, b, _ in sched])
    assert [s["step"] for s in steps] == list(range(first_step, first_step + len(sched))), [s["step"] for s in steps]
    want = sum(len(mbs) for _, _, mbs in sched)
    assert rec["count"] == want, f"read_metrics divides by {rec['count']}, the schedule has {want} minibatches"


def split(flat, sizes):
    return [flat[:sizes[0]], flat[sizes[0]:sizes[0] + sizes[1]]]


def check_updates(L, rec, tag):
    """Every step's move p_{k+1} - p_k against optimizer_step_ref(p_k, g_k, s_k) by test_optimizers' update-error rule.
    Returns (the largest err / (UPDATE_F x torch fp32's), whether the clip engaged in some step, and idled in some)."""
    import torch
    cfg, steps = L.cfg, rec["steps"]
    sizes = [L.ppo.model_range(m)[1] for m in (0, 1)]
    worst, engaged, idle, bad = 0.0, False, False, []
    for k, s in enumerate(steps):
        nxt = steps[k + 1]["params"] if k + 1 < len(steps) else rec["final"]
        state = {key: split(s[key], sizes) for key in ("exp_avg", "exp_avg_sq")}
        args = (cfg.optimizer, split(s["params"], sizes), split(s["grads"], sizes), state, s["step"],
                (cfg.policy_lr, cfg.critic_lr), MAX_NORM)
        new64, _, coefs = lr.optimizer_step_ref(*args, torch.float64)
        new32, _, _ = lr.optimizer_step_ref(*args, torch.float32)
        engaged |= any(c < 1.0 for c in coefs)
        idle |= any(c == 1.0 for c in coefs)
        for name, p0, p1, w64, w32 in zip(("policy", "critic"), split(s["params"], sizes), split(nxt, sizes), new64, new32):
            d64 = w64 - p0.double()
            err = float(((p1.double() - p0.double()) - d64).norm() / d64.norm())
            yard = float(((w32.double() - p0.double()) - d64).norm() / d64.norm())
            assert yard > 0, f"{tag} step {k} {name}: torch fp32's update is float64's"
            worst = max(worst, err / (UPDATE_F * yard))
            if not err <= UPDATE_F * yard:
                bad.append(f"step {k} {name}: update error {err:.3e}, torch fp32 {yard:.3e}")
    assert float((rec["final"] - steps[0]["params"]).abs().max()) > 0, f"{tag}: the parameters did not move"
    assert not bad, f"{tag}: " + "; ".join(bad)
    return worst, engaged, idle


def grad_ratio(got, r64, r32, mods, mode, n):
    """The largest err / allowed over the parameter tensors under check_grads' two normwise rules (for the record)."""
    worst = 0.0
    for label, o, k in pr.param_tensors(mods):
        g, w, t = got[o:o + k].double(), r64["grads"][o:o + k], r32["grads"][o:o + k].double()
        err, yard, wn = float((g - w).norm()), float((t - w).norm()), float(w.norm())
        floor = 1e-7 * wn + (pr.scalar_floor(n, r64["head_bias_scale"]) if k == 1 else 0.0)
        worst = max(worst, err / (pr.factor(mode, n) * yard + floor), err / (1e-4 * wn))
    return worst


def check_against_float64(L, rec, orders, sched, tag, **options):
    """Gradient, side conditions, metrics and the last step's grad-norm metrics against the float64 restatement."""
    import torch
    cfg, steps, data = L.cfg, rec["steps"], rec["data"]
    mode = cfg.train_gemm
    arch = (L.W, 90, cfg.policy_layers, cfg.critic_layers, cfg.layer_norm, cfg.activation)
    worst, errs, m64, m32, s64, ns = 0.0, [], [], [], [], []
    for k, (s, entry) in enumerate(zip(steps, sched)):
        b0, b1 = lr.entry_range(entry)
        rows = orders[entry[0]][b0:b1]
        mods32 = lr.modules_from_flat(s["params"], *arch, torch.float32)
        r64 = lr.batch_step(lr.modules_from_flat(s["params"], *arch, torch.float64), data, rows, entry, cfg.batch_size, **options)
        r32 = lr.batch_step(mods32, data, rows, entry, cfg.batch_size, **options)
        why = [f"minibatch {i}: {w}" for i, w in enumerate(r64["side"]) if w is not None]
        assert not why, f"{tag} step {k}: the float64 reference does not decide this step: " + "; ".join(why)
        n = max(r64["n"])
        worst = max(worst, grad_ratio(s["grads"], r64, r32, mods32, mode, n))
        try:
            pr.check_grads(s["grads"], r64, r32, mods32, mode, f"{tag} step {k} (epoch {entry[0]} batch {entry[1]})", n)
        except AssertionError as e:
            errs.append(str(e))
        m64.append(r64["metrics"])
        m32.append(r32["metrics"])
        s64.append(r64["scales"])
        ns += r64["n"]
    assert not errs, "\n".join(errs)
    # the last step's grad-norm metrics (test_optimizer_clip_and_adamw's rule)
    sizes = [L.ppo.model_range(m)[1] for m in (0, 1)]
    for name, g64, g32 in zip(("Policy", "Critic"), split(r64["grads"], sizes), split(r32["grads"].double(), sizes)):
        want, got = float(g64.norm()), rec["metrics"][f"{name} Grad Norm"]
        tol = 4.0 * float((g32 - g64).norm()) + (1e-7 + 7e-7) * want
        assert abs(got - want) <= tol, f"{tag}: {name} Grad Norm {got!r} vs {want!r}, allowed {tol:.2e}"
    # the six means over every minibatch of the schedule
    m64, m32, s64 = (np.concatenate(x).mean(0) for x in (m64, m32, s64))
    names = ("Policy Entropy", "Mean KL Divergence", "Policy Loss", "Critic Loss", "Ratio", "SB3 Clip Fraction")
    res = [pr.one_element(nm, rec["metrics"][nm], m64[i], m32[i], s64[i], mode, max(ns)) for i, nm in enumerate(names)]
    assert all(ok for ok, _ in res), f"{tag}: " + "; ".join(fig for ok, fig in res if not ok)
    return worst


def run_case(gpu, tag, kw, *, iterations=1, old_team=None, prepare=None, first_ranges=None, **options):
    L, recs = run_learn(gpu, kw, iterations, old_team, prepare)
    first_step = 0
    try:
        for rec in recs:
            M, orders, sched = orders_of(gpu, L, rec, old_team)
            if first_ranges is not None:
                assert [lr.entry_range(e) for e in sched if e[0] == 0] == first_ranges, sched
            check_schedule(rec, sched, first_step)
            g = check_against_float64(L, rec, orders, sched, f"{tag} it {rec['iteration']}", **options)
            u, engaged, idle = check_updates(L, rec, f"{tag} it {rec['iteration']}")
            print(f"learn loop {tag} it {rec['iteration']}: M {M}, steps {len(sched)}, gradient err / allowed {g:.3f}, "
                  f"update err / allowed {u:.3f}, clip engaged {engaged}, idle {idle}, seed {kw['seed']}")
            first_step += len(sched)
    finally:
        L.close()
    return recs


# ------------------------------------------------------------------ GPU: the cases
@pytest.mark.gpu
@pytest.mark.parametrize("mode", pr.MODES, ids=pr.MODE_IDS)
def test_overbatch(gpu, mode):
    """M = 240, batch 100, minibatch 50: ranges (0, 100), (100, 240); minibatches 50, 50 then 50, 50, 40 (the tail); the
    last batch weighted by 100, not 140; indexed advantage statistics.  In the three GEMM modes."""
    run_case(gpu, f"overbatch/{pr.MODE_IDS[mode]}", dict(BASE, train_gemm=mode), first_ranges=[(0, 100), (100, 240)])


@pytest.mark.gpu
def test_dropped(gpu):
    """overbatching off: ranges (0, 100), (100, 200); the rows order[200:240] are trained by nobody."""
    run_case(gpu, "dropped", dict(BASE, overbatching=False), first_ranges=[(0, 100), (100, 200)])


@pytest.mark.gpu
def test_whole(gpu):
    """batch_size None: one batch of 240, the un-gathered advantage-statistics shortcut; minibatches 64, 64, 64, 48."""
    recs = run_case(gpu, "whole", dict(BASE, batch_size=None, mini_batch_size=64), first_ranges=[(0, 240)])
    assert recs[0]["count"] == 8


@pytest.mark.gpu
def test_short(gpu):
    """M = 240 < batch_size = 400: one batch of 240 weighted by 400."""
    run_case(gpu, "short", dict(BASE, batch_size=400), first_ranges=[(0, 240)])


@pytest.mark.gpu
@pytest.mark.parametrize("old_team", [1, 0])
def test_old_team(gpu, old_team):
    """An old version holds one team (set after consume()): the M = 120 rows of the other team only, through
    k_train_rows and k_compose; ranges (0, 50), (50, 120)."""
    run_case(gpu, f"old_team{old_team}", dict(BASE, batch_size=50, mini_batch_size=25), old_team=old_team,
             first_ranges=[(0, 50), (50, 120)])


def desynchronise(L):
    """test_trajectories' way of spreading the arenas' episode counters, so that trajectories end on different steps."""
    from rlgpu.state import ARENA
    max_len = int(L.cfg.max_episode_duration * (120.0 / 8))
    st = np.frombuffer(L.env.get_arenas().tobytes(), ARENA).copy()
    st["env"]["episode_steps"] = np.random.default_rng(1).integers(0, max_len, L.cfg.num_arenas)
    L.env.set_arenas(np.frombuffer(st.tobytes(), np.uint8))


@pytest.mark.gpu
def test_trajectory(gpu):
    """experience_mode 1 (test_trajectories' config): Learn switches to the combined batch; M is what it holds (at
    least ts_per_itr = 1200), the ranges and tails follow from it."""
    recs = run_case(gpu, "trajectory", TRAJECTORY, prepare=desynchronise)
    assert recs[0]["data"]["adv"].size >= 1200


@pytest.mark.gpu
def test_second_iteration(gpu):
    """overbatch, finish_iteration(), and a second collect / consume / learn: the permutation counter
    iteration * epochs + epoch, and the Adam state carried across iterations (the first hook of iteration 1 sees step 4)."""
    recs = run_case(gpu, "second_iteration", BASE, iterations=2)
    assert [r["iteration"] for r in recs] == [0, 1] and recs[1]["steps"][0]["step"] == 4
    assert float(recs[1]["steps"][0]["exp_avg_sq"].abs().max()) > 0


@pytest.mark.gpu
def test_temperature(gpu):
    """policy_temperature 0.7 and mask_entropy: Learn hands both to every minibatch."""
    run_case(gpu, "temperature", dict(BASE, policy_temperature=0.7, mask_entropy=True), temperature=0.7, mask_entropy=True)


@pytest.mark.gpu
def test_default_kind(gpu):
    """The default activation (leaky_relu: the row-fused training path) through Learn, against a twin PPO handle loaded
    with p_k and driven from Python over the same schedule: every step's gradient within 1e-5 normwise (whether it is
    bit-equal is printed).  Schedule, order and update checks as for the other cases; the last step's grad-norm metrics
    against the norms of the recorded gradient itself, within the (1e-7 + 7e-7) of the fp32 sum of squares."""
    import torch
    from rlgpu.ppo import PPO
    kw = dict(BASE, activation="leaky_relu")
    L, recs = run_learn(gpu, kw)
    rec = recs[0]
    twin = PPO(obs_size=L.W, policy_layers=WIDTHS, critic_layers=WIDTHS, max_rows=L.T * L.P, seed=1, init=False, device=gpu)
    try:
        M, orders, sched = orders_of(gpu, L, rec, None)
        check_schedule(rec, sched, 0)
        u, engaged, idle = check_updates(L, rec, "default_kind")
        D = rec["dev"]
        sizes = [L.ppo.model_range(m)[1] for m in (0, 1)]
        worst, equal = 0.0, True
        for k, (s, entry) in enumerate(zip(rec["steps"], sched)):
            for m, part in zip((0, 1), split(s["params"], sizes)):
                twin.model_slice(m).copy_(part.to(gpu))
            twin.refresh_half()
            b0, b1 = lr.entry_range(entry)
            order = torch.from_numpy(orders[entry[0]].astype(np.int32)).to(gpu)
            twin.adv_normalizer(D["adv"][order[b0:b1].long()].contiguous())
            twin.zero_grad()
            for s0, n in entry[2]:
                twin.minibatch(D["obs"], D["masks"], D["acts"], D["old"], D["adv"], D["tgt"], order, s0, n, kw["batch_size"])
            torch.cuda.synchronize()
            g, w = s["grads"].double(), twin.flat(grads=True).cpu().double()
            d = float((g - w).norm() / w.norm())
            worst, equal = max(worst, d), equal and torch.equal(s["grads"], twin.flat(grads=True).cpu())
            assert float(w.norm()) > 0 and d <= 1e-5, f"default_kind step {k}: ||g - twin|| / ||twin|| = {d:.3g}"
        for name, g in zip(("Policy", "Critic"), split(rec["steps"][-1]["grads"].double(), sizes)):
            want, got = float(g.norm()), rec["metrics"][f"{name} Grad Norm"]
            assert abs(got - want) <= (1e-7 + 7e-7) * want, (name, got, want)
        print(f"learn loop default_kind: M {M}, steps {len(sched)}, largest ||g - twin|| / ||twin|| {worst:.3g}, bit-equal "
              f"{equal}, update err / allowed {u:.3f}, clip engaged {engaged}, idle {idle}, seed {kw['seed']}")
    finally:
        twin.close()
        L.close()

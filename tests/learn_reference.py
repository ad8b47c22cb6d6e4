"""PPOLearner::Learn's loop around the minibatch body, restated for the tests of the host Learner's Learn
(test_learn_loop): which rows make which batch, what each batch's gradient is, and what one clip + optimizer step
makes of it.  Written from the reference (PPOLearner.cpp:322-530 and ExperienceBuffer::GetAllBatchesShuffled,
ExperienceBuffer.cpp:100-163), not from host/learner.cpp:

  * per epoch one shuffle of the M rows; the batches are consecutive ranges of batchSize of that order; with
    overbatching the remainder joins the last batch (a batch of up to 2 batchSize - 1 rows, and one short batch when
    M < batchSize), without it the remainder is dropped (no batch at all when M < batchSize)        ExperienceBuffer.cpp:143-160
  * per batch the advantages of exactly its rows are normalised, (adv - mean) / (std(unbiased) + 1e-8)  PPOLearner.cpp:364-370
  * the batch is walked in minibatches of miniBatchSize, the last one short; each is weighted
    (stop - start) / config.batchSize -- the configured size, also for an over-long or short batch     :374, :509-512
  * the gradients accumulate over the batch's minibatches; then one clip_grad_norm_(0.5) per model and one optimizer
    step (which drops the gradients)                                                                      :520-529
  * the report's six means divide by the number of minibatches run                                       :492, :537-543

The minibatch body and the rules an engine result is held to are ppo_reference's (minibatch_ref, side_conditions,
check_grads, one_element); the optimizer statements are test_optimizers' (restated_step, torch_step) and
test_ppo_variants' (adamw_optimizers).  Like minibatch_ref, batch_step and optimizer_step_ref are generic in the dtype:
on float64 they are the reference, on torch fp32 the yardstick.

This is a helper module: pytest does not rewrite its asserts, so every assert here carries its message.
"""
import numpy as np

import ppo_reference as pr


# ------------------------------------------------------------------ which rows, when
def batch_ranges_ref(M, batch_size, overbatching):
    """GetAllBatchesShuffled's batch boundaries over M shuffled rows, in closed form: floor(M / batch_size) full
    batches; with overbatching the remainder joins the last one (or is the only, short, batch); without it the
    remainder is dropped.  batch_size None: one batch of M."""
    if M <= 0:
        return []
    if batch_size is None:
        return [(0, M)]
    full, rem = divmod(M, batch_size)
    if full == 0:
        return [(0, M)] if overbatching else []
    out = [(i * batch_size, (i + 1) * batch_size) for i in range(full)]
    if overbatching and rem:
        out[-1] = (out[-1][0], M)
    return out


def learn_schedule(M, batch_size, mini_batch_size, overbatching, epochs):
    """[(epoch, batch, [(s0, n), ...])] in the order Learn runs them: s0 is the minibatch's first position in the
    epoch's order, n its row count; a batch's rows are order[s0 of its first minibatch : s0 + n of its last]."""
    out = []
    for epoch in range(epochs):
        for bi, (b0, b1) in enumerate(batch_ranges_ref(M, batch_size, overbatching)):
            out.append((epoch, bi, [(s0, min(mini_batch_size, b1 - s0)) for s0 in range(b0, b1, mini_batch_size)]))
    return out


def entry_range(entry):
    """(b0, b1) of a schedule entry."""
    mbs = entry[2]
    return mbs[0][0], mbs[-1][0] + mbs[-1][1]


def train_rows_ref(T, P, old_team):
    """The rows of a [T, P] rollout that Learn trains while an old version plays team old_team (the team of player p
    is p % 2): the other team's, t * P + 2 * q + (1 - old_team), time-major."""
    t, q = np.divmod(np.arange(T * (P // 2)), P // 2)
    return (t * P + 2 * q + (1 - old_team)).astype(np.int64)


# ------------------------------------------------------------------ one batch's gradient
def batch_step(mods, data, rows, schedule_entry, batch_size, **options):
    """The gradient one batch leaves for the optimizer, in the dtype of mods = (policy, critic).  data: numpy arrays
    "obs", "masks", "acts", "old", "adv", "tgt" over all rows; rows: the batch's row indices in its order
    (order[b0:b1]); schedule_entry: its learn_schedule entry; batch_size: the configured one (None: the batch is all
    rows, so its own length), passed to minibatch_ref unchanged: it weights every minibatch n / batch_size whatever the
    batch's length is.  options: minibatch_ref's.
    The advantages are normalised over exactly `rows` in float64 and then cast.
    Returns {"grads": the flat accumulated gradient (policy, then critic), "metrics" / "scales": [minibatches, 6],
    "side": side_conditions of every minibatch (None or a reason), "n": the minibatch row counts,
    "head_bias_scale": the sum of the minibatches' (the head's bias gradient is their sum, so are its roundings)}."""
    import torch
    rows = np.asarray(rows, np.int64)
    b0, b1 = entry_range(schedule_entry)
    assert b1 - b0 == rows.size, f"batch {schedule_entry[:2]}: {rows.size} rows for the range ({b0}, {b1})"
    dt = next(mods[0].parameters()).dtype
    denom = rows.size if batch_size is None else batch_size
    adv = data["adv"][rows].astype(np.float64)
    advn = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8) if rows.size > 1 else adv  # :364 numel() > 1
    T = torch.from_numpy
    slope_free = pr.Case("learn", data["obs"].shape[1], data["masks"].shape[1], (), (), slope=1.0)
    grads, metrics, scales, side, ns, head = None, [], [], [], [], 0.0
    for s0, n in schedule_entry[2]:
        sl = slice(s0 - b0, s0 - b0 + n)
        r = rows[sl]
        ref = pr.minibatch_ref(mods[0], mods[1], T(data["obs"][r]).to(dt), T(data["masks"][r]), T(data["acts"][r]),
                               T(data["old"][r]).to(dt), T(advn[sl]).to(dt), T(data["tgt"][r]).to(dt), denom, **options)
        grads = ref["grads"] if grads is None else grads + ref["grads"]
        metrics.append(ref["metrics"])
        scales.append(ref["scales"])
        side.append(pr.side_conditions(slope_free, ref, T(data["masks"][r])))
        ns.append(n)
        head += ref["head_bias_scale"]
    return {"grads": grads, "metrics": np.array(metrics), "scales": np.array(scales), "side": side, "n": ns,
            "head_bias_scale": head}


# ------------------------------------------------------------------ one clip + one optimizer step
def optimizer_step_ref(kind, params, grads, state, step, lrs, max_norm, dtype, weight_decay=1e-2):
    """clip_grad_norm_(max_norm) and one step of optimizer `kind` per model, from given parameters, gradients and
    optimizer state, in `dtype` (float64: the reference; float32: the yardstick).  params / grads: one flat tensor per
    model (every optimizer here is elementwise but for its per-model norms, so a model is one tensor); state: {"exp_avg":
    [...], "exp_avg_sq": [...]} per model (adagrad's sum and rmsprop's square average live in exp_avg_sq, as in the
    engine); step: the steps taken before this one.  adamw / adam: torch.optim.AdamW with the state loaded
    (test_ppo_variants.adamw_optimizers; adam: weight_decay 0); the others: test_optimizers.restated_step.
    Returns (the new flat parameters per model, the unclipped gradient norms, the clip coefficients)."""
    import torch
    from test_optimizers import clip_coef, restated_step, torch_step
    from test_ppo_variants import adamw_optimizers
    ps = [torch.nn.Parameter(p.detach().to(dtype).clone()) for p in params]
    gs = [g.detach().to(dtype).clone() for g in grads]
    norms = [float(g.double().norm()) for g in gs]
    if kind in ("adamw", "adam"):
        opts = adamw_optimizers([[p] for p in ps], lrs, 0.0 if kind == "adam" else weight_decay)
        for k, (p, g, o) in enumerate(zip(ps, gs, opts)):
            p.grad = g
            o.state[p] = {"step": torch.tensor(float(step)), "exp_avg": state["exp_avg"][k].detach().to(dtype).clone(),
                          "exp_avg_sq": state["exp_avg_sq"][k].detach().to(dtype).clone()}
            torch_step(kind, [p], o, max_norm)
    else:
        for k, (p, g) in enumerate(zip(ps, gs)):
            with torch.no_grad():
                restated_step(kind, [p], [g], [state["exp_avg_sq"][k].detach().to(dtype).clone()], lrs[k], max_norm)
    coefs = [clip_coef([g], max_norm) for g in grads]
    return [p.detach() for p in ps], norms, coefs


# ------------------------------------------------------------------ torch modules of flat engine parameters
def modules_from_flat(flat, obs_size, num_actions, policy_layers, critic_layers, layer_norm, activation, dtype):
    """(policy, critic) torch modules in `dtype` holding the engine's flat fp32 parameters (policy, then critic: PPO.flat()
    order, which is torch's parameters() order): ppo_reference.make_engine's loading, in the other direction."""
    import torch
    from rlgpu.ppo import make_sequential
    mods = [make_sequential(obs_size, num_actions, policy_layers, layer_norm, 0.01, activation),
            make_sequential(obs_size, 1, critic_layers, layer_norm, 0.01, activation)]
    flat = flat.detach().cpu().float()
    o = 0
    with torch.no_grad():
        for m in mods:
            for prm in m.parameters():
                prm.copy_(flat[o:o + prm.numel()].view_as(prm))
                o += prm.numel()
    assert o == flat.numel(), f"{flat.numel()} flat parameters for modules of {o}"
    return [m.to(dtype) for m in mods]


"""Obs standardisation on the device (LearnerConfig::standardizeObs; Learner.cpp:679-693, Util/WelfordStat.h:69-243).

The reference below is a numpy restatement of the reference's arithmetic: the fp64 Welford increment over the drawn
rows in draw order, the coefficients in fp64 -> fp32, and the fp32 rewrite as a rounded product and a rounded add (numpy
rounds each ufunc on its own).  Its draws come from rlgpu_obs_sample_rows.  Everything on the device is compared with
it bit for bit: the state (count, means, m2) and the rewritten rows.

  * CPU: the host draw rule (deterministic, in range, seed-dependent, splittable by count, with replacement).
  * GPU, rlgpu_obs_stat_step: five steps from a zero state and a sixth after a download / upload of the state, for
    shapes that take every path of the row rewrite (16-byte body, scalar head of a view that starts at row 1, scalar
    tail) and of the update (S < rows, S = rows, S = 1), on inputs that take every branch of the coefficients.
  * GPU, Learner: the rollout's rows against the restatement over the raw rows a step hook records; hooked against
    fused collection; the trajectory mode; the collection path and the refusals; the feature off.
"""
import numpy as np
import pytest

W = 167
SEED = 0x5EED1234ABCD
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ the restatement
class RefStat:
    def __init__(self, width=W):
        self.count, self.mean, self.m2 = 0, np.zeros(width, F64), np.zeros(width, F64)

    def step(self, x, seed, max_samples=100, mean_range=3.0, min_std=0.1):
        """One reference step on x [P, W] fp32: returns (rewritten copy, info on the branches taken)."""
        from rlgpu.learner import obs_sample_rows
        x = np.ascontiguousarray(x, F32)
        P = x.shape[0]
        S = min(P, max_samples)
        rows = obs_sample_rows(seed, self.count, P, S)
        for r in rows:
            delta = x[r].astype(F64) - self.mean
            delta_n = delta / F64(self.count + 1)
            self.mean = self.mean + delta_n
            self.m2 = self.m2 + (delta * delta_n) * F64(self.count)
            self.count += 1
        info = {"active": self.count >= 2, "rows": rows}
        if self.count < 2:
            return x.copy(), info
        var = self.m2 / F64(self.count - 1)
        std = np.where(var > 0, np.sqrt(np.where(var > 0, var, 1.0)), 1.0)
        mn, mr = F64(F32(min_std)), F64(F32(mean_range))
        cstd = np.where(std > mn, std, mn)
        lo = np.where(self.mean > -mr, self.mean, -mr)
        cmean = np.where(lo < mr, lo, mr)
        inv = F32(1.0) / cstd.astype(F32)
        shift = -(cmean.astype(F32)) * inv
        out = x * inv[None, :]
        out = out + shift[None, :]
        info.update(var_zero=var <= 0, std_clamped=std < mn, mean_hi=self.mean > mr, mean_lo=self.mean < -mr)
        return out.astype(F32), info


def _inputs(rows, step):
    """[rows, W] fp32 whose columns take every branch: 0 constant (var = 0), 1 noise of 1e-3 (min-std clamp), 2 / 3
    around +50 / -50 (both mean clamps), 4 / 5 of 1e4 scale, a -0.0 at [0, 7]; the rest unit noise."""
    rng = np.random.default_rng(1000 + 7 * step + rows)
    x = rng.standard_normal((rows, W)).astype(F32)
    x[:, 0] = F32(0.25)
    x[:, 1] *= F32(1e-3)
    x[:, 2] += F32(50)
    x[:, 3] -= F32(50)
    x[:, 4:6] *= F32(1e4)
    x[0, 7] = F32(-0.0)
    return x


# ------------------------------------------------------------------ CPU: the draws
def test_sample_rows_host_rule():
    from rlgpu.learner import obs_sample_rows
    a = obs_sample_rows(SEED, 0, 16384, 500)
    assert np.array_equal(a, obs_sample_rows(SEED, 0, 16384, 500))
    for rows in (1, 4, 5, 16384):
        d = obs_sample_rows(SEED, 3, rows, 2000)
        assert d.min() >= 0 and d.max() < rows, rows
    assert (obs_sample_rows(SEED, 0, 1, 50) == 0).all()
    assert len(np.unique(obs_sample_rows(SEED, 0, 16384, 2000))) > 1500  # spread over the range, not stuck
    assert not np.array_equal(a, obs_sample_rows(SEED + 1, 0, 16384, 500))
    # the counter of draw i is count + i: two calls over c .. c + n - 1 are one call
    c = (1 << 32) - 40  # across the counter's low word
    whole = obs_sample_rows(SEED, c, 1000, 100)
    assert np.array_equal(whole, np.concatenate([obs_sample_rows(SEED, c, 1000, 37), obs_sample_rows(SEED, c + 37, 1000, 63)]))
    # with replacement: more draws than rows repeat rows
    d = obs_sample_rows(SEED, 0, 4, 64)
    assert len(d) == 64 and set(d.tolist()) <= {0, 1, 2, 3} and len(set(d.tolist())) > 1


def test_restatement_takes_every_branch():
    """The inputs reach the constant column, both clamps and the inactive first step on the restatement alone."""
    st = RefStat()
    x = _inputs(100, 0)
    out, info = st.step(x, SEED)
    assert info["active"] and info["var_zero"][0] and not info["var_zero"][1:].any()
    assert info["std_clamped"][1] and not info["std_clamped"][2:].any()
    assert info["mean_hi"][2] and info["mean_lo"][3] and not info["mean_hi"][6:].any() and not info["mean_lo"][6:].any()
    assert np.array_equal(out[:, 0], np.full(100, F32(0.25) * F32(1.0) + F32(-0.25)))  # std 1, mean inside the clamp
    assert abs(float(out[:, 2].mean()) - 47.0 * float(1.0 / np.sqrt(st.m2[2] / (st.count - 1)))) < 1.0  # (x - 3) / std
    one = RefStat()
    out, info = one.step(x, SEED, max_samples=1)
    assert not info["active"] and one.count == 1 and np.array_equal(out.view(np.uint32), x.view(np.uint32))


# ------------------------------------------------------------------ GPU: rlgpu_obs_stat_step
def _device_state(state):
    b = state.cpu().numpy()
    return (int(b[:8].view(np.int64)[0]), b[8:8 + 8 * W].view(np.uint64).copy(),
            b[8 + 8 * W:8 + 16 * W].view(np.uint64).copy())


# rows, max_samples, the first row of the view inside its buffer (1: the view starts 668 B into it, off the 16-byte grid)
CASES = [(4, 100, 0), (5, 100, 0), (5, 100, 1), (100, 100, 0), (1000, 100, 0), (16, 100, 0), (5, 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows, max_samples, first", CASES)
def test_obs_stat_step_bit_exact(gpu, rows, max_samples, first):
    import torch
    from rlgpu.learner import obs_stat_bytes, obs_stat_step
    nbytes = obs_stat_bytes(W)
    assert nbytes >= 8 + 16 * W
    state = torch.zeros(nbytes, dtype=torch.uint8, device=gpu)
    buf = torch.zeros((first + rows + 1, W), dtype=torch.float32, device=gpu)  # a guard row behind, `first` before
    ref = RefStat()
    seen = {"var_zero": False, "std_clamped": False, "mean_hi": False, "mean_lo": False, "inactive": False}
    for step in range(6):
        x = _inputs(rows, step)
        want, info = ref.step(x, SEED, max_samples)
        if info["active"]:
            seen["var_zero"] |= bool(info["var_zero"][0])
            seen["std_clamped"] |= bool(info["std_clamped"][1])
            seen["mean_hi"] |= bool(info["mean_hi"][2])
            seen["mean_lo"] |= bool(info["mean_lo"][3])
        else:
            seen["inactive"] = True
            assert np.array_equal(want.view(np.uint32), x.view(np.uint32)) and np.signbit(want[0, 7])
        if step == 5:  # resume: only (count, means, m2) travel, into a fresh block
            kept = state[:8 + 16 * W].cpu()
            state = torch.zeros(nbytes, dtype=torch.uint8, device=gpu)
            state[:8 + 16 * W] = kept.to(gpu)
        buf.fill_(7.0)
        buf[first:first + rows] = torch.from_numpy(x).to(gpu)
        obs_stat_step(state, buf[first:first + rows], SEED, max_samples)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        cnt, mean, m2 = _device_state(state)
        assert cnt == ref.count == min(rows, max_samples) * (step + 1), (step, cnt)
        assert np.array_equal(mean, ref.mean.view(np.uint64)), (step, "means")
        assert np.array_equal(m2, ref.m2.view(np.uint64)), (step, "m2")
        bad = np.argwhere(got[first:first + rows].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (step, bad[:4], got[first:first + rows][tuple(bad[0])], want[tuple(bad[0])])
        assert (got[:first] == 7.0).all() and (got[first + rows:] == 7.0).all(), "wrote outside the rows"
    # the restatement reached every branch on these inputs (else the comparison above covered less than it claims)
    assert seen["var_zero"] and seen["std_clamped"] and seen["mean_hi"] and seen["mean_lo"], seen
    assert seen["inactive"] == (max_samples == 1), seen
    if max_samples == 1:
        assert ref.count == 6


@pytest.mark.gpu
def test_obs_stat_step_refuses_bad_arguments(gpu):
    import torch
    from rlgpu._lib import RLGPUError
    from rlgpu.learner import obs_stat_bytes, obs_stat_step
    state = torch.zeros(obs_stat_bytes(W), dtype=torch.uint8, device=gpu)
    x = torch.zeros((4, W), dtype=torch.float32, device=gpu)
    for kw, word in ((dict(min_std=0.0), "min_std"), (dict(min_std=float("nan")), "min_std"),
                     (dict(max_mean_range=-1.0), "max_mean_range"), (dict(max_samples=0), "max_samples")):
        with pytest.raises(RLGPUError, match=r"\(-1\).*" + word):
            obs_stat_step(state, x, SEED, **kw)


# ------------------------------------------------------------------ GPU: the Learner
BASE = dict(num_arenas=8, rollout_len=8, mini_batch_size=128, policy_layers=(64, 64), critic_layers=(64, 64), seed=21,
            train_against_old_versions=False, max_episode_duration=0.27)  # episodes of 4 steps end truncated (code 2)
S = 32  # min(players, max_obs_samples) = min(4 * 8, 100)


def _learner(gpu, **kw):
    from rlgpu.learner import Learner, LearnerConfig
    return Learner(LearnerConfig(**{**BASE, **kw}), device=gpu)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _stat_bits(L):
    n, mean, m2 = L.obs_stat.get()
    return n, mean.view(np.uint64).tolist(), m2.view(np.uint64).tolist()


def _record(L):
    """A step hook that only records: the raw pre-reset rows (phase 0) and the raw post-reset rows (phase 1)."""
    import torch
    torch.cuda.synchronize()
    raw, pre = [L.env.obs.cpu().numpy().copy()], []

    def hook(phase):
        torch.cuda.synchronize()
        (pre if phase == 0 else raw).append(L.env.obs.cpu().numpy().copy())
    L.set_step_hook(hook)
    return raw, pre


def _same_rows(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


@pytest.mark.gpu
def test_learner_rows_follow_the_restatement(gpu):
    import torch
    L = _learner(gpu, standardize_obs=True)
    T = L.T
    raw, pre = _record(L)
    ref = RefStat()
    L.collect()
    torch.cuda.synchronize()
    assert len(raw) == T + 1 and len(pre) == T
    obs = L.obs.cpu().numpy()
    outs = [ref.step(raw[k], BASE["seed"])[0] for k in range(T + 1)]
    assert not np.array_equal(outs[3], raw[3])  # the rewrite is active
    for k in range(T + 1):
        _same_rows(obs[k], outs[k], ("row", k))
    assert _stat_bits(L) == (S * (T + 1), ref.mean.view(np.uint64).tolist(), ref.m2.view(np.uint64).tolist())
    terms, trunc = L.terms.cpu().numpy(), L.trunc_obs.cpu().numpy()
    assert (terms == 2).any(), "no truncation: the raw truncation rows were not exercised"
    for t in range(T):
        sel = terms[t] == 2
        _same_rows(trunc[t][sel], pre[t][sel], ("trunc", t))  # raw, as the reference's traj.nextStates
    last = obs[T].copy()
    L.consume()
    L.learn()
    L.finish_iteration()
    L.collect()
    torch.cuda.synchronize()
    obs = L.obs.cpu().numpy()
    _same_rows(obs[0], last, "row 0 of iteration 2 is row T of iteration 1, not rewritten again")
    for k in range(1, T + 1):
        _same_rows(obs[k], ref.step(raw[T + k], BASE["seed"])[0], ("row", T + k))
    n, mean, m2 = L.obs_stat.get()
    assert n == S * (2 * T + 1) == ref.count
    assert np.array_equal(mean.view(np.uint64), ref.mean.view(np.uint64)) and np.array_equal(m2.view(np.uint64), ref.m2.view(np.uint64))
    assert L.obs_stat.to_json()["count"] == n and len(L.obs_stat.to_json()["vars"]) == W
    L.close()


@pytest.mark.gpu
def test_hooked_and_fused_collection_agree(gpu):
    import torch
    A, B = _learner(gpu, standardize_obs=True), _learner(gpu, standardize_obs=True)
    calls = []
    B.set_step_hook(calls.append)
    for L in (A, B):
        L.iterate()
    torch.cuda.synchronize()
    assert calls == [0, 1] * A.T
    for name in ("obs", "masks", "actions", "logp", "rewards", "terms", "values", "adv", "target"):
        assert torch.equal(_bits(getattr(A, name)), _bits(getattr(B, name))), name
    sel = A.terms == 2
    assert sel.any() and torch.equal(_bits(A.trunc_obs[sel]), _bits(B.trunc_obs[sel]))
    assert _stat_bits(A) == _stat_bits(B) and _stat_bits(A)[0] == S * (A.T + 1)
    assert torch.equal(_bits(A.ppo.params), _bits(B.ppo.params))
    A.close()
    B.close()


@pytest.mark.gpu
def test_trajectory_mode_rows(gpu):
    import torch
    L = _learner(gpu, standardize_obs=True, experience_mode=1, ts_per_itr=96)
    raw, pre = _record(L)
    L.collect()
    L.consume()
    torch.cuda.synchronize()
    b = L.batch()
    steps, Tm = b["steps"], b["store_rows"]
    assert b["first_step"] == 0 and 0 < steps < Tm and b["num_rows"] >= 96 and len(raw) == steps + 1
    ref = RefStat()
    store = L.obs.cpu().numpy()
    for k in range(steps + 1):  # store row k = the obs the step at row k acted on (the first iteration does not wrap)
        _same_rows(store[k], ref.step(raw[k], BASE["seed"])[0], ("store row", k))
    assert L.obs_stat.get()[0] == S * (steps + 1) == ref.count
    cobs = b["obs"].cpu().numpy()
    segs = [b[k].cpu().numpy() for k in ("seg_player", "seg_start", "seg_len", "seg_off", "seg_code", "seg_tidx")]
    trunc = b["trunc_obs"].cpu().numpy()
    ntr = 0
    for p, st, ln, off, code, tidx in zip(*segs):
        for j in range(ln):
            _same_rows(cobs[off + j], store[(st + j) % Tm, p], ("combined row", int(off + j)))
        if code == 2:
            _same_rows(trunc[tidx], pre[st + ln - 1][p], ("trunc row", int(tidx)))  # raw pre-reset row of its last step
            ntr += 1
    assert ntr == b["num_truncs"] > 0
    L.learn()
    L.finish_iteration()
    L.close()


@pytest.mark.gpu
def test_collection_takes_the_per_step_path(gpu):
    """collect_groups = -1 (the collection loop) and 2 (arena groups) with the feature on still train, on the
    one-launch-per-step path: the same rollout, statistic and parameters as collect_groups = 1, env_launch_arenas =
    all arenas, and per-step env timings (the loop reports T equal shares of one launch)."""
    import torch
    Ls = [_learner(gpu, standardize_obs=True, collect_groups=g) for g in (1, -1, 2)]
    reps = []
    for L in Ls:
        L.set_env_timing(True)
        before = L.ppo.params.clone()
        reps.append(L.iterate())
        assert not torch.equal(before, L.ppo.params)
    torch.cuda.synchronize()
    for L, rep in zip(Ls[1:], reps[1:]):
        for name in ("obs", "actions", "logp", "rewards", "terms", "adv"):
            assert torch.equal(_bits(getattr(Ls[0], name)), _bits(getattr(L, name))), (L.cfg.collect_groups, name)
        assert _stat_bits(L) == _stat_bits(Ls[0]) and _stat_bits(L)[0] == S * (L.T + 1)
        assert torch.equal(_bits(Ls[0].ppo.params), _bits(L.ppo.params))
        assert rep["env_launch_arenas"] == BASE["num_arenas"]
        assert not (rep["env_kernel_min_ms"] == rep["env_kernel_median_ms"] == rep["env_kernel_max_ms"]), rep
    # without the feature the same configs leave that path: 2 groups step half the arenas per launch
    G = _learner(gpu, collect_groups=2)
    assert G.iterate()["env_launch_arenas"] == BASE["num_arenas"] // 2
    for L in Ls + [G]:
        L.close()


@pytest.mark.gpu
def test_refusals_name_the_field(gpu):
    from rlgpu._lib import RLGPUError
    from rlgpu.learner import _ObsStat
    L = _learner(gpu)
    with pytest.raises(RLGPUError, match=r"\(-4\).*not enabled"):
        _ObsStat(L).get()  # rlgpu_learner_get_obs_stat before enabling
    with pytest.raises(RLGPUError, match=r"\(-1\).*min_std"):
        L.set_obs_standardization(True, min_std=0.0)
    with pytest.raises(RLGPUError, match=r"\(-1\).*min_std"):
        L.set_obs_standardization(True, min_std=-0.5)
    with pytest.raises(RLGPUError, match=r"\(-1\).*max_mean_range"):
        L.set_obs_standardization(True, max_mean_range=float("inf"))
    with pytest.raises(RLGPUError, match=r"\(-1\).*max_samples"):
        L.set_obs_standardization(True, max_samples=0)
    L.collect()
    with pytest.raises(RLGPUError, match=r"\(-4\).*standardize_obs.*first collection"):
        L.set_obs_standardization(True)
    L.close()
    K = _learner(gpu, frame_stack=2)
    with pytest.raises(RLGPUError, match=r"\(-5\).*frame_stack"):
        K.set_obs_standardization(True)
    K.close()
    with pytest.raises(RLGPUError, match=r"\(-5\).*frame_stack"):
        _learner(gpu, frame_stack=2, standardize_obs=True)
    M = _learner(gpu, standardize_obs=True)
    M.collect()
    with pytest.raises(RLGPUError, match=r"\(-4\).*first collection"):
        M.obs_stat.set(0, np.zeros(W), np.zeros(W))
    M.close()


@pytest.mark.gpu
def test_feature_off_is_the_default_path(gpu):
    """A learner told set_obs_standardization(0, ...) collects and trains bit for bit what one that never heard of the
    setter does, and neither allocates the statistic."""
    import torch
    from rlgpu._lib import RLGPUError
    A, B = _learner(gpu), _learner(gpu)
    B.set_obs_standardization(False, 0.5, 1.0, 7)
    assert B.obs_stat is None
    for L in (A, B):
        L.iterate()
    torch.cuda.synchronize()
    for name in ("obs", "masks", "actions", "logp", "rewards", "terms", "values", "adv", "target", "ret"):
        assert torch.equal(_bits(getattr(A, name)), _bits(getattr(B, name))), name
    assert torch.equal(_bits(A.ppo.params), _bits(B.ppo.params))
    from rlgpu.learner import _ObsStat
    with pytest.raises(RLGPUError, match=r"\(-4\)"):
        _ObsStat(B).get()
    # and on differs from off: the same learner with the feature on rewrites its rows
    C = _learner(gpu, standardize_obs=True)
    raw0 = C.env.obs.clone()
    assert torch.equal(_bits(C.obs[0]), _bits(raw0))  # row 0 waits for the first collection (and a checkpoint's state)
    C.collect()
    torch.cuda.synchronize()
    assert not torch.equal(_bits(C.obs[0]), _bits(raw0))
    for L in (A, B, C):
        L.close()

"""The collection loop (rlgpu_learner_config.collect_groups = -1, rlgpu_envset_collect_loop: the whole rollout in one
launch, every env workgroup looping over the T steps of its own 4 arenas with the policy forward of its 16 players
inside it) against the per-step collection (collect_groups = 1), byte for byte: every rollout array, the arena
records, the StepCallback totals and counts and the parameters after each of two iterations.  8 arenas (two full
workgroups) and 6 (the last workgroup half empty); a 4-step episode cap gives truncations without a reset (code 2) inside
the loop, and arena 1 starts with the ball in a goal, so with a GoalScoreCondition its first step ends NORMAL (code 1) and it is reset inside
the loop.  The second iteration covers the carry of row T into row 0 and of the StepCallback call counter (T = 6 is
no multiple of its every-4th-call cadence)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROLLOUT = ("obs", "masks", "actions", "logp", "rewards", "terms", "values", "adv", "target", "ret")


def _learner(gpu, n, groups, **kw):
    from rlgpu import plugins
    from rlgpu.learner import Learner, LearnerConfig
    kw.setdefault("terminals", [plugins.terminal("NoTouchCondition", 8), plugins.terminal("GoalScoreCondition")])
    cfg = LearnerConfig(**{**dict(num_arenas=n, rollout_len=6, mini_batch_size=64, seed=11, max_episode_duration=0.27,
                                  collect_groups=groups, train_against_old_versions=False), **kw})
    L = Learner(cfg, device=gpu)
    # arena 1: the ball at rest deep inside a goal (a goal is |y| > 5215.5 uu; records are in Bullet units, uu / 50)
    from rlgpu.state import ARENA
    rec = np.frombuffer(L.env.get_arenas(1, 1).tobytes(), ARENA).copy()
    rec["ball"]["pos"][0] = (0.0, 5700.0 / 50.0, 200.0 / 50.0)
    rec["ball"]["vel"][0] = 0.0
    rec["ball"]["angvel"][0] = 0.0
    L.env.set_arenas(rec.view(np.uint8), 1)
    return L


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _metric_sums(L):
    from rlgpu import _lib
    tot, cnt = np.zeros(8, np.float64), np.zeros(8, np.uint64)
    _lib.check(_lib.lib().rlgpu_learner_step_metrics(L._h, tot.ctypes.data, cnt.ctypes.data, 0), "step_metrics")
    return tot.view(np.uint64).tolist(), cnt.tolist()


def _same(A, B, what):
    import torch
    torch.cuda.synchronize()
    for name in ROLLOUT:
        assert torch.equal(_bits(getattr(A, name)), _bits(getattr(B, name))), (what, name)
    sel = A.terms == 2
    assert torch.equal(_bits(A.trunc_obs[sel]), _bits(B.trunc_obs[sel])), (what, "trunc_obs")
    assert np.array_equal(A.env.get_arenas(), B.env.get_arenas()), (what, "arena records")
    assert _metric_sums(A) == _metric_sums(B), (what, "step metrics")
    assert torch.equal(_bits(A.ppo.flat()), _bits(B.ppo.flat())), (what, "parameters")


@pytest.mark.parametrize("n", (8, 6))
def test_loop_equals_per_step_collection(gpu, n):
    A, B = _learner(gpu, n, 1), _learner(gpu, n, -1)
    B.set_env_timing(True)
    seen = set()
    for it in range(2):
        ra, rb = A.iterate(), B.iterate()
        assert ra["env_launch_arenas"] == n and rb["env_launch_arenas"] == n
        # one launch, reported as its T equal shares
        assert rb["env_kernel_ms"] > 0
        assert rb["env_kernel_min_ms"] == rb["env_kernel_median_ms"] == rb["env_kernel_max_ms"]
        _same(A, B, (n, it))
        seen |= set(np.unique(B.terms.cpu().numpy()).tolist())
    assert {1, 2} <= seen, seen  # a NORMAL end with its reset and a truncation without one, inside the loop
    assert A.total_steps == B.total_steps == 2 * 6 * 4 * n  # agent steps
    A.close()
    B.close()


def test_old_version_iteration_takes_the_per_step_path(gpu):
    """The second iteration plays one team with an old version: the loop runs one set of weights, so that
    iteration is collected per step, and the next one in the loop again."""
    kw = dict(train_against_old_versions=True, train_against_old_chance=1.0)
    A, B = _learner(gpu, 8, 1, **kw), _learner(gpu, 8, -1, **kw)
    old = []
    for it in range(3):
        ra, rb = A.iterate(), B.iterate()
        assert ra["env_launch_arenas"] == rb["env_launch_arenas"] == 8
        assert ra["old_version"] == rb["old_version"]
        old.append(rb["old_version"] is not None)
        _same(A, B, ("old", it))
    assert old[0] is False and any(old[1:])
    A.close()
    B.close()


def test_step_hook_takes_the_per_step_path(gpu):
    A, B = _learner(gpu, 8, 1), _learner(gpu, 8, -1)
    calls = []
    B.set_step_hook(calls.append)
    ra, rb = A.iterate(), B.iterate()
    assert calls == [0, 1] * 6  # the hook ran after every step and every reset: not the loop
    assert ra["env_launch_arenas"] == rb["env_launch_arenas"] == 8
    _same(A, B, "hook")
    B.set_step_hook(None)
    ra, rb = A.iterate(), B.iterate()  # and without it, the loop again
    _same(A, B, "hook off")
    A.close()
    B.close()

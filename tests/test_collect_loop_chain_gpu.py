"""The collection loop kernel after its chain was shortened (the forward and the step body as called functions, the
forward's deeper weight prefetch; csrc/env_step.hpp) against the per-step collection, byte for byte, and its profiled
instantiation (rlgpu_envset_set_collect_split) against the default one.

collect_groups = -1 against collect_groups = 1: every rollout array, the arena records, the StepCallback sums and the
parameters after one Learn.  The shapes are the smallest that reach every path: 5 arenas (the last workgroup holds
one arena, its forward has 4 rows), 8 (two full workgroups) and 3 (one partial workgroup); T = 3 and 6; both 16-bit
inference formats; a 2-step episode cap gives truncation rows inside the launch and arena 1 starts with the ball in a
goal, so its first step ends the episode and it is reset inside the launch; the t = 0 forward reads rows the host's
launch wrote, the later ones rows the workgroup wrote."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROLLOUT = ("obs", "masks", "actions", "logp", "rewards", "terms", "values", "adv", "target", "ret")
SLOTS, PARTS = 8, 7  # include/rlgpu_env.h RLGPU_COLLECT_SPLIT_SLOTS; csrc/env_step.hpp kSplit*


def _learner(gpu, n, groups, T, fp16):
    from rlgpu import plugins
    from rlgpu.learner import Learner, LearnerConfig
    from rlgpu.state import ARENA
    cfg = LearnerConfig(num_arenas=n, rollout_len=T, mini_batch_size=64, seed=11, max_episode_duration=0.14,
                        collect_groups=groups, train_against_old_versions=False, infer_fp16=fp16,
                        terminals=[plugins.terminal("NoTouchCondition", 8), plugins.terminal("GoalScoreCondition")])
    L = Learner(cfg, device=gpu)
    # arena 1: the ball at rest deep inside a goal (a goal is |y| > 5215.5 uu; records are in Bullet units, uu / 50)
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


@pytest.mark.parametrize("fp16", (False, True), ids=("bf16", "fp16"))
@pytest.mark.parametrize("T", (3, 6))
@pytest.mark.parametrize("n", (5, 8, 3))
def test_loop_equals_per_step_collection(gpu, n, T, fp16):
    from rlgpu import _lib
    A, B = _learner(gpu, n, 1, T, fp16), _learner(gpu, n, -1, T, fp16)
    assert _lib.lib().rlgpu_envset_collect_loop_ok(B.env._h, B.ppo._h) == 1
    ra, rb = A.iterate(), B.iterate()
    assert ra["env_launch_arenas"] == n and rb["env_launch_arenas"] == n
    _same(A, B, (n, T, fp16))
    seen = set(np.unique(B.terms.cpu().numpy()).tolist())
    assert {1, 2} <= seen, seen  # a NORMAL end with its reset and a truncation without one, inside the launch
    assert A.total_steps == B.total_steps == T * 4 * n
    A.close()
    B.close()


@pytest.mark.parametrize("fp16", (False, True), ids=("bf16", "fp16"))
def test_profiled_instantiation_equals_the_default(gpu, fp16):
    """5 arenas, T = 3: the profiled instantiation leaves the default one's outputs, and every part's slot of both
    workgroups has counted."""
    import torch
    from rlgpu import _lib
    n, T = 5, 3
    A, B = _learner(gpu, n, -1, T, fp16), _learner(gpu, n, -1, T, fp16)
    wg = (n + 3) // 4
    slots = torch.zeros(wg * SLOTS, dtype=torch.int64, device=gpu)
    lib = _lib.lib()
    lib.rlgpu_envset_set_collect_split.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    assert lib.rlgpu_envset_set_collect_split(B.env._h, ctypes.c_void_p(slots.data_ptr()), wg * SLOTS - 1) != 0  # too small
    _lib.check(lib.rlgpu_envset_set_collect_split(B.env._h, ctypes.c_void_p(slots.data_ptr()), slots.numel()), "set_collect_split")
    A.iterate()
    B.iterate()
    _same(A, B, ("profiled", fp16))
    got = slots.view(wg, SLOTS).cpu().numpy()
    assert (got[:, :PARTS] > 0).all(), got
    assert (got[:, PARTS:] == 0).all(), got
    # off again: the default instantiation, which leaves the slots alone
    _lib.check(lib.rlgpu_envset_set_collect_split(B.env._h, None, 0), "set_collect_split off")
    A.iterate()
    B.iterate()
    _same(A, B, ("profiled off", fp16))
    assert np.array_equal(slots.view(wg, SLOTS).cpu().numpy(), got)
    A.close()
    B.close()

"""The host Learner gives back every persistent device allocation it makes (rlgpu_live_device_allocations).

The count is the library's own, per process: free device memory is device-wide and proves nothing on a shared card.
The baseline is taken after one warm-up Learner was created, iterated once and closed, so whatever the process
creates once and keeps already exists.  8 arenas, T = 4, minibatch 64, one epoch throughout:
  * a constructor that throws after the env set and the PPO handle exist (experience_capacity too small), or between
    the two (frame_stack = 17), leaves the count at the baseline;
  * create -> iterate -> close returns to the baseline for the rollout mode with an old-version team and truncated
    episodes (row selection, truncation gather buffers), the trajectory mode with stacked frames over two
    iterations (trajectory store, stage buffer, combined batch) and a guided rollout mode (guide logits);
  * while a Learner lives the count is above the baseline.
"""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

BASE = dict(num_arenas=8, rollout_len=4, mini_batch_size=64)


def live():
    from rlgpu import _lib
    f = _lib.lib().rlgpu_live_device_allocations
    f.restype = ctypes.c_int64
    return int(f())


@pytest.fixture(scope="module")
def baseline(gpu):
    from rlgpu.learner import Learner, LearnerConfig
    L = Learner(LearnerConfig(**BASE, epochs=1, train_against_old_versions=False), device=gpu)
    L.iterate()
    L.close()
    return live()


@pytest.mark.parametrize("extra, word", [(dict(), "experience_capacity"), (dict(frame_stack=17), "frame_stack")])
def test_failed_construction_releases_everything(gpu, baseline, extra, word):
    from rlgpu._lib import RLGPUError
    from rlgpu.learner import Learner, LearnerConfig
    cfg = LearnerConfig(**BASE, experience_mode=1, max_episode_duration=1.0, experience_capacity=1, **extra)
    with pytest.raises(RLGPUError, match=word):
        Learner(cfg, device=gpu)
    assert live() == baseline


def _old_team(L):
    """Rollout mode, team 0 acting with an old version for one iteration; episodes of 3 steps end truncated."""
    import torch
    from rlgpu import _lib
    L.ppo.set_version(L.ppo.policy_version())
    _lib.check(_lib.lib().rlgpu_learner_set_old_team(L._h, 0), "rlgpu_learner_set_old_team")
    L.collect()
    L.consume()
    torch.cuda.synchronize()
    assert bool((L.terms == 2).any()), "no truncated episode: the gather buffers were not exercised"
    L.learn()
    L.finish_iteration()


def _trajectories(L):
    L.iterate()
    L.iterate()
    assert L.batch()["num_rows"] > 0


def _guided(L):
    L.set_guide(L.ppo.policy_version().clone(), 0.03)
    L.iterate()
    assert L.guide_logits_view() is not None


@pytest.mark.parametrize("kw, run", [
    (dict(max_episode_duration=0.2), _old_team),
    (dict(experience_mode=1, frame_stack=2, max_episode_duration=0.3), _trajectories),
    (dict(), _guided),
], ids=["old_team_truncations", "trajectories_stacked", "guide"])
def test_create_iterate_close_returns_to_baseline(gpu, baseline, kw, run):
    import torch
    from rlgpu.learner import Learner, LearnerConfig
    L = Learner(LearnerConfig(**BASE, epochs=1, train_against_old_versions=False, **kw), device=gpu)
    assert live() > baseline
    run(L)
    torch.cuda.synchronize()
    assert live() > baseline
    L.close()
    assert live() == baseline

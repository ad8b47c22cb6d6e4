"""DefaultObs and DefaultObsPadded without a GPU: the widths the library reports and what it refuses, the Python
builder objects, the facade's translation of an EnvCreateFn's builder (rlgpu_obs_builder_plan, no device), and the
distribution of the padded builder's shuffles as the reference states them (tests/default_obs_reference.py).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import default_obs_reference as ref
from conftest import PKG


def test_obs_builder_size():
    from rlgpu import _lib
    from rlgpu.env import obs_builder_size
    assert obs_builder_size(0) == 167
    assert obs_builder_size(0, 5) == 167  # max_players is DefaultObsPadded's alone
    assert obs_builder_size(1) == 127
    assert obs_builder_size(2, 2) == 127
    assert obs_builder_size(2, 3) == 165
    L = _lib.lib()
    L.rlgpu_obs_builder_size.argtypes = [ctypes.c_int32, ctypes.c_int32]
    for bad, name in ((1, "maxPlayers 1"), (0, "maxPlayers 0"), (4, "maxPlayers 4"), (1 << 30, "maxPlayers")):
        assert L.rlgpu_obs_builder_size(2, bad) == -1
        assert name in _lib.last_error(), _lib.last_error()
    assert "teammate" in (L.rlgpu_obs_builder_size(2, 1), _lib.last_error())[1]
    assert "167" in (L.rlgpu_obs_builder_size(2, 4), _lib.last_error())[1]
    assert L.rlgpu_obs_builder_size(3, 2) == -1 and "obs builder 3" in _lib.last_error()
    assert L.rlgpu_obs_builder_size(-1, 2) == -1 and "obs builder -1" in _lib.last_error()
    with pytest.raises(_lib.RLGPUError, match="maxPlayers 4"):
        obs_builder_size(2, 4)
    assert ref.width(ref.spec(ref.DEFAULT)) == 127 and ref.width(ref.spec(ref.PADDED, 3)) == 165


def test_python_builders():
    from rlgpu import env
    from rlgpu.env import ADVANCED_OBS, DefaultObs, DefaultObsPadded, obs_builder_spec
    from rlgpu.learner import LearnerConfig
    assert (ADVANCED_OBS.kind, ADVANCED_OBS.obs_size) == (0, 167)
    assert obs_builder_spec(None) is ADVANCED_OBS
    d = DefaultObs()
    assert (d.kind, d.obs_size) == (1, 127)
    f = np.float32
    assert d.pos_coef == (float(f(1) / f(4096)), float(f(1) / f(5120)), float(f(1) / f(2044)))
    assert d.vel_coef == float(f(1) / f(2300)) and d.ang_vel_coef == float(f(1) / f(5.5))
    c = DefaultObs(pos_coef=(0.5, 0.25, 2), vel_coef=0.1, ang_vel_coef=3)
    assert c.pos_coef == (0.5, 0.25, 2.0) and c.vel_coef == float(f(0.1)) and c.ang_vel_coef == 3.0
    assert [DefaultObsPadded(m).obs_size for m in (2, 3)] == [127, 165]
    p = DefaultObsPadded(3, vel_coef=0.5)
    assert (p.kind, p.max_players, p.vel_coef, p.pos_coef) == (2, 3, 0.5, d.pos_coef)
    cfg = env._Config()
    assert env.set_obs_builder(cfg, p) is p
    assert (cfg.obs_builder, cfg.obs_max_players, cfg.obs_vel_coef) == (2, 3, 0.5)
    assert tuple(cfg.obs_pos_coef) == d.pos_coef and cfg.obs_ang_vel_coef == d.ang_vel_coef
    cfg = env._Config()
    env.set_obs_builder(cfg, None)  # all zero: AdvancedObs
    assert (cfg.obs_builder, cfg.obs_max_players, tuple(cfg.obs_pos_coef), cfg.obs_vel_coef) == (0, 0, (0, 0, 0), 0)
    with pytest.raises(ValueError, match="max_players 1 leaves 0 teammate"):
        DefaultObsPadded(1)
    with pytest.raises(ValueError, match="max_players 4 makes rows of 203"):
        DefaultObsPadded(4)
    with pytest.raises(ValueError, match="must be an integer"):
        DefaultObsPadded(2.5)
    with pytest.raises(ValueError, match="vel_coef is not finite"):
        DefaultObs(vel_coef=float("nan"))
    with pytest.raises(ValueError, match="pos_coef is not finite"):
        DefaultObsPadded(2, pos_coef=(1, float("inf"), 1))
    with pytest.raises(ValueError, match="3 components"):
        DefaultObs(pos_coef=(1, 2))
    with pytest.raises(ValueError, match="all coefficients are zero"):
        DefaultObs((0, 0, 0), 0, 0)
    with pytest.raises(ValueError, match="is no obs builder"):
        obs_builder_spec("default")
    assert LearnerConfig().obs_builder is None
    assert LearnerConfig(obs_builder=p).obs_builder is p


def test_config_mirrors_hold_the_obs_fields():
    from rlgpu import _lib, env, learner
    L = _lib.lib()
    L.rlgpu_learner_config_size.restype = ctypes.c_int32
    assert env.config_size() == ctypes.sizeof(env._Config)
    assert L.rlgpu_learner_config_size() == ctypes.sizeof(learner._CConfig)
    obs = ["obs_builder", "obs_max_players", "obs_pos_coef", "obs_vel_coef", "obs_ang_vel_coef"]
    names = [f[0] for f in env._Config._fields_]
    i = names.index("obs_builder")
    assert names[i:i + 5] == obs
    lnames = [f[0] for f in learner._CConfig._fields_]
    i = lnames.index("n_state_setters") + 1  # next to the state setter
    assert lnames[i:i + 5] == obs


def _plan_lines():
    exe = os.path.join(PKG, "rlgpu", "rlgpu_obs_builder_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(line.split(": ", 1) for line in r.stdout.splitlines())


def test_facade_translates_the_builders():
    """An EnvCreateFn returning new DefaultObs() / new DefaultObsPadded(3), through EnvSetGPU::CreateEnvs (one call
    per arena, no device): the plan's kind and width; a subclass is refused by name."""
    out = _plan_lines()
    f = np.float32
    defaults = "coef %.9g %.9g %.9g %.9g %.9g" % tuple(float(x) for x in (f(1) / f(4096), f(1) / f(5120), f(1) / f(2044),
                                                                          f(1) / f(2300), f(1) / f(5.5)))
    assert out["none"] == out["advanced"] == "kind 0 width 167 max_players 0 coef 0 0 0 0 0"
    assert out["default"] == "kind 1 width 127 max_players 0 " + defaults
    assert out["default_coef"] == "kind 1 width 127 max_players 0 coef %.9g %.9g %.9g %.9g %.9g" % tuple(
        float(x) for x in (f(1) / f(4000), f(1) / f(5000), f(1) / f(2000), f(1) / f(2000), f(0.25)))
    assert out["padded2"] == "kind 2 width 127 max_players 2 " + defaults
    assert out["padded3"] == "kind 2 width 165 max_players 3 " + defaults
    assert out["padded1"].startswith("refused: ") and "maxPlayers 1" in out["padded1"]
    assert out["padded4"].startswith("refused: ") and "maxPlayers 4" in out["padded4"]
    assert out["subclass"].startswith("refused: EnvCreateResult: obs builder ") and "UserDefaultObs" in out["subclass"]
    assert out["user"].startswith("refused: EnvCreateResult: obs builder ") and "UserObs" in out["user"]
    for k in ("differ", "differ_coef"):
        assert out[k].startswith("refused: EnvCreateFn(1) returned plugins that differ"), out[k]


def test_reference_shuffle_is_uniform():
    """24,000 (player, tick) keys at max_players = 3: each of the 6 opponent orders within 1/6 +- 0.02 (8 sigma of a
    fair draw: sigma = sqrt(5/36 / 24000) = 0.0024), both teammate orders within 1/2 +- 0.03 (sigma 0.0032)."""
    players, ticks = np.meshgrid(np.arange(240), 8 * np.arange(100), indexing="ij")
    team, opp = ref.shuffles(1234, players.ravel(), ticks.ravel(), 3)
    assert team.shape == (24000, 2) and opp.shape == (24000, 3)
    assert (np.sort(opp, axis=1) == np.arange(3)).all() and (np.sort(team, axis=1) == np.arange(2)).all()
    code = opp[:, 0] * 9 + opp[:, 1] * 3 + opp[:, 2]
    orders, counts = np.unique(code, return_counts=True)
    assert len(orders) == 6
    assert (np.abs(counts / 24000 - 1 / 6) <= 0.02).all(), counts
    share = (team[:, 0] == 0).mean()
    assert abs(share - 0.5) <= 0.03 and abs((team[:, 0] == 1).mean() - 0.5) <= 0.03, share
    # max_players = 2: one teammate slot, two opponent orders on the same draw as the last swap above
    team2, opp2 = ref.shuffles(1234, players.ravel(), ticks.ravel(), 2)
    assert team2.shape == (24000, 1) and not team2.any()
    assert abs((opp2[:, 0] == 0).mean() - 0.5) <= 0.03
    # another seed gives another sequence; the same key gives the same one
    assert (ref.shuffles(1235, players.ravel(), ticks.ravel(), 3)[1] != opp).any()
    assert (ref.shuffles(1234, players.ravel(), ticks.ravel(), 3)[1] == opp).all()

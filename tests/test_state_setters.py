"""RandomState and CombinedState as device state setters, the part that needs no GPU.

* the reference helper's generator (tests/state_setter_reference.py) is anchored to the engine's Philox stream:
  the oracle's FuzzedKickoffState is rebuilt from its plain kickoff plus the helper's 12 draws, field for field
  bit-equal (64 arenas, two seeds), and philox0 equals the oracle's own on three known counters;
* the reference's invariants over 256 arenas for each of the 8 flag sets: the source's position bounds, on-ground
  cars at z 17 with zero pitch / roll / vel.z / angular velocity, orthonormal rotation rows, the documented draw
  count; CombinedState with weights (1, 0) and (0, 1);
* the oracle steps 6 steps from reference states with fast cars in the air (the inputs of the GPU tests);
* both ctypes config mirrors equal the library's _size() exports;
* rlgpu.env's spec validation names the entry at fault, and so does rlgpu_envset_create (it validates the setter
  before any device work);
* the facade's translation, printed by the stand-alone rlgpu_state_setter_plan.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
import state_setter_reference as ref
from rlgpu.state import ARENA
from tests_util import arena_diff, random_actions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_BIN = os.path.join(ROOT, "reinforcement-learning_amd", "rlgpu", "rlgpu_state_setter_plan")
N_INV, SEED_INV = 256, 17


def _records(o):
    return np.frombuffer(o.get_arenas().tobytes(), ARENA).copy()


def test_philox_is_the_oracles():
    L = oracle.lib()
    L.oracle_philox.restype = ctypes.c_uint32
    L.oracle_philox.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]
    for seed, arena, counter in ((1, 2, 3), (0xDEADBEEFCAFE, 77, 123456), (2**64 - 1, 2**32 - 1, 2**32 - 1)):
        assert int(ref.philox0(seed, arena, counter)) == L.oracle_philox(seed, arena, counter)
    u = ref.uniform(np.array([0, 255, 256, 2**32 - 1], np.uint32))
    assert u.dtype == np.float32 and u.tolist() == [0.0, 0.0, 2.0**-24, 1.0 - 2.0**-24]


@pytest.mark.parametrize("seed", (3, 99))
def test_generator_rebuilds_the_oracles_fuzzed_kickoff(seed):
    n = 64
    kick = _records(oracle.EnvSet(n, seed=seed))
    fuzz = _records(oracle.EnvSet(n, seed=seed, state_setter=1))
    assert (kick["env"]["rng_counter"] == 4).all()
    for i in range(n):
        ref.fuzzed_kickoff(kick[i], seed, i)
    assert (kick["env"]["rng_counter"] == ref.draw_count(ref.FUZZED)).all()
    assert not arena_diff(kick, fuzz)
    moved = kick["cars"]["body"]["pos"] != _records(oracle.EnvSet(n, seed=seed))["cars"]["body"]["pos"]
    assert moved.any(axis=(1, 2)).all()  # the 12 draws did something in every arena


@pytest.fixture(scope="module")
def kickoffs():
    """256 oracle kickoff records, shared and left unchanged."""
    rec = _records(oracle.EnvSet(N_INV, seed=SEED_INV))
    rec.setflags(write=False)
    return rec


@pytest.mark.parametrize("flags", range(8))
def test_reference_invariants(kickoffs, flags):
    rec = kickoffs.copy()
    for i in range(N_INV):
        ref.random_state(rec[i], SEED_INV, i, flags)
    # the documented draw count, and nothing but the ball and the cars' SetState fields changed
    assert (rec["env"]["rng_counter"] == ref.draw_count(ref.RANDOM, flags)).all()
    assert ref.draw_count(ref.RANDOM, flags) == 4 + 3 + 7 * (flags & 1) + 4 * (7 + 10 * ((flags >> 1) & 1) + (1 - (flags >> 2)))
    keep = rec.copy()
    for part in ("ball", "ball_vel_impulse_cache"):
        keep[part] = kickoffs[part]
    keep["cars"]["body"] = kickoffs["cars"]["body"]
    keep["cars"]["boost"] = kickoffs["cars"]["boost"]
    keep["env"]["rng_counter"] = kickoffs["env"]["rng_counter"]
    assert not arena_diff(keep, kickoffs)
    # the source's bounds (uu)
    bp = rec["ball"]["pos"].astype(np.float64) * 50
    assert (np.abs(bp[:, 0]) <= 3500.01).all() and (np.abs(bp[:, 1]) <= 4000.01).all()
    assert (bp[:, 2] >= 92.75 - 0.01).all() and (bp[:, 2] <= 1820.01).all()
    assert (rec["ball"]["rot"] == np.eye(3, dtype=np.float32).ravel()).all()
    bv = np.linalg.norm(rec["ball"]["vel"].astype(np.float64) * 50, axis=1)
    if flags & ref.RAND_BALL_SPEED:
        assert (bv <= 4000.01).all() and bv.max() > 2000 and (np.abs(rec["ball"]["angvel"]) <= 4).all()
        assert rec["ball"]["angvel"].any(axis=1).all()
    else:
        assert not rec["ball"]["vel"].any() and not rec["ball"]["angvel"].any()
    body = rec["cars"]["body"]
    cp = body["pos"].astype(np.float64) * 50
    assert (np.abs(cp[..., 0]) <= 3500.01).all() and (np.abs(cp[..., 1]) <= 4000.01).all()
    boost = rec["cars"]["boost"]
    assert (boost >= 0).all() and (boost < 100).all() and boost.std() > 20
    assert (rec["cars"]["is_on_ground"] == 1).all()  # the CarState default, whatever the height
    on_ground = body["pos"][..., 2] == np.float32(17) * ref.UU2BT
    air = ~on_ground
    if flags & ref.CARS_ON_GROUND:
        assert on_ground.all()
    else:
        assert 0.35 < on_ground.mean() < 0.65  # the coin
        assert (cp[..., 2][air] >= 150 - 0.01).all() and (cp[..., 2][air] <= 1820.01).all()
    rot = body["rot"].astype(np.float64).reshape(N_INV, 4, 3, 3)
    # on the ground: yaw only (pitch = roll = 0), no vertical or angular velocity
    g = rot[on_ground]
    assert (g[:, 2, 2] == 1).all() and (g[:, 2, 0] == 0).all() and (g[:, 2, 1] == 0).all()
    assert (g[:, 0, 2] == 0).all() and (g[:, 1, 2] == 0).all()
    assert not body["vel"][..., 2][on_ground].any() and not body["angvel"][on_ground].any()
    # rotation rows orthonormal to 1e-6
    gram = np.einsum("ncij,nckj->ncik", rot, rot)
    assert np.abs(gram - np.eye(3)).max() <= 1e-6
    speed = np.linalg.norm(body["vel"].astype(np.float64) * 50, axis=-1)
    spin = np.linalg.norm(body["angvel"].astype(np.float64), axis=-1)
    if flags & ref.RAND_CAR_SPEED:
        assert (speed <= 2300.01).all() and speed.max() > 1500
        assert np.abs(spin[air] - 5.5).max(initial=0) <= 1e-5
    else:
        assert not body["vel"].any() and not body["angvel"].any()


def test_combined_state_weight_edges(kickoffs):
    kids = lambda a, b: ref.as_children(("combined", [("kickoff", a), (("random", 3), b)]))[1]  # noqa: E731
    for (a, b), want in (((1, 0), 0), ((0, 1), 1)):
        rec = kickoffs.copy()
        picks = [ref.combined_pick(ref.Stream(rec[i], SEED_INV, i), kids(a, b)) for i in range(N_INV)]
        assert picks == [want] * N_INV
        assert (rec["env"]["rng_counter"] == kickoffs["env"]["rng_counter"] + 1).all()  # one draw
    rec = kickoffs.copy()
    picks = np.array([ref.combined_pick(ref.Stream(rec[i], SEED_INV, i), kids(1, 3)) for i in range(N_INV)])
    assert 0.15 < (picks == 0).mean() < 0.35
    assert ref.draw_count(ref.RANDOM, 3, combined=True) == ref.draw_count(ref.RANDOM, 3) + 1


def test_oracle_steps_from_reference_states():
    """The GPU tests' inputs are steppable: 6 steps from RandomState(true, true, false) records."""
    n, seed = 8, 21
    o, _ = ref.created(n, ("random", 3), seed)
    rec = _records(o)
    assert (rec["cars"]["body"]["pos"][..., 2] > 1.0).any() and rec["cars"]["body"]["vel"].any()
    assert (rec["env"]["rng_counter"] == ref.draw_count(ref.RANDOM, 3)).all()
    rng = np.random.default_rng(seed)
    for _ in range(6):
        o.step(random_actions(o.masks, rng), False)
    rec = _records(o)
    for part in (rec["ball"], rec["cars"]["body"]):
        for k in ("pos", "rot", "vel", "angvel"):
            assert np.isfinite(part[k]).all()
    assert np.isfinite(o.obs).all() and np.isfinite(o.rewards).all()
    assert (rec["env"]["tick_count"] == 6 * 8).all()
    assert (rec["env"]["manifold_overflow"] == 0).all()  # no contact dropped by a build limit: parity is exact


def test_config_mirrors_match_the_library():
    from rlgpu import _lib, env, learner
    L = _lib.lib()
    L.rlgpu_learner_config_size.restype = ctypes.c_int32
    assert env.config_size() == ctypes.sizeof(env._Config)
    assert L.rlgpu_learner_config_size() == ctypes.sizeof(learner._CConfig)
    names = [f[0] for f in env._Config._fields_]
    assert names[-4:] == ["state_setter", "state_setter_flags", "state_setters", "n_state_setters"]
    lnames = [f[0] for f in learner._CConfig._fields_]
    i = lnames.index("n_terminals") + 1  # beside the learner config's other env lists
    assert lnames[i:i + 4] == names[-4:]
    assert env.STATE_SETTER_SPEC.itemsize == 12


def test_python_spec_validation():
    from rlgpu.env import (CombinedState, FUZZED_KICKOFF_STATE, KICKOFF_STATE, RandomState, state_setter_spec)
    assert state_setter_spec(KICKOFF_STATE) == (0, 0, None)
    assert state_setter_spec(FUZZED_KICKOFF_STATE) == (1, 0, None)
    assert state_setter_spec(RandomState()) == (2, 7, None)
    assert state_setter_spec(RandomState(True, False, False)) == (2, 1, None)
    assert state_setter_spec(RandomState(rand_ball_speed=False, rand_car_speed=True, cars_on_ground=False)) == (2, 2, None)
    t, f, kids = state_setter_spec(CombinedState([(KICKOFF_STATE, 1), (RandomState(True, True, False), 2),
                                                  (FUZZED_KICKOFF_STATE, 0.5)]))
    assert (t, f) == (3, 0)
    assert kids.tolist() == [(0, 1.0, 0), (2, 2.0, 3), (1, 0.5, 0)]
    with pytest.raises(ValueError, match=r"setter 1 .*weight of -1"):
        CombinedState([(KICKOFF_STATE, 1), (RandomState(), -1.0)])
    with pytest.raises(ValueError, match=r"setter 0 .*weight of nan"):
        CombinedState([(KICKOFF_STATE, float("nan"))])
    with pytest.raises(ValueError, match=r"setter 1 .*weight of inf"):
        CombinedState([(KICKOFF_STATE, 1), (FUZZED_KICKOFF_STATE, float("inf"))])
    with pytest.raises(ValueError, match="list is empty"):
        CombinedState([])
    with pytest.raises(ValueError, match=r"setter 1 is a CombinedState: a nested"):
        CombinedState([(KICKOFF_STATE, 1), (CombinedState([(KICKOFF_STATE, 1)]), 1)])
    with pytest.raises(ValueError, match=r"9 setters, at most 8"):
        CombinedState([(KICKOFF_STATE, 1)] * 9)
    with pytest.raises(ValueError, match=r"setter 2: 5 is no state setter"):
        CombinedState([(KICKOFF_STATE, 1), (KICKOFF_STATE, 1), (5, 1)])
    with pytest.raises(ValueError, match=r"state_setter: 7 is no state setter"):
        state_setter_spec(7)
    from rlgpu.learner import LearnerConfig
    assert LearnerConfig().state_setter == KICKOFF_STATE
    assert isinstance(LearnerConfig(state_setter=RandomState()).state_setter, RandomState)


def test_facade_translation():
    if not os.path.exists(PLAN_BIN):
        pytest.fail(f"{PLAN_BIN} is not built (make -C reinforcement-learning_amd)")
    r = subprocess.run([PLAN_BIN], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    out = r.stdout.splitlines()
    assert "kickoff: setter 0 flags 0 children 0" in out and "fuzzed: setter 1 flags 0 children 0" in out
    for f in range(8):
        assert f"random{f}: setter 2 flags {f} children 0" in out
    i = out.index("combined3: setter 3 flags 0 children 3")
    assert out[i + 1:i + 4] == ["  child 0: type 0 weight 1 flags 0", "  child 1: type 2 weight 2 flags 3",
                                "  child 2: type 1 weight 0.5 flags 0"]
    line = {ln.split(":")[0]: ln for ln in out if not ln.startswith(" ")}
    assert "refused" in line["nested"] and "setter 1 is a CombinedState" in line["nested"]
    assert "refused" in line["user"] and "UserSetter" in line["user"]
    assert "refused" in line["combined_user"] and "setter 1" in line["combined_user"] and "UserSetter" in line["combined_user"]
    assert "refused" in line["combined9"] and "RLGPU_MAX_STATE_SETTERS" in line["combined9"]
    assert "refused" in line["bad_weight"] and "weight of -1" in line["bad_weight"]
    assert "refused" in line["empty"]
    assert line["same"] == "same: equal 1 weights 0 flags 0 count 0 random_flags 0 kickoff_vs_random 0"
    assert "mismatch" not in r.stdout


def test_create_rejects_bad_setter_configs():
    """rlgpu_envset_create validates the setter before any device work, so the refusals show without a GPU: each
    names the entry at fault."""
    from rlgpu import _lib, env
    L = env._bind()

    def refused(setter, flags=0, kids=None, n=None):
        cfg = env._Config(8, 8, 7, 1)
        cfg.state_setter, cfg.state_setter_flags = setter, flags
        arr = None
        if kids is not None:
            arr = np.array(kids, env.STATE_SETTER_SPEC)
            cfg.state_setters = arr.ctypes.data
            cfg.n_state_setters = len(kids) if n is None else n
        elif n is not None:
            cfg.n_state_setters = n
        h = ctypes.c_void_p()
        st = L.rlgpu_envset_create(ctypes.byref(cfg), ctypes.byref(h))
        assert st != 0 and not h.value
        return _lib.last_error()

    assert "unknown state setter 5" in refused(5)
    assert "state_setter_flags 8" in refused(2, flags=8)
    assert "1..8 entries, got none" in refused(3)
    assert "1..8 entries, got 0" in refused(3, kids=[(0, 1, 0)], n=0)
    assert "1..8 entries, got 9" in refused(3, kids=[(0, 1, 0)] * 9)
    assert "state setter 1 has a negative or invalid weight of -1" in refused(3, kids=[(0, 1, 0), (2, -1, 0)])
    assert "state setter 0 has a negative or invalid weight of nan" in refused(3, kids=[(1, np.nan, 0)])
    assert "state setter 2 has a negative or invalid weight of inf" in refused(3, kids=[(0, 1, 0), (0, 1, 0), (2, np.inf, 7)])
    assert "state setter 1 is RLGPU_SS_COMBINED" in refused(3, kids=[(0, 1, 0), (3, 1, 0)])
    assert "state setter 1 has unknown type 4" in refused(3, kids=[(0, 1, 0), (4, 1, 0)])
    assert "state setter 0 has flags 9" in refused(3, kids=[(2, 1, 9)])

"""InferUnit without a GPU: the numpy reference of its rows (tests/infer_unit_reference.py) against the CPU oracle
env, the struct mirrors' sizes, and the argument checks of the C ABI, which come before any device work."""
import ctypes

import numpy as np
import pytest

import infer_unit_reference as ref
from tests_util import random_actions

ARENAS, STEPS, SEED = 6, 40, 17


def _same_bits(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.dtype == np.float32:
        g, w = g.view(np.uint32), w.view(np.uint32)
    bad = np.argwhere(g != w)
    assert not len(bad), f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}"


@pytest.fixture(scope="module")
def states():
    """GameState records of 6 oracle arenas after 40 steps of seeded random actions, and the oracle's rows of them.
    Every step's rows are compared on the way: the oracle's step rebuilds the rows of the arenas it resets in the same
    call, and the records are read after that call, so the records and every row are of the same moment."""
    import oracle
    from rlgpu.env import gamestates_from_arenas
    o = oracle.EnvSet(ARENAS, seed=SEED)
    rng = np.random.default_rng(SEED)
    jump_off = False
    for t in range(STEPS):
        o.step(random_actions(o.masks, rng), True)
        gs = gamestates_from_arenas(o.get_arenas())
        _same_bits(ref.build_rows(gs), o.obs, ("obs", t))
        _same_bits(ref.mask_rows(gs), o.masks, ("masks", t))
        jump_off = jump_off or bool((o.masks[:, ref._TABLE[3] != 0] == 0).all(axis=1).any())
    assert jump_off, "no row ever had the jump actions off: the masks prove little"
    assert len({m.tobytes() for m in o.masks}) > 1
    return gs, o.obs.copy(), o.masks.copy()


def test_reference_rows_equal_the_oracle(states):
    gs, obs, masks = states
    assert obs.shape == (4 * ARENAS, ref.WIDTH) and ref.WIDTH == 167
    _same_bits(ref.build_rows(gs), obs, "obs")
    _same_bits(ref.mask_rows(gs), masks, "masks")
    # a subset in another order is the same rows
    rows = [(5, 2), (0, 0), (3, 3)]
    _same_bits(ref.build_rows(gs, rows), obs[[22, 0, 15]], "subset")


def test_reference_action_table_equals_the_oracle():
    import oracle
    t, m = oracle.action_table()
    mine = ref.action_table()
    _same_bits(mine[0], t, "table")
    for k in range(4):  # ground, air, jump, boost
        _same_bits(mine[1 + k], m[k], ("mask table", k))


def test_reference_order_follows_team_and_car_id(states):
    """Players permuted to blue, blue, orange, orange: each player's row is what it was."""
    gs, obs, _ = states
    perm = [0, 2, 1, 3]
    g = gs.copy()
    g["players"] = gs["players"][:, perm]
    g["players"]["index"] = np.arange(4)
    rows = [(a, perm.index(p)) for a in range(len(gs)) for p in range(4)]
    _same_bits(ref.build_rows(g, rows), obs, "permuted")


def test_struct_mirrors_have_the_c_sizes():
    from rlgpu import _lib, infer_unit
    from rlgpu.env import gamestate_size
    from rlgpu.state import GAMESTATE
    assert infer_unit.config_size() == ctypes.sizeof(infer_unit._Cfg) == 40
    assert gamestate_size() == GAMESTATE.itemsize
    infer_unit._bind()
    assert _lib.lib().rlgpu_infer_unit_obs_size(None) == -1 and _lib.lib().rlgpu_infer_unit_one_launch(None) == 0


def test_row_checks_fail_by_name(states):
    from rlgpu import _lib
    from rlgpu.infer_unit import check_rows
    gs = states[0]
    check_rows(gs)
    check_rows(gs, [(5, 3), (0, 0)])
    bad = gs.copy()
    bad["players"]["team"][2, 1] = 0  # three blue, one orange
    with pytest.raises(_lib.RLGPUError, match=r"state 2 has 3 blue and 1 orange players: two per team"):
        check_rows(bad)
    bad = gs.copy()
    bad["players"]["car_id"][4, 3] = bad["players"]["car_id"][4, 0]
    with pytest.raises(_lib.RLGPUError, match=r"state 4: players 0 and 3 share car_id 1 \(duplicate car_id\)"):
        check_rows(bad)
    bad = gs.copy()
    bad["players"]["team"][1, 0] = 2
    with pytest.raises(_lib.RLGPUError, match=r"state 1: player 0 has team 2"):
        check_rows(bad)
    with pytest.raises(_lib.RLGPUError, match=r"player_of_row\[1\] = 4 is outside 0\.\.3"):
        check_rows(gs, [(0, 0), (0, 4)])
    with pytest.raises(_lib.RLGPUError, match=r"player_of_row\[0\] = -1 is outside 0\.\.3"):
        check_rows(gs, [(0, -1)])
    with pytest.raises(_lib.RLGPUError, match=r"state_of_row\[0\] = 6 is outside the 6 states"):
        check_rows(gs, [(6, 0)])
    with pytest.raises(_lib.RLGPUError, match=r"n must be > 0, got 0"):
        check_rows(gs, np.zeros((0, 2), np.int64))


@pytest.mark.parametrize("temperature", (0.0, -1.0, float("nan"), float("inf")))
def test_temperature_is_checked_before_anything_else(states, temperature):
    """rlgpu_infer_unit_infer refuses the temperature by name before it looks at the unit (none here)."""
    from rlgpu import _lib, infer_unit
    L = infer_unit._bind()
    gs, sor, por = infer_unit._rows(states[0], None)
    idx, act = np.zeros(24, np.int32), np.zeros((24, 8), np.float32)
    rc = L.rlgpu_infer_unit_infer(None, gs.ctypes.data, len(gs), sor.ctypes.data, por.ctypes.data, 24, 0, 0, temperature, 0,
                                  idx.ctypes.data, None, act.ctypes.data, None)
    assert rc == -1 and "temperature must be finite and > 0" in _lib.last_error()
    rc = L.rlgpu_infer_unit_infer(None, gs.ctypes.data, len(gs), sor.ctypes.data, por.ctypes.data, 24, 0, 0, 1.0, 0,
                                  idx.ctypes.data, None, act.ctypes.data, None)
    assert rc == -1 and "null argument" in _lib.last_error()


def test_python_unit_checks_its_arguments_first():
    from rlgpu.env import DefaultObsPadded
    from rlgpu.infer_unit import InferUnit
    with pytest.raises(ValueError, match="no obs builder"):
        InferUnit(obs_builder="advanced", models_folder="nowhere")
    with pytest.raises(ValueError, match="give a PPO"):
        InferUnit(obs_builder=DefaultObsPadded(3))

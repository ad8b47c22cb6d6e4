"""InferUnit on the device, bit for bit against code that exists without it: the rows of iu::gs_rows against the env
set's own rows of the same moment and against the numpy restatements of the reference's builders, the actions and log
probs of rlgpu_infer_unit_infer (one launch, iu::gs_infer_wave, or rows + the handle's own inference path) against
the PPO handle's inference on the env set's rows.

The states: an EnvSet of 6 arenas (24 rows: one full 16-row workgroup and a ragged one of 8) under
RandomState(True, True, False) -- cars in the air, without boost, at every attitude -- after 40 steps of seeded random
actions and a build_obs, so that the env's rows and the GameState records are of the same moment.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import default_obs_reference as dref
import infer_unit_reference as ref
from tests_util import random_actions

pytestmark = pytest.mark.gpu

ARENAS, STEPS, SEED = 6, 40, 23
P = 4 * ARENAS
ROWS = (1, 16, 17, 24)
BUILDERS = ("advanced", "default", "padded3")
MODELS = {
    "c2": dict(policy_layers=(512, 512), critic_layers=(8,)),                           # tests/test_infer_wave.py's
    "small_no_ln": dict(policy_layers=(64,), critic_layers=(8,), layer_norm=False),
    "shared_head": dict(policy_layers=(96,), critic_layers=(8,), shared_layers=(128, 64)),
    "fp16": dict(policy_layers=(96, 40), critic_layers=(8,), infer_fp16=True),
}


def _builder(name):
    from rlgpu.env import ADVANCED_OBS, DefaultObs, DefaultObsPadded
    return {"advanced": ADVANCED_OBS, "default": DefaultObs(), "padded3": DefaultObsPadded(3)}[name]


def _np(t):
    return t.detach().cpu().contiguous().numpy().copy()


def _same_bits(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.dtype == np.float32:
        g, w = g.view(np.uint32), w.view(np.uint32)
    bad = np.argwhere(g != w)
    assert not len(bad), f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}"


_RUNS = {}


def _run(gpu, name):
    """One builder's env run, made once: (GameState records, env obs, env masks) of the same moment.  Every builder's
    run takes the AdvancedObs run's actions: the builder does not touch the physics."""
    if name in _RUNS:
        return _RUNS[name]
    import torch
    from rlgpu.env import EnvSet, RandomState
    g = EnvSet(ARENAS, seed=SEED, device=gpu, state_setter=RandomState(True, True, False), obs_builder=_builder(name))
    rng = np.random.default_rng(SEED)
    for _ in range(STEPS):
        g.step(torch.from_numpy(random_actions(_np(g.action_masks), rng)).to(gpu), True)
    g.build_obs()
    torch.cuda.synchronize()
    _RUNS[name] = (g.gamestates(), _np(g.obs), _np(g.action_masks))
    g.close()
    return _RUNS[name]


def _policy(gpu, model="small_no_ln", obs_size=167, **kw):
    from rlgpu.ppo import PPO
    return PPO(obs_size=obs_size, max_rows=64, seed=5, device=gpu, **{**MODELS[model], **kw})


def _unit(gpu, name, ppo, obs_seed=SEED, one_launch=True):
    """A unit that asks for the one-launch kernel (it runs where the policy is eligible), unless told otherwise."""
    from rlgpu.infer_unit import InferUnit
    return InferUnit(obs_builder=_builder(name), ppo=ppo, obs_seed=obs_seed, one_launch=one_launch)


# ---- 1. rows equal the env's
@pytest.mark.parametrize("name", BUILDERS)
def test_rows_equal_the_env_sets(gpu, name):
    gs, obs, masks = _run(gpu, name)
    jump = ref._TABLE[3] != 0
    assert len({m.tobytes() for m in masks}) > 2, "the masks are all alike: the inputs prove nothing"
    assert (masks[:, jump] == 0).all(axis=1).any(), "no row has the jump actions off"
    assert not gs["players"]["car"]["is_on_ground"].all() and (gs["players"]["car"]["boost"] == 0).any()
    ppo = _policy(gpu, obs_size=obs.shape[1])
    u = _unit(gpu, name, ppo)
    assert u.obs_size == obs.shape[1] == {"advanced": 167, "default": 127, "padded3": 165}[name]
    o, m = u.build_rows(gs)
    _same_bits(_np(o), obs, (name, "obs"))
    _same_bits(_np(m), masks, (name, "masks"))
    if name == "padded3":  # the shuffle key is the seed's: another seed gives other rows; row0 moves the stream
        v = _unit(gpu, name, ppo, obs_seed=SEED + 1)
        assert not np.array_equal(_np(v.build_rows(gs)[0]), obs)
        v.close()
        o8, _ = u.build_rows(gs[2:], row0=8)
        _same_bits(_np(o8), obs[8:], (name, "arenas 2.. at row0 8"))
    u.close()
    ppo.close()


# ---- 2. any player order
def _permuted(gs, perm):
    g = gs.copy()
    g["players"] = gs["players"][:, perm]
    g["players"]["index"] = np.arange(4)
    return g


@pytest.mark.parametrize("perm", ([0, 2, 1, 3], [3, 2, 1, 0]), ids=("blue_blue_orange_orange", "reversed"))
@pytest.mark.parametrize("name", ("advanced", "default"))
def test_any_player_order(gpu, name, perm):
    gs, obs, masks = _run(gpu, name)
    g2 = _permuted(gs, perm)
    assert (g2["players"]["car_id"] == gs["players"]["car_id"][:, perm]).all()
    if name == "advanced":
        want = ref.build_rows(g2)
    else:
        want, _ = dref.build_rows(g2, dref.spec(dref.DEFAULT))
    want_masks = ref.mask_rows(g2)
    ppo = _policy(gpu, obs_size=obs.shape[1])
    u = _unit(gpu, name, ppo)
    o, m = u.build_rows(g2)
    _same_bits(_np(o), want, (name, perm, "obs"))
    _same_bits(_np(m), want_masks, (name, perm, "masks"))
    # blue, blue, orange, orange keeps every list's order, so each player's row is the env's; the reverse swaps the
    # opponents of every row
    back = [4 * a + perm[p] for a in range(ARENAS) for p in range(4)]
    assert np.array_equal(_np(o), obs[back]) == (perm == [0, 2, 1, 3])
    order = np.random.default_rng(3).permutation(P)
    for n in (1, 16, 17):
        rows = [(int(r) // 4, int(r) % 4) for r in order[:n]]
        o, m = u.build_rows(g2, rows)
        _same_bits(_np(o), want[order[:n]], (name, perm, n, "subset obs"))
        _same_bits(_np(m), want_masks[order[:n]], (name, perm, n, "subset masks"))
    u.close()
    ppo.close()


# ---- 3. actions equal the policy path's
def _check_infer(gpu, u, ref_ppo, temp, n, det, rows_api=True, row0=37):
    """unit.infer on the first n rows against ref_ppo (policy_temperature = temp) on the env's rows."""
    import torch
    gs, obs, masks = _run(gpu, "advanced")
    rows = [(r // 4, r % 4) for r in range(n)]
    o, m = torch.from_numpy(obs[:n]).to(gpu), torch.from_numpy(masks[:n]).to(gpu)
    if rows_api:
        wa, wl = ref_ppo.infer_actions_rows(o, m, row0=row0, step=11, deterministic=det)
    else:
        assert row0 == 0
        wa, wl = ref_ppo.infer_actions(o, m, step=11, deterministic=det)
    act, idx, lp = u.infer(gs, rows, deterministic=det, temperature=temp, step=11, row0=row0)
    what = (temp, n, det)
    _same_bits(idx, _np(wa), (what, "index"))
    _same_bits(lp, _np(wl), (what, "logp"))
    return act, idx, lp


def _check_parsed(act, idx, masks):
    import oracle
    table, _ = oracle.action_table()
    _same_bits(act, table[idx], "parsed actions")
    assert (masks[np.arange(len(idx)), idx] == 1).all(), "a masked action"


@pytest.mark.parametrize("model", sorted(MODELS))
def test_actions_equal_the_policy_path(gpu, model):
    _, _, masks = _run(gpu, "advanced")
    ppos = {1.0: _policy(gpu, model), 0.7: _policy(gpu, model, policy_temperature=0.7)}
    u = _unit(gpu, "advanced", ppos[1.0])  # the unit's handle has temperature 1: 0.7 is the call's
    assert u.one_launch
    for temp, p in ppos.items():
        for n in ROWS:
            for det in (False, True):
                act, idx, lp = _check_infer(gpu, u, p, temp, n, det)
                _check_parsed(act, idx, masks[:n])
    # the default unit does not ask for the one-launch kernel: rows, the handle's fused kernel, parse -- the same bits
    d = _unit(gpu, "advanced", ppos[1.0], one_launch=False)
    assert not d.one_launch
    gs = _run(gpu, "advanced")[0]
    for a, b in zip(d.infer(gs, temperature=0.7, step=11, row0=37), u.infer(gs, temperature=0.7, step=11, row0=37)):
        _same_bits(a, b, "default path against one launch")
    _check_infer(gpu, d, ppos[0.7], 0.7, 17, False)
    d.close()
    # another row0 changes the draws
    _, idx37, _ = _check_infer(gpu, u, ppos[1.0], 1.0, 24, False)
    _, idx38, _ = _check_infer(gpu, u, ppos[1.0], 1.0, 24, False, row0=38)
    assert not np.array_equal(idx37, idx38)
    # the unit's own call counter is the step
    gs = _run(gpu, "advanced")[0]
    a0 = u.infer(gs)
    a1 = u.infer(gs)
    assert not np.array_equal(a0[1], a1[1])
    _same_bits(u.infer(gs, step=0)[1], a0[1], "step 0")
    _same_bits(u.infer_action(gs[3], 2, deterministic=True), u.infer(gs, deterministic=True)[0][14], "InferAction")
    u.close()
    for p in ppos.values():
        p.close()


# ---- 4. the two-step path
@pytest.mark.parametrize("case", ("tanh", "wide"))
def test_two_step_path(gpu, case):
    from rlgpu.ppo import PPO
    _, _, masks = _run(gpu, "advanced")
    if case == "tanh":  # on the fused 8-wave kernel: infer_actions_rows takes it
        kw = dict(policy_layers=(64, 32), critic_layers=(8,), activation="tanh", max_rows=64)
    else:  # [1024] is off the fused kernel: the layered path, in chunks of max_rows = 16 rows
        kw = dict(policy_layers=(1024,), critic_layers=(8,), max_rows=16)
    ppos = {t: PPO(seed=5, device=gpu, policy_temperature=t, **kw) for t in (1.0, 0.7)}
    u = _unit(gpu, "advanced", ppos[1.0])
    assert not u.one_launch
    for temp, p in ppos.items():
        for n in ROWS:
            for det in (False, True):
                if case == "tanh":
                    act, idx, lp = _check_infer(gpu, u, p, temp, n, det)
                else:  # rlgpu_ppo_infer_actions_rows refuses a handle off the fused kernel: the rows from 0
                    act, idx, lp = _check_infer(gpu, u, p, temp, n, det, rows_api=False, row0=0)
                _check_parsed(act, idx, masks[:n])
    u.close()
    for p in ppos.values():
        p.close()


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = [{tests!r}, {root!r}, {pkg!r}]
from rlgpu.env import ADVANCED_OBS
from rlgpu.infer_unit import InferUnit
from rlgpu.ppo import PPO
from rlgpu.state import GAMESTATE
gs = np.fromfile({states!r}, GAMESTATE)
p = PPO(max_rows=64, seed=5, policy_layers=(512, 512), critic_layers=(8,))
u = InferUnit(obs_builder=ADVANCED_OBS, ppo=p, one_launch=True)
out = dict(one_launch=np.array(u.one_launch))
for det in (0, 1):
    act, idx, lp = u.infer(gs, deterministic=bool(det), temperature=0.7, step=11, row0=0)
    o, m = u.build_rows(gs)
    wa, wl = PPO(max_rows=64, seed=5, policy_layers=(512, 512), critic_layers=(8,), policy_temperature=0.7).infer_actions(
        o, m, step=11, deterministic=bool(det))
    out.update({{f"act{{det}}": act, f"idx{{det}}": idx, f"lp{{det}}": lp, f"wa{{det}}": wa.cpu().numpy(), f"wl{{det}}": wl.cpu().numpy()}})
np.savez({result!r}, **out)
"""


def test_forced_two_step_equals_one_launch(gpu, tmp_path):
    """RLGPU_FUSED_INFER=0 in a fresh process: the c2 policy leaves the one-launch kernel, and the rows + layered
    path give the bits of the one-launch kernel here."""
    from conftest import PKG, ROOT
    gs, _, _ = _run(gpu, "advanced")
    states, result = str(tmp_path / "states.bin"), str(tmp_path / "child.npz")
    gs.tofile(states)
    code = _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)), root=ROOT, pkg=PKG, states=states, result=result)
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "RLGPU_FUSED_INFER": "0"}, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    c = np.load(result)
    assert not bool(c["one_launch"])
    p = _policy(gpu, "c2")
    u = _unit(gpu, "advanced", p)
    assert u.one_launch
    for det in (0, 1):
        _same_bits(c[f"idx{det}"], c[f"wa{det}"], (det, "forced: index against infer_actions"))
        _same_bits(c[f"lp{det}"], c[f"wl{det}"], (det, "forced: logp against infer_actions"))
        act, idx, lp = u.infer(gs, deterministic=bool(det), temperature=0.7, step=11, row0=0)
        _same_bits(c[f"idx{det}"], idx, (det, "forced against one launch: index"))
        _same_bits(c[f"lp{det}"], lp, (det, "forced against one launch: logp"))
        _same_bits(c[f"act{det}"], act, (det, "forced against one launch: actions"))
    u.close()
    p.close()


def test_fp32_inference_handle(gpu):
    """An fp32-inference handle: the sampler's result on forward(precision 0) logits, as
    tests/test_sampler.py::test_fp32_inference_bit_exact_vs_oracle has it."""
    import oracle
    import torch
    from rlgpu.ppo import PPO
    gs, obs, masks = _run(gpu, "advanced")
    p = PPO(max_rows=64, seed=41, infer_fp16=2, policy_layers=(64, 64), critic_layers=(8,), device=gpu)
    u = _unit(gpu, "advanced", p)
    assert not u.one_launch
    logits = p.forward(0, torch.from_numpy(obs).to(gpu)).cpu().numpy()
    for det in (True, False):
        for row0 in (0, 37):
            act, idx, lp = u.infer(gs, deterministic=det, step=3, row0=row0)
            wa, wlp = oracle.sample_actions(logits, masks, det, p.cfg.seed, 3, row0)
            _same_bits(idx, wa, (det, row0, "index"))
            _same_bits(lp, wlp, (det, row0, "logp"))
            _check_parsed(act, idx, masks)
    u.close()
    p.close()


# ---- 5. allocations
def test_device_allocations_return_to_the_baseline(gpu):
    import ctypes
    from rlgpu import _lib
    from rlgpu.env import DefaultObs
    from rlgpu.infer_unit import InferUnit
    L = _lib.lib()
    L.rlgpu_live_device_allocations.restype = ctypes.c_int64
    gs, _, _ = _run(gpu, "advanced")
    for model, kw in (("c2", {}), ("small_no_ln", dict(activation="sigmoid"))):  # one launch, two steps
        p = _policy(gpu, model, **kw)
        base = L.rlgpu_live_device_allocations()
        u = _unit(gpu, "advanced", p)
        assert u.one_launch == (model == "c2")
        assert L.rlgpu_live_device_allocations() > base
        u.infer(gs, [(0, 0)])
        small = L.rlgpu_live_device_allocations()
        u.infer(gs)          # 24 rows of 6 states: the staging blocks grow in place
        u.infer(np.tile(gs, 4))
        assert L.rlgpu_live_device_allocations() == small
        u.close()
        assert L.rlgpu_live_device_allocations() == base
        # refused creates leave nothing behind
        with pytest.raises(_lib.RLGPUError, match="makes rows of 127 floats and the policy handle's obs_size is 167"):
            InferUnit(obs_builder=DefaultObs(), ppo=p)
        assert L.rlgpu_live_device_allocations() == base
        p.close()
    from rlgpu.ppo import PPO
    p = PPO(num_actions=50, max_rows=64, policy_layers=(32,), critic_layers=(8,), device=gpu)
    base = L.rlgpu_live_device_allocations()
    with pytest.raises(_lib.RLGPUError, match="num_actions is 50 and DefaultAction has 90"):
        InferUnit(ppo=p)
    assert L.rlgpu_live_device_allocations() == base
    p.close()


def test_models_folder_constructor(gpu, tmp_path):
    """The folder constructor loads POLICY.lt (+ SHARED_HEAD.lt) with the guiding policy's loader; a missing file and a
    checkpoint trained with standardizeObs are refused by name."""
    import json
    from rlgpu import _lib, checkpoint
    from rlgpu.infer_unit import InferUnit
    gs, _, _ = _run(gpu, "advanced")
    p = _policy(gpu, "shared_head")
    for mi in (0, 2):
        checkpoint.write_model(p.torch_module(mi), checkpoint.model_path(str(tmp_path), checkpoint.MODEL_NAMES[mi]))
    kw = dict(policy_layers=(96,), shared_layers=(128, 64), seed=5)
    u, w = InferUnit(models_folder=str(tmp_path), **kw), _unit(gpu, "advanced", p)
    for det in (True, False):
        for a, b in zip(u.infer(gs, deterministic=det, step=4), w.infer(gs, deterministic=det, step=4)):
            _same_bits(a, b, det)
    u.close()
    w.close()
    p.close()
    os.remove(checkpoint.model_path(str(tmp_path), "shared_head"))
    with pytest.raises(FileNotFoundError, match="SHARED_HEAD.lt does not exist"):
        InferUnit(models_folder=str(tmp_path), **kw)
    with open(tmp_path / "RUNNING_STATS.json", "w") as f:
        json.dump({"obs_stat": {"means": [], "vars": [], "count": 0}}, f)
    with pytest.raises(_lib.RLGPUError, match="standardizeObs"):
        InferUnit(models_folder=str(tmp_path), **kw)


# ---- 6. the C++ facade
def _facade(*args):
    from conftest import PKG
    exe = os.path.join(PKG, "rlgpu", "rlgpu_infer_unit_test")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_facade_infer_unit(gpu, tmp_path):
    """GGL::InferUnit (facade/InferUnit.hpp through <GigaLearnCPP/Util/InferUnit.h>) in a process of its own: it loads
    the checkpoint folder saved here, converts RLGC::GameStates to records and back, finds the players by carId, and its
    deterministic actions are the Python unit's (deterministic mode does not depend on the call counter)."""
    from rlgpu import checkpoint
    gs, _, _ = _run(gpu, "advanced")
    p = _policy(gpu, "shared_head")
    for mi in (0, 2):
        checkpoint.write_model(p.torch_module(mi), checkpoint.model_path(str(tmp_path), checkpoint.MODEL_NAMES[mi]))
    states = str(tmp_path / "states.bin")
    gs.tofile(states)
    out = _facade("run", str(tmp_path), states, "96", "128,64").splitlines()
    u = _unit(gpu, "advanced", p, one_launch=False)  # the default, as the facade's unit
    want, _, _ = u.infer(gs, deterministic=True)
    assert out[0] == f"one launch: {int(u.one_launch)}" == "one launch: 0"
    parse = lambda line: np.array(line.split(":")[1].split(), np.float32)  # noqa: E731
    _same_bits(parse(out[1]), want[14], "InferAction(player 2 of state 3)")
    rows = [ln for ln in out if ln.startswith("row ")]
    assert len(rows) == P
    _same_bits(np.stack([parse(ln) for ln in rows]), want, "BatchInferActions")
    assert len({tuple(r) for r in want.tolist()}) > 2  # the policy does not answer every row alike
    assert "absent player: InferUnit: player 0 (carId 77) is not in its GameState" in out
    u.close()
    p.close()
    # refusals, by name
    empty = tmp_path / "empty"
    empty.mkdir()
    msgs = _facade("refuse", str(empty))
    assert "custom obs builder: InferUnit: obs builder" in msgs and "has no device code" in msgs
    assert "useGPU false: InferUnit: useGPU = false" in msgs
    assert "wrong obsSize: InferUnit: obsSize 167 is not the obs builder's width 127" in msgs
    assert f"missing model: InferUnit: {empty}/POLICY.lt does not exist" in msgs
    assert "accepted" not in msgs

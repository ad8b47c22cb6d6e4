"""GGL::InferUnit (GigaLearnCPP/Util/InferUnit.{h,cpp}) over the C ABI of include/rlgpu_infer_unit.h: actions of a
trained policy for (player, GameState) pairs that live in no env set.

    unit = InferUnit(obs_builder=ADVANCED_OBS, policy_layers=(512, 512), models_folder="checkpoints/123456")
    actions, index, logp = unit.infer(states)            # every player of every state, in order

states is a numpy array of rlgpu.state.GAMESTATE records (EnvSet.gamestates(), gamestates_from_arenas, or records
filled from a game).  A row's players are ordered as the reference orders them: self, the teammates in
state.players order, the opponents in state.players order; sides come from `team`, self is found by `car_id`.

Deviation from the reference: it samples from libtorch's global generator; here the draw of a row is a function of
(the policy's seed, row0 + i, step), so two units with the same seed and the same calls give the same actions.
"""
import ctypes
import json
import math
import os

import numpy as np

from . import _lib
from .env import obs_builder_spec
from .state import GAMESTATE


class _Cfg(ctypes.Structure):
    _fields_ = [("obs_builder", ctypes.c_int32), ("obs_max_players", ctypes.c_int32),
                ("obs_pos_coef", ctypes.c_float * 3), ("obs_vel_coef", ctypes.c_float),
                ("obs_ang_vel_coef", ctypes.c_float), ("obs_seed", ctypes.c_uint64)]


_bound = False


def _bind():
    global _bound
    L = _lib.lib()
    if _bound:
        return L
    if L.rlgpu_infer_unit_config_size() != ctypes.sizeof(_Cfg):
        raise _lib.RLGPUError(f"rlgpu_infer_unit_config is {L.rlgpu_infer_unit_config_size()} bytes in the library, "
                              f"{ctypes.sizeof(_Cfg)} in rlgpu/infer_unit.py: the binding is out of date")
    vp, i32, i64, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float
    L.rlgpu_infer_unit_create.argtypes = [ctypes.POINTER(_Cfg), vp, ctypes.POINTER(vp)]
    L.rlgpu_infer_unit_destroy.argtypes = [vp]
    L.rlgpu_infer_unit_obs_size.argtypes = [vp]
    L.rlgpu_infer_unit_one_launch.argtypes = [vp]
    L.rlgpu_infer_unit_set_one_launch.argtypes = [vp, i32]
    L.rlgpu_infer_unit_check_rows.argtypes = [vp, i32, vp, vp, i32]
    L.rlgpu_infer_unit_build_rows.argtypes = [vp, vp, i32, vp, vp, i32, i64, vp, vp, vp]
    L.rlgpu_infer_unit_infer.argtypes = [vp, vp, i32, vp, vp, i32, i64, i32, f32, u64, vp, vp, vp, vp]
    _bound = True
    return L


def config_size():
    """sizeof(rlgpu_infer_unit_config) in the library, for checking the _Cfg mirror."""
    return _lib.lib().rlgpu_infer_unit_config_size()


def _rows(states, rows):
    """(states, state_of_row, player_of_row) as contiguous arrays; rows None: every player of every state."""
    states = np.ascontiguousarray(states, GAMESTATE).reshape(-1)
    if rows is None:
        sor = np.repeat(np.arange(len(states), dtype=np.int32), 4)
        por = np.tile(np.arange(4, dtype=np.int32), len(states))
    else:
        r = np.asarray(rows, np.int64).reshape(-1, 2)
        sor, por = np.ascontiguousarray(r[:, 0], np.int32), np.ascontiguousarray(r[:, 1], np.int32)
    return states, sor, por


def check_rows(states, rows=None):
    """The argument checks of infer / build_rows alone (rlgpu_infer_unit_check_rows; no GPU): raises RLGPUError naming
    a state that is not two players per team, a duplicate car_id, an index out of range, or an empty call."""
    L = _bind()
    states, sor, por = _rows(states, rows)
    _lib.check(L.rlgpu_infer_unit_check_rows(states.ctypes.data, len(states), sor.ctypes.data, por.ctypes.data, len(sor)),
               "rlgpu_infer_unit_check_rows")


def _standardized(folder):
    """Whether the checkpoint's RUNNING_STATS.json holds an obs statistic (LearnerConfig::standardizeObs)."""
    p = os.path.join(folder, "RUNNING_STATS.json")
    if not os.path.exists(p):
        return False
    with open(p) as f:
        return "obs_stat" in json.load(f)


class InferUnit:
    """obs builder + DefaultAction + shared head -> policy on GameState records."""

    def __init__(self, obs_builder=None, policy_layers=(512, 512), shared_layers=(), models_folder=None, ppo=None,
                 activation="leaky_relu", layer_norm=True, infer_fp16=False, seed=42, obs_seed=0, leaky_slope=0.01,
                 max_rows=4096, device="cuda:0", one_launch=False):
        """Either wraps `ppo` (a PPO whose obs_size is the builder's width; the caller keeps it alive) or builds one
        from the layer lists and loads <models_folder>/POLICY.lt (+ SHARED_HEAD.lt); a missing file is an error.
        obs_builder: ADVANCED_OBS (None), a DefaultObs or a DefaultObsPadded (rlgpu.env); obs_seed keys
        DefaultObsPadded's shuffles (an env set's seed reproduces that set's rows).  seed: the sampler's.  one_launch:
        ask for the one-launch kernel (see the one_launch property; off by default, it measured slower)."""
        from .ppo import PPO
        L = _bind()
        self.obs_builder = b = obs_builder_spec(obs_builder)
        self._owns_ppo = ppo is None
        if ppo is None:
            if models_folder is None:
                raise ValueError("InferUnit: give a PPO (ppo=) or a folder with POLICY.lt (models_folder=)")
            if _standardized(models_folder):
                raise _lib.RLGPUError(f"InferUnit: {models_folder} was trained with standardizeObs (its RUNNING_STATS.json "
                                      "holds an obs_stat), and the unit does not standardise observations")
            from .learner import load_teacher
            ppo = PPO(obs_size=b.obs_size, num_actions=90, policy_layers=policy_layers, critic_layers=(8,),
                      shared_layers=shared_layers, layer_norm=layer_norm, activation=activation, infer_fp16=infer_fp16,
                      seed=seed, leaky_slope=leaky_slope, max_rows=max_rows, init=False, device=device)
            try:
                load_teacher(ppo, models_folder)
            except Exception:
                ppo.close()
                raise
        self.ppo = ppo
        self.device = ppo.device
        c = _Cfg()
        c.obs_builder, c.obs_max_players, c.obs_seed = b.kind, b.max_players, int(obs_seed)
        if b.kind:
            c.obs_pos_coef = (ctypes.c_float * 3)(*b.pos_coef)
            c.obs_vel_coef, c.obs_ang_vel_coef = b.vel_coef, b.ang_vel_coef
        h = ctypes.c_void_p()
        try:
            _lib.check(L.rlgpu_infer_unit_create(ctypes.byref(c), ppo._h, ctypes.byref(h)), "rlgpu_infer_unit_create")
        except Exception:
            if self._owns_ppo:
                ppo.close()
            raise
        self._h = h
        self.obs_size = L.rlgpu_infer_unit_obs_size(h)
        self._calls = 0
        if one_launch:
            _lib.check(L.rlgpu_infer_unit_set_one_launch(h, 1), "rlgpu_infer_unit_set_one_launch")

    def close(self):
        if getattr(self, "_h", None):
            _lib.check(_lib.lib().rlgpu_infer_unit_destroy(self._h), "rlgpu_infer_unit_destroy")
            self._h = None
            if self._owns_ppo:
                self.ppo.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def one_launch(self):
        """The next call is one kernel launch (asked for at construction, and the policy is on the one-wave inference
        kernel), else rows + the handle's own inference path + parse."""
        return bool(_lib.lib().rlgpu_infer_unit_one_launch(self._h))

    def build_rows(self, states, rows=None, row0=0):
        """(obs [n, obs_size] float32, masks [n, 90] uint8) device tensors of the rows."""
        import torch
        states, sor, por = _rows(states, rows)
        n = len(sor)
        obs = torch.empty((max(n, 0), self.obs_size), device=self.device)
        masks = torch.empty((max(n, 0), 90), dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib().rlgpu_infer_unit_build_rows(self._h, states.ctypes.data, len(states), sor.ctypes.data,
                                                          por.ctypes.data, n, int(row0), _lib.ptr(obs), _lib.ptr(masks),
                                                          _lib.stream_ptr()), "rlgpu_infer_unit_build_rows")
        return obs, masks

    def infer(self, states, rows=None, deterministic=False, temperature=1.0, step=None, row0=0):
        """InferUnit::BatchInferActions: (actions [n, 8] float32, index [n] int32, logp [n] float32), numpy.  rows:
        (state, player) pairs, default every player of every state in order.  step None: the unit's own call counter,
        which the call advances."""
        states, sor, por = _rows(states, rows)
        n = len(sor)
        if step is None:
            step = self._calls
            self._calls += 1
        if not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature <= 0:
            raise _lib.RLGPUError(f"InferUnit.infer: temperature must be finite and > 0, got {temperature!r}")
        actions = np.zeros((max(n, 0), 8), np.float32)
        index = np.zeros(max(n, 0), np.int32)
        logp = np.zeros(max(n, 0), np.float32)
        _lib.check(_lib.lib().rlgpu_infer_unit_infer(self._h, states.ctypes.data, len(states), sor.ctypes.data,
                                                     por.ctypes.data, n, int(row0), int(deterministic), float(temperature),
                                                     int(step), index.ctypes.data, logp.ctypes.data, actions.ctypes.data,
                                                     _lib.stream_ptr()), "rlgpu_infer_unit_infer")
        return actions, index, logp

    def infer_action(self, state, player, deterministic=False, temperature=1.0, step=None):
        """InferUnit::InferAction: the parsed action [8] of one player (index in state.players) of one state."""
        return self.infer(np.asarray(state, GAMESTATE).reshape(1), [(0, int(player))], deterministic, temperature, step)[0][0]

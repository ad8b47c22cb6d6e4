"""EnvSet -- Python mirror of RLGC::EnvSet (GigaLearnCPP/RLGymCPP/src/RLGymCPP/EnvSet/EnvSet.h:67-124)
over the C ABI of include/rlgpu_env.h.  Every arena lives in HBM; the state buffers
(obs, action masks, rewards, terminals) are exposed as torch tensors that alias the
library's device memory, so the policy reads observations without a copy.

Method map (reference -> here):
    EnvSet(config)          EnvSet.cpp:46-111    -> EnvSet(num_arenas, seed, tick_skip, action_delay)
    StepFirstHalf(async)    EnvSet.cpp:113-130   -> step_first_half()
    StepSecondHalf(a, async)EnvSet.cpp:132-273   -> step_second_half(actions)
    Sync()                  EnvSet.h:107         -> sync()
    Reset()                 EnvSet.cpp:331-354   -> reset()
    ResetArena(i)           EnvSet.cpp:275-329   -> reset_arenas(mask)
    state.obs / actionMasks / rewards / terminals EnvSet.h:35-65 -> .obs / .action_masks / ...
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import alias as _alias
from .state import ARENA, GAMESTATE

OBS, ACTIONS, REWARDS, PADS, CARS = 167, 90, 13, 34, 4


class _Config(ctypes.Structure):
    _fields_ = [("num_arenas", ctypes.c_int32), ("tick_skip", ctypes.c_int32), ("action_delay", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("save_rewards", ctypes.c_int32), ("max_episode_steps", ctypes.c_int32),
                ("mesh_tris", ctypes.c_void_p), ("mesh_ntris", ctypes.c_int32), ("mesh_objects", ctypes.c_int32),
                ("mesh_object_ntris", ctypes.c_void_p), ("rewards", ctypes.c_void_p), ("n_rewards", ctypes.c_int32),
                ("terminals", ctypes.c_void_p), ("n_terminals", ctypes.c_int32), ("arith", ctypes.c_int32),
                ("arena_offset", ctypes.c_int32), ("obs_builder", ctypes.c_int32),
                ("obs_max_players", ctypes.c_int32), ("obs_pos_coef", ctypes.c_float * 3),
                ("obs_vel_coef", ctypes.c_float), ("obs_ang_vel_coef", ctypes.c_float),
                ("state_setter", ctypes.c_int32), ("state_setter_flags", ctypes.c_int32),
                ("state_setters", ctypes.c_void_p), ("n_state_setters", ctypes.c_int32)]

# the reference build whose Bullet arithmetic the arenas follow (include/rlgpu_arith.h)
ARITH_MSVC_X64, ARITH_GCC_X64, ARITH_SCALAR = 0, 1, 2
# EnvCreateResult::stateSetter (include/rlgpu_env.h RLGPU_SS_*)
KICKOFF_STATE, FUZZED_KICKOFF_STATE = 0, 1
_SS_RANDOM, _SS_COMBINED, MAX_STATE_SETTERS = 2, 3, 8
STATE_SETTER_SPEC = np.dtype([("type", np.int32), ("weight", np.float32), ("flags", np.int32)])


class RandomState:
    """RLGC::RandomState(randBallSpeed, randCarSpeed, carsOnGround) (RG/StateSetters/RandomState.h): the
    kickoff, then the ball and the four cars placed at random (RLGPU_SS_RANDOM)."""

    def __init__(self, rand_ball_speed=True, rand_car_speed=True, cars_on_ground=True):
        self.rand_ball_speed, self.rand_car_speed = bool(rand_ball_speed), bool(rand_car_speed)
        self.cars_on_ground = bool(cars_on_ground)

    @property
    def flags(self):
        return int(self.rand_ball_speed) | int(self.rand_car_speed) << 1 | int(self.cars_on_ground) << 2

    def __repr__(self):
        return f"RandomState({self.rand_ball_speed}, {self.rand_car_speed}, {self.cars_on_ground})"


class CombinedState:
    """RLGC::CombinedState({{setter, weight}, ...}) (RG/StateSetters/CombinedState.h): every reset runs one child,
    chosen at random by weight.  Children: KICKOFF_STATE, FUZZED_KICKOFF_STATE or a RandomState."""

    def __init__(self, setters):
        self.setters = [(s, float(w)) for s, w in setters]
        state_setter_spec(self)  # reject a bad list where it is written

    def __repr__(self):
        return f"CombinedState({self.setters})"


def _plain_setter(s, who):
    """(type, flags) of a setter that is not a CombinedState."""
    if isinstance(s, RandomState):
        return _SS_RANDOM, s.flags
    if isinstance(s, (int, np.integer)) and not isinstance(s, bool) and int(s) in (KICKOFF_STATE, FUZZED_KICKOFF_STATE):
        return int(s), 0
    raise ValueError(f"{who}: {s!r} is no state setter (KICKOFF_STATE, FUZZED_KICKOFF_STATE, RandomState(...) or "
                     "CombinedState([...]))")


def state_setter_spec(setter):
    """(state_setter, state_setter_flags, children) of rlgpu_envset_config for a setter: children is a
    STATE_SETTER_SPEC array for a CombinedState, else None.  Raises ValueError naming the entry at fault."""
    if not isinstance(setter, CombinedState):
        t, f = _plain_setter(setter, "state_setter")
        return t, f, None
    if not setter.setters:
        raise ValueError("CombinedState: the setter list is empty")
    if len(setter.setters) > MAX_STATE_SETTERS:
        raise ValueError(f"CombinedState: {len(setter.setters)} setters, at most {MAX_STATE_SETTERS} "
                         "(RLGPU_MAX_STATE_SETTERS)")
    out = np.zeros(len(setter.setters), STATE_SETTER_SPEC)
    for i, (s, w) in enumerate(setter.setters):
        who = f"CombinedState: setter {i}"
        if isinstance(s, CombinedState):
            raise ValueError(f"{who} is a CombinedState: a nested CombinedState has no device code")
        t, f = _plain_setter(s, who)
        if not np.isfinite(w) or w < 0:
            raise ValueError(f"{who} ({s!r}) has a negative or invalid weight of {w}")
        out[i] = (t, w, f)
    return _SS_COMBINED, 0, out


class _AdvancedObs:
    """RLGC::AdvancedObs (RLGPU_OBS_ADVANCED), the default obs builder: 167 floats."""
    kind, obs_size, max_players = 0, OBS, 0

    def __repr__(self):
        return "ADVANCED_OBS"


ADVANCED_OBS = _AdvancedObs()


class DefaultObs:
    """RLGC::DefaultObs(posCoef, velCoef, angVelCoef) (RG/ObsBuilders/DefaultObs.h, RLGPU_OBS_DEFAULT): 127 floats.
    The defaults are the reference's: (1/4096, 1/5120, 1/2044), 1/2300, 1/5.5 in float32."""
    kind, obs_size, max_players = 1, 127, 0

    def __init__(self, pos_coef=None, vel_coef=None, ang_vel_coef=None):
        f = np.float32
        pos = (f(1) / f(4096), f(1) / f(5120), f(1) / f(2044)) if pos_coef is None else tuple(pos_coef)
        if len(pos) != 3:
            raise ValueError(f"{type(self).__name__}: pos_coef must have 3 components, got {len(pos)}")
        self.pos_coef = tuple(float(f(x)) for x in pos)
        self.vel_coef = float(f(1) / f(2300) if vel_coef is None else f(vel_coef))
        self.ang_vel_coef = float(f(1) / f(5.5) if ang_vel_coef is None else f(ang_vel_coef))
        for name, v in (("pos_coef", self.pos_coef), ("vel_coef", (self.vel_coef,)),
                        ("ang_vel_coef", (self.ang_vel_coef,))):
            if not all(np.isfinite(x) for x in v):
                raise ValueError(f"{type(self).__name__}: {name} is not finite ({v})")
        if not any(self.pos_coef) and not self.vel_coef and not self.ang_vel_coef:
            raise ValueError(f"{type(self).__name__}: all coefficients are zero, which the C ABI reads as "
                             "\"the defaults\" (rlgpu_envset_config)")

    def __repr__(self):
        return f"{type(self).__name__}({self.pos_coef}, {self.vel_coef}, {self.ang_vel_coef})"


class DefaultObsPadded(DefaultObs):
    """RLGC::DefaultObsPadded(maxPlayers, posCoef, velCoef, angVelCoef) (RLGPU_OBS_DEFAULT_PADDED): the row of a
    DefaultObs with max_players - 1 teammate and max_players opponent slots, each list shuffled, 51 + 38 x
    max_players floats.  max_players is 2 or 3 in 2v2."""
    kind = 2

    def __init__(self, max_players, pos_coef=None, vel_coef=None, ang_vel_coef=None):
        if isinstance(max_players, bool) or not isinstance(max_players, (int, np.integer)):
            raise ValueError(f"DefaultObsPadded: max_players must be an integer, got {max_players!r}")
        self.max_players = int(max_players)
        if self.max_players < 2:
            raise ValueError(f"DefaultObsPadded: max_players {self.max_players} leaves {self.max_players - 1} "
                             "teammate slots, and a 2v2 player has one teammate")
        if self.max_players > 3:
            raise ValueError(f"DefaultObsPadded: max_players {self.max_players} makes rows of "
                             f"{51 + 38 * self.max_players} floats, and the env kernel's staging rows hold {OBS} "
                             "(max_players 2 or 3)")
        self.obs_size = 51 + 38 * self.max_players
        super().__init__(pos_coef, vel_coef, ang_vel_coef)

    def __repr__(self):
        return f"DefaultObsPadded({self.max_players}, {self.pos_coef}, {self.vel_coef}, {self.ang_vel_coef})"


def obs_builder_spec(builder):
    """The obs builder as an ADVANCED_OBS / DefaultObs / DefaultObsPadded object (None = ADVANCED_OBS); raises
    ValueError naming anything else."""
    if builder is None:
        return ADVANCED_OBS
    if isinstance(builder, (_AdvancedObs, DefaultObs)):
        return builder
    raise ValueError(f"obs_builder: {builder!r} is no obs builder (ADVANCED_OBS, DefaultObs(...) or "
                     "DefaultObsPadded(max_players, ...))")


def set_obs_builder(cfg, builder):
    """Fill the obs_* fields of an rlgpu_envset_config / rlgpu_learner_config mirror from a builder object."""
    b = obs_builder_spec(builder)
    cfg.obs_builder, cfg.obs_max_players = b.kind, b.max_players
    if b.kind:
        cfg.obs_pos_coef = (ctypes.c_float * 3)(*b.pos_coef)
        cfg.obs_vel_coef, cfg.obs_ang_vel_coef = b.vel_coef, b.ang_vel_coef
    return b


class StepOutputs(ctypes.Structure):
    """rlgpu_step_outputs: experience-append destinations of the fused step (device pointers)."""
    _fields_ = [("obs", ctypes.c_void_p), ("masks", ctypes.c_void_p), ("rewards", ctypes.c_void_p),
                ("terminals", ctypes.c_void_p), ("trunc_obs", ctypes.c_void_p)]

    @classmethod
    def of(cls, obs=None, masks=None, rewards=None, terminals=None, trunc_obs=None):
        for t, n in ((obs, "obs"), (masks, "masks"), (rewards, "rewards"), (terminals, "terminals"),
                     (trunc_obs, "trunc_obs")):
            _lib.require_gpu_tensor(t, n)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return cls(p(obs), p(masks), p(rewards), p(terminals), p(trunc_obs))


class _Buffers(ctypes.Structure):
    _fields_ = [("obs", ctypes.c_void_p), ("action_masks", ctypes.c_void_p), ("rewards", ctypes.c_void_p),
                ("terminals", ctypes.c_void_p), ("last_rewards", ctypes.c_void_p), ("trunc_obs", ctypes.c_void_p),
                ("num_players", ctypes.c_int32), ("num_arenas", ctypes.c_int32), ("num_rewards", ctypes.c_int32),
                ("arena_player_start", ctypes.c_void_p)]


_bound = False


def _bind():
    global _bound
    if _bound:
        return _lib.lib()
    L = _lib.lib()
    if L.rlgpu_envset_config_size() != ctypes.sizeof(_Config):
        raise _lib.RLGPUError(f"rlgpu_envset_config is {L.rlgpu_envset_config_size()} bytes in the library, "
                              f"{ctypes.sizeof(_Config)} in rlgpu/env.py: the binding is out of date")
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.rlgpu_envset_create.argtypes = [ctypes.POINTER(_Config), ctypes.POINTER(vp)]
    L.rlgpu_envset_destroy.argtypes = [vp]
    L.rlgpu_envset_buffers_get.argtypes = [vp, ctypes.POINTER(_Buffers)]
    L.rlgpu_envset_obs_size.argtypes = [vp]
    L.rlgpu_obs_builder_size.argtypes = [i32, i32]
    L.rlgpu_envset_reset.argtypes = [vp, vp]
    L.rlgpu_envset_reset_arenas.argtypes = [vp, vp, vp]
    L.rlgpu_envset_step_first_half.argtypes = [vp, vp]
    L.rlgpu_envset_step_second_half.argtypes = [vp, vp, vp]
    L.rlgpu_envset_step.argtypes = [vp, vp, i32, ctypes.POINTER(StepOutputs), vp]
    L.rlgpu_envset_step_range.argtypes = [vp, i32, i32, vp, i32, ctypes.POINTER(StepOutputs), vp]
    L.rlgpu_envset_sync.argtypes = [vp, vp]
    L.rlgpu_envset_build_obs.argtypes = [vp, vp]
    L.rlgpu_envset_get_arenas.argtypes = [vp, i32, i32, vp]
    L.rlgpu_envset_set_arenas.argtypes = [vp, i32, i32, vp]
    L.rlgpu_step_metric_name.argtypes = [i32]
    L.rlgpu_step_metric_name.restype = ctypes.c_char_p
    L.rlgpu_envset_enable_step_metrics.argtypes = [vp, i32]
    L.rlgpu_envset_step_metrics.argtypes = [vp, vp, vp, i32, vp]
    L.rlgpu_envset_step_metric_slots.argtypes = [vp, vp, vp]
    L.rlgpu_envset_download_gamestates.argtypes = [vp, i32, i32, vp, vp]
    L.rlgpu_gamestates_from_arenas.argtypes = [vp, i32, i32, vp]
    L.rlgpu_envset_enable_reward_values.argtypes = [vp, i32]
    L.rlgpu_envset_reward_values.argtypes = [vp]
    L.rlgpu_envset_reward_values.restype = vp
    _bound = True
    return L


def obs_builder_size(kind, max_players=0):
    """rlgpu_obs_builder_size: the row width of an obs builder kind (167 / 127 / 51 + 38 x max_players); raises
    RLGPUError naming a refused kind or max_players."""
    w = _bind().rlgpu_obs_builder_size(int(kind), int(max_players))
    if w < 0:
        _lib.check(1, "rlgpu_obs_builder_size")
    return w


def arena_state_size():
    return _lib.lib().rlgpu_arena_state_size()


def config_size():
    """sizeof(rlgpu_envset_config) in the library, for checking the _Config mirror."""
    return _lib.lib().rlgpu_envset_config_size()


def gamestate_size():
    return _lib.lib().rlgpu_gamestate_size()


def gamestates_from_arenas(buf, tick_skip=8):
    """GameState records (numpy GAMESTATE array) of wire-format arena records (rlgpu_gamestates_from_arenas,
    GameState::UpdateFromArena on the record)."""
    L = _bind()
    buf = np.ascontiguousarray(buf, np.uint8)
    count = buf.size // ARENA.itemsize
    out = np.zeros(count, GAMESTATE)
    _lib.check(L.rlgpu_gamestates_from_arenas(buf.ctypes.data_as(ctypes.c_void_p), count, int(tick_skip),
                                              out.ctypes.data_as(ctypes.c_void_p)), "rlgpu_gamestates_from_arenas")
    return out


class EnvSet:
    """Vectorised 2v2 arena set resident in HBM (AdvancedObs / DefaultObs / DefaultObsPadded, DefaultAction, a state setter, and a
    reward / terminal list from the device registry -- ExampleMain's 13 rewards and NoTouch(8 s) +
    ScoreLimit(3) by default)."""

    def __init__(self, num_arenas, seed=1234, tick_skip=8, action_delay=7, save_rewards=True, device="cuda:0",
                 max_episode_steps=0, mesh=None, rewards=None, terminals=None, arith=ARITH_MSVC_X64, arena_offset=0,
                 state_setter=KICKOFF_STATE, obs_builder=None):
        """mesh: an rlgpu.mesh.ArenaMesh (e.g. ArenaMesh.from_folder("collision_meshes")), or None for
        the built-in synthetic arena mesh.  rewards / terminals: lists of rlgpu.plugins.reward(...) /
        terminal(...) specs (or structured arrays), None = ExampleMain's.  arith: the reference build
        whose Bullet arithmetic the step follows (ARITH_MSVC_X64 = build.ps1's, ARITH_GCC_X64, ARITH_SCALAR).
        arena_offset: global index of arena 0 for the arenas' random streams (a rank's first arena).
        state_setter: KICKOFF_STATE, FUZZED_KICKOFF_STATE (the skill tracker's, rlgpu.skill), a RandomState or a
        CombinedState of those.  obs_builder: ADVANCED_OBS (None), a DefaultObs or a DefaultObsPadded; self.obs_size
        is its row width."""
        import torch
        if not torch.cuda.is_available():
            raise _lib.RLGPUError("EnvSet needs an MI355X: the product path has no CPU fallback")
        L = _bind()
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        cfg = _Config(num_arenas, tick_skip, action_delay, seed, int(save_rewards), max_episode_steps)
        cfg.arith = int(arith)
        cfg.arena_offset = int(arena_offset)
        cfg.state_setter, cfg.state_setter_flags, self._ss = state_setter_spec(state_setter)
        if self._ss is not None:
            cfg.state_setters, cfg.n_state_setters = self._ss.ctypes.data, self._ss.size
        self.arith = int(arith)
        self.obs_builder = set_obs_builder(cfg, obs_builder)
        if mesh is not None:
            cfg.mesh_tris = mesh.tris.ctypes.data
            cfg.mesh_ntris = mesh.num_tris
            cfg.mesh_objects = mesh.num_objects
            cfg.mesh_object_ntris = mesh.object_ntris.ctypes.data
        from . import plugins
        # a non-NULL list pointer selects the given list, even an empty one (a 1-record buffer then)
        if rewards is not None:
            rw = rewards if isinstance(rewards, np.ndarray) else plugins.rewards_array(rewards)
            self._rw = np.ascontiguousarray(rw if rw.size else np.zeros(1, plugins.REWARD_SPEC))
            cfg.rewards, cfg.n_rewards = self._rw.ctypes.data, rw.size
        if terminals is not None:
            tc = terminals if isinstance(terminals, np.ndarray) else plugins.terminals_array(terminals)
            self._tc = np.ascontiguousarray(tc if tc.size else np.zeros(1, plugins.TERMINAL_SPEC))
            cfg.terminals, cfg.n_terminals = self._tc.ctypes.data, tc.size
        h = ctypes.c_void_p()
        _lib.check(L.rlgpu_envset_create(ctypes.byref(cfg), ctypes.byref(h)), "rlgpu_envset_create")
        self._h = h
        self.tick_skip, self.action_delay = tick_skip, action_delay
        self._alias_buffers(L)

    @classmethod
    def wrap(cls, handle, device, tick_skip=8, action_delay=7, owner=None):
        """An EnvSet view of a handle owned elsewhere (the C++ Learner's RLGC::EnvSetGPU)."""
        import torch
        L = _bind()
        self = cls.__new__(cls)
        self._h, self._owned, self._owner = ctypes.c_void_p(handle), False, owner
        self.device = torch.device(device)
        self.tick_skip, self.action_delay = tick_skip, action_delay
        self._alias_buffers(L)
        return self

    _owned = True

    def _alias_buffers(self, L):
        import torch
        b = _Buffers()
        _lib.check(L.rlgpu_envset_buffers_get(self._h, ctypes.byref(b)), "rlgpu_envset_buffers_get")
        self.num_arenas, self.num_players, self.num_rewards = b.num_arenas, b.num_players, b.num_rewards
        P, N, dev = b.num_players, b.num_arenas, self.device
        self.obs_size = W = L.rlgpu_envset_obs_size(self._h)
        self.obs = _alias(b.obs, (P, W), torch.float32, dev)
        self.action_masks = _alias(b.action_masks, (P, ACTIONS), torch.uint8, dev)
        self.rewards = _alias(b.rewards, (P,), torch.float32, dev)
        self.terminals = _alias(b.terminals, (N,), torch.uint8, dev)
        self.last_rewards = _alias(b.last_rewards, (N, self.num_rewards), torch.float32, dev)
        self.trunc_obs = _alias(b.trunc_obs, (P, W), torch.float32, dev)
        self.arena_player_start = _alias(b.arena_player_start, (N,), torch.int32, dev)

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                _lib.check(_lib.lib().rlgpu_envset_destroy(self._h), "rlgpu_envset_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _actions(actions):
        import torch
        _lib.require_gpu_tensor(actions, "actions")
        if actions.dtype != torch.int32 or not actions.is_contiguous():
            raise _lib.RLGPUError("actions must be a contiguous int32 device tensor [num_players]")
        return _lib.ptr(actions)

    def step_first_half(self, stream=None):
        _lib.check(_lib.lib().rlgpu_envset_step_first_half(self._h, _lib.stream_ptr(stream)), "step_first_half")

    def step_second_half(self, actions, stream=None):
        _lib.check(_lib.lib().rlgpu_envset_step_second_half(self._h, self._actions(actions), _lib.stream_ptr(stream)),
                   "step_second_half")

    def step(self, actions, reset_terminated=True, out=None, stream=None):
        """Fused StepFirstHalf + StepSecondHalf (+ Reset of terminated arenas); `out` is a
        StepOutputs (experience append into rollout rows) or None."""
        o = ctypes.byref(out) if out is not None else None
        _lib.check(_lib.lib().rlgpu_envset_step(self._h, self._actions(actions), int(reset_terminated), o,
                                                _lib.stream_ptr(stream)), "rlgpu_envset_step")

    def step_range(self, first, count, actions, reset_terminated=True, out=None, stream=None):
        """The fused step of arenas [first, first + count) only (rlgpu_envset_step_range; first a multiple
        of 4).  `actions` is the whole set's [num_players] tensor; `out` holds the range's players' rows."""
        o = ctypes.byref(out) if out is not None else None
        a = ctypes.c_void_p(self._actions(actions).value + CARS * int(first) * actions.element_size())
        _lib.check(_lib.lib().rlgpu_envset_step_range(self._h, int(first), int(count), a, int(reset_terminated), o,
                                                      _lib.stream_ptr(stream)), "rlgpu_envset_step_range")

    def set_output_only(self, on=True):
        """rlgpu_envset_set_output_only: rows given to step(out=...) go only there, not also to self.obs /
        self.action_masks / self.trunc_obs."""
        _lib.check(_lib.lib().rlgpu_envset_set_output_only(self._h, int(on)), "rlgpu_envset_set_output_only")

    def sync(self, stream=None):
        _lib.check(_lib.lib().rlgpu_envset_sync(self._h, _lib.stream_ptr(stream)), "sync")

    def reset(self, stream=None):
        _lib.check(_lib.lib().rlgpu_envset_reset(self._h, _lib.stream_ptr(stream)), "reset")

    def reset_arenas(self, mask=None, stream=None):
        _lib.require_gpu_tensor(mask, "mask")
        _lib.check(_lib.lib().rlgpu_envset_reset_arenas(self._h, _lib.ptr(mask), _lib.stream_ptr(stream)),
                   "reset_arenas")

    def build_obs(self, stream=None):
        _lib.check(_lib.lib().rlgpu_envset_build_obs(self._h, _lib.stream_ptr(stream)), "build_obs")

    def get_arenas(self, first=0, count=None):
        """Wire-format snapshot (uint8 [count * arena_state_size()]) of arenas [first, first+count)."""
        import torch
        torch.cuda.synchronize(self.device)
        count = self.num_arenas - first if count is None else count
        buf = np.zeros(count * ARENA.itemsize, np.uint8)
        _lib.check(_lib.lib().rlgpu_envset_get_arenas(self._h, first, count, buf.ctypes.data_as(ctypes.c_void_p)),
                   "get_arenas")
        return buf

    def set_arenas(self, buf, first=0):
        import torch
        torch.cuda.synchronize(self.device)
        buf = np.ascontiguousarray(buf, np.uint8)
        count = buf.size // ARENA.itemsize
        _lib.check(_lib.lib().rlgpu_envset_set_arenas(self._h, first, count, buf.ctypes.data_as(ctypes.c_void_p)),
                   "set_arenas")

    def gamestates(self, first=0, count=None, stream=None):
        """RLGC::GameState records (numpy GAMESTATE array, rlgpu.state) of arenas [first, first+count) as the
        last step left them: what the reference hands a StepCallbackFn (Learner.cpp:796-797)."""
        count = self.num_arenas - first if count is None else count
        out = np.zeros(count, GAMESTATE)
        _lib.check(_bind().rlgpu_envset_download_gamestates(self._h, first, count, out.ctypes.data_as(ctypes.c_void_p),
                                                            _lib.stream_ptr(stream)), "download_gamestates")
        return out

    def enable_reward_values(self, on=True):
        """Every later builders launch writes each reward's value before its weight: reward_values() is then
        a [num_players, num_rewards] device tensor (None while disabled)."""
        _lib.check(_bind().rlgpu_envset_enable_reward_values(self._h, int(on)), "enable_reward_values")

    def reward_values(self):
        import torch
        p = _bind().rlgpu_envset_reward_values(self._h)
        if not p:
            return None
        return _alias(p, (self.num_players, max(self.num_rewards, 1)), torch.float32, self.device)

    # ---- ExampleMain's StepCallback metrics (include/rlgpu_env.h rlgpu_envset_step_metrics)
    STEP_METRIC_SLOTS = 32

    @staticmethod
    def step_metric_names():
        L = _bind()
        return [L.rlgpu_step_metric_name(i).decode() for i in range(8)]

    def enable_step_metrics(self, on=True):
        """Every later builders launch (fused step / second half) is one StepCallback call."""
        _lib.check(_bind().rlgpu_envset_enable_step_metrics(self._h, int(on)), "enable_step_metrics")

    def step_metrics(self, reset=False, stream=None):
        """{Report key: (total, count)} since the last reset (Report::Avg, Report.h:11-45)."""
        tot, cnt = np.zeros(8, np.float64), np.zeros(8, np.uint64)
        _lib.check(_bind().rlgpu_envset_step_metrics(self._h, tot.ctypes.data_as(ctypes.c_void_p),
                                                     cnt.ctypes.data_as(ctypes.c_void_p), int(reset),
                                                     _lib.stream_ptr(stream)), "step_metrics")
        return {k: (float(t), int(c)) for k, t, c in zip(self.step_metric_names(), tot, cnt)}

    def step_metric_slots(self, stream=None):
        """The raw per-arena fp64 slots [num_arenas, 32]."""
        out = np.zeros((self.num_arenas, self.STEP_METRIC_SLOTS), np.float64)
        _lib.check(_bind().rlgpu_envset_step_metric_slots(self._h, out.ctypes.data_as(ctypes.c_void_p),
                                                          _lib.stream_ptr(stream)), "step_metric_slots")
        return out

    def serialize_arena(self, index):
        """RocketSim Arena::Serialize bytes of arena `index` (rlgpu.arena_wire)."""
        from . import arena_wire
        return arena_wire.envset_serialize(self, index)

    def deserialize_arena(self, index, data):
        """Arena::DeserializeNew of `data` into arena `index`; returns the bytes consumed (build_obs()
        refreshes the arena's obs / mask rows)."""
        from . import arena_wire
        return arena_wire.envset_deserialize(self, index, data)

"""The reference of the device state setters RLGPU_SS_RANDOM and RLGPU_SS_COMBINED: one copy, shared by
test_state_setters (CPU) and test_state_setters_gpu.

It restates RLGymCPP's RandomState::ResetArena (RG/StateSetters/RandomState.cpp:11-63) and
CombinedState::ResetArena (CombinedState.h:33-41) in numpy float32, operation by operation, on top of what the
oracle already gives: the kickoff (oracle.EnvSet.reset_arenas, its 4 shuffle draws, the pads, the env
bookkeeping), the wire format (get_arenas / set_arenas), build_obs and the deterministic sine / cosine
(oracle.detmath_trig = rs_sinf / rs_cosf).  It is a restatement of the source, not of the kernel.

The stream.  Draw k of arena a is philox0(seed, a, k) (Philox4x32-10, first word; a = the arena's global index, k =
the record's env.rng_counter, advanced by one per draw) and RocketSim's RandFloat fraction is
u = (x >> 8) * 2^-24; RandFloat(lo, hi) = lo + u * (hi - lo) (RocketSim Math.cpp:54-57).  test_state_setters
anchors this generator to the engine's stream by rebuilding the oracle's FuzzedKickoffState from it.

The draw order the reference leaves open (unspecified operand order, an unordered_set walk, a time-seeded engine)
is fixed as DESIGN.md section 6 states it: the source text read left to right, cars in index order.
    CombinedState          1    f = RandFloat(0, totalWeight), before the child's own draws
    kickoff                4    the spawn shuffle (the oracle's)
    FuzzedKickoffState    12    after the kickoff
    RandomState ball       3    position x, y, z
      randBallSpeed       +7    direction x, y, z; speed; angular velocity x, y, z
    RandomState per car    3    position x, y, z
      randCarSpeed       +10    the unused randVelDir 3; direction 3; speed 1; angular direction 3
                           3    yaw, pitch, roll
      !carsOnGround       +1    the on-ground coin RandFloat() > 0.5
                           1    boost
"""
import ctypes

import numpy as np

import oracle

KICKOFF, FUZZED, RANDOM, COMBINED = 0, 1, 2, 3
RAND_BALL_SPEED, RAND_CAR_SPEED, CARS_ON_GROUND = 1, 2, 4

F = np.float32
UU2BT = F(1) / F(50)
BT2UU = F(50)
EPS2 = F(1.1920928955078125e-07) * F(1.1920928955078125e-07)  # FLT_EPSILON * FLT_EPSILON (Vec::Normalized)
PI = F(np.pi)           # (float)M_PI
HALF_PI = F(np.pi / 2)  # (float)(M_PI / 2)
X_MAX, Y_MAX, Z_MAX, CAR_Z_MIN, BALL_RADIUS = F(3500), F(4000), F(1820), F(150), F(92.75)


def philox0(seed, arena, counter):
    """First output word of Philox4x32-10 with key `seed` (low, high word) and counter (arena, counter,
    0x9E3779B9, 0x85EBCA6B): the engine's per-arena stream.  Scalars or arrays (broadcast); returns uint32."""
    seed = int(seed)
    M = np.uint64(0xFFFFFFFF)
    x0 = np.asarray(arena, np.uint64) & M
    x1 = np.asarray(counter, np.uint64) & M
    x0, x1 = np.broadcast_arrays(x0, x1)
    x2 = np.full(x0.shape, 0x9E3779B9, np.uint64)
    x3 = np.full(x0.shape, 0x85EBCA6B, np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * x0
        p1 = np.uint64(0xCD9E8D57) * x2
        y0 = (p1 >> np.uint64(32)) ^ x1 ^ np.uint64(k0)
        y2 = (p0 >> np.uint64(32)) ^ x3 ^ np.uint64(k1)
        x0, x1, x2, x3 = y0, p1 & M, y2, p0 & M
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return x0.astype(np.uint32)


def uniform(x):
    """RandFloat's fraction of a draw: (x >> 8) * 2^-24, float32 in [0, 1)."""
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * F(1.0 / 16777216.0)


class Stream:
    """The draws of one arena record, in order: reads and advances rec["env"]["rng_counter"]."""

    BLOCK = 96  # draws generated at a time (a RandomState reset takes at most 87)

    def __init__(self, rec, seed, arena):
        self.rec, self.seed, self.arena = rec, seed, arena
        self.base, self.block = 0, ()

    def u(self):
        k = int(self.rec["env"]["rng_counter"])
        self.rec["env"]["rng_counter"] = (k + 1) & 0xFFFFFFFF
        if not self.base <= k < self.base + len(self.block):
            self.base = k
            self.block = uniform(philox0(self.seed, self.arena, (k + np.arange(self.BLOCK)) & 0xFFFFFFFF))
        return F(self.block[k - self.base])

    def rand_float(self, lo=F(0), hi=F(1)):  # RocketSim Math::RandFloat
        lo, hi = F(lo), F(hi)
        return F(lo + F(self.u() * F(hi - lo)))

    def rand_vec(self, lo, hi):  # RLGC Math::RandVec (RG/Math.cpp:3-9): x, y, z
        return [self.rand_float(lo[0], hi[0]), self.rand_float(lo[1], hi[1]), self.rand_float(lo[2], hi[2])]

    def rand_norm_vec(self):  # RandNormVec (RandomState.cpp:7-9)
        return normalized(self.rand_vec((-1, -1, -1), (1, 1, 1)))


def normalized(v):
    """Vec::Normalized (MathTypes.h:88-95) over Vec::Length: true division, the zero vector when too short."""
    x, y, z = v
    l2 = F(F(F(x * x) + F(y * y)) + F(z * z))
    length = F(np.sqrt(l2)) if l2 > 0 else F(0)
    if length > EPS2:
        return [F(x / length), F(y / length), F(z / length)]
    return [F(0), F(0), F(0)]


def scaled(v, s):
    return [F(c * F(s)) for c in v]


def euler_ypr(yaw, pitch, roll):
    """btMatrix3x3::setEulerYPR(yaw, pitch, roll) (btMatrix3x3.h:290-321) row-major, on rs_sinf / rs_cosf."""
    ang = np.array([roll, pitch, yaw], np.float32)
    si, sj, sh = (F(v) for v in oracle.detmath_trig("sin", ang))
    ci, cj, ch = (F(v) for v in oracle.detmath_trig("cos", ang))
    cc, cs, sc, ss = F(ci * ch), F(ci * sh), F(si * ch), F(si * sh)
    return np.array([F(cj * ch), F(F(sj * sc) - cs), F(F(sj * cc) + ss),
                     F(cj * sh), F(F(sj * ss) + cc), F(F(sj * cs) - sc),
                     F(-sj), F(cj * si), F(cj * ci)], np.float32)


def random_draws(flags):
    """Draws RandomState takes after its kickoff."""
    ball = 3 + (7 if flags & RAND_BALL_SPEED else 0)
    car = 3 + (10 if flags & RAND_CAR_SPEED else 0) + 3 + (0 if flags & CARS_ON_GROUND else 1) + 1
    return ball + 4 * car


def draw_count(kind, flags=0, combined=False):
    """Draws one reset takes: the documented count per setter and flag set."""
    return int(combined) + 4 + (12 if kind == FUZZED else 0) + (random_draws(flags) if kind == RANDOM else 0)


def random_state(rec, seed, arena, flags):
    """RandomState::ResetArena after its Arena::ResetToRandomKickoff, on one kickoff record (an element of a
    structured ARENA array, changed in place): Ball::SetState / Car::SetState of default states with the drawn
    fields (uu -> Bullet units on position and velocity, angular velocity as is, isOnGround = true whatever the
    height: a fresh kickoff record already holds every other default)."""
    s = Stream(rec, seed, arena)
    pos = s.rand_vec((-X_MAX, -Y_MAX, BALL_RADIUS), (X_MAX, Y_MAX, Z_MAX))
    vel, ang = [F(0)] * 3, [F(0)] * 3
    if flags & RAND_BALL_SPEED:
        d = s.rand_norm_vec()
        vel = scaled(d, s.rand_float(0, 4000))
        ang = s.rand_vec((-4, -4, -4), (4, 4, 4))
    ball = rec["ball"]
    ball["pos"] = scaled(pos, UU2BT)
    ball["rot"] = np.eye(3, dtype=np.float32).ravel()
    ball["vel"] = scaled(vel, UU2BT)
    ball["angvel"] = ang
    rec["ball_vel_impulse_cache"] = 0
    for ci in range(4):
        pos = s.rand_vec((-X_MAX, -Y_MAX, CAR_Z_MIN), (X_MAX, Y_MAX, Z_MAX))
        vel, ang = [F(0)] * 3, [F(0)] * 3
        if flags & RAND_CAR_SPEED:
            s.rand_vec((-1, -1, -1), (1, 1, 1))  # randVelDir: drawn, never used
            d = s.rand_norm_vec()
            vel = scaled(d, s.rand_float(0, 2300))
            ang = scaled(s.rand_norm_vec(), 5.5)
        yaw = s.rand_float(-PI, PI)
        pitch = s.rand_float(-HALF_PI, HALF_PI)
        roll = s.rand_float(-PI, PI)
        on_ground = True if flags & CARS_ON_GROUND else bool(s.rand_float() > F(0.5))
        if on_ground:
            pos[2] = F(17)
            pitch = roll = F(0)
            vel[2] = F(0)
            ang = [F(0)] * 3
        rot = euler_ypr(yaw, F(-pitch), F(-roll))  # Angle::ToRotMat: setEulerYPR(yaw, -pitch, -roll)
        boost = s.rand_float(0, 100)
        car = rec["cars"][ci]
        car["body"]["pos"] = scaled(pos, UU2BT)
        car["body"]["rot"] = rot
        car["body"]["vel"] = scaled(vel, UU2BT)
        car["body"]["angvel"] = ang
        car["vel_impulse_cache"] = 0
        car["boost"] = boost
        car["is_on_ground"] = 1


def fuzzed_kickoff(rec, seed, arena):
    """FuzzedKickoffState after its kickoff (FuzzedKickoffState.h:7-26): every car's position moved by
    RandFloat(-0.1, 0.1) uu per axis through a CarState (Bullet units -> uu -> Bullet units, the velocity too).
    The oracle has its own; this one exists to anchor the generator against it."""
    s = Stream(rec, seed, arena)
    for ci in range(4):
        b = rec["cars"][ci]["body"]
        for k in range(3):
            r = s.rand_float(-0.1, 0.1)
            b["pos"][k] = F(F(F(b["pos"][k]) * BT2UU + r) * UU2BT)
            b["vel"][k] = F(F(F(b["vel"][k]) * BT2UU) * UU2BT)


def as_children(setter):
    """(combined, [(type, weight, flags), ...]) of a setter given as ("kickoff" | "fuzzed" | ("random", flags)) or
    ("combined", [(child, weight), ...])."""
    def plain(s):
        if s == "kickoff":
            return KICKOFF, 0
        if s == "fuzzed":
            return FUZZED, 0
        assert s[0] == "random", s
        return RANDOM, int(s[1])
    if isinstance(setter, tuple) and setter[0] == "combined":
        return True, [(*plain(c)[:1], F(w), plain(c)[1]) for c, w in setter[1]]
    t, f = plain(setter)
    return False, [(t, F(1), f)]


def combined_pick(stream, children):
    """CombinedState::ResetArena's choice: f = RandFloat(0, totalWeight), the first child with
    f <= cumulativeWeights[i]; the weights summed in float32 in list order."""
    cum, total = [], F(0)
    for _, w, _ in children:
        total = F(total + F(w))
        cum.append(total)
    f = stream.rand_float(0, total)
    for i, c in enumerate(cum):
        if f <= c:
            return i
    raise AssertionError("CombinedState ran out of setters")


def reset(o, mask, setter, seed, arena_offset=0):
    """The setter's reset of the arenas of oracle set `o` where mask != 0 (None: all), with their obs / mask
    rows rebuilt: CombinedState's draw first, then the oracle's own kickoff (or fuzzed kickoff) on the same
    stream, then RandomState on top.  Returns each arena's child index (-1 where not reset)."""
    from rlgpu.state import ARENA
    n = o.n
    mask = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    combined, children = as_children(setter)
    pick = np.full(n, -1)
    rec = np.frombuffer(o.get_arenas().tobytes(), ARENA).copy()
    for i in np.nonzero(mask)[0]:
        pick[i] = combined_pick(Stream(rec[i], seed, i + arena_offset), children) if combined else 0
    o.set_arenas(rec.view(np.uint8))
    kinds = np.array([children[p][0] if p >= 0 else -1 for p in pick])
    o.L.oracle_env_set_state_setter.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for fuzz in (0, 1):
        m = mask & ((kinds == FUZZED) == bool(fuzz))
        if m.any():
            o.L.oracle_env_set_state_setter(o.h, fuzz)
            o.reset_arenas(m.astype(np.uint8))
    o.L.oracle_env_set_state_setter(o.h, 0)
    rec = np.frombuffer(o.get_arenas().tobytes(), ARENA).copy()
    for i in np.nonzero(kinds == RANDOM)[0]:
        random_state(rec[i], seed, i + arena_offset, children[pick[i]][2])
    o.set_arenas(rec.view(np.uint8))
    o.build_obs()
    return pick


def created(n, setter, seed, arena_offset=0, **kw):
    """An oracle set as EnvSet's constructor leaves it with this state setter: every arena reset once."""
    o = oracle.EnvSet(n, seed=seed, arena_offset=arena_offset, **kw)
    from rlgpu.state import ARENA
    rec = np.frombuffer(o.get_arenas().tobytes(), ARENA).copy()
    rec["env"]["rng_counter"] = 0  # the constructor's own kickoff is taken again, after CombinedState's draw
    o.set_arenas(rec.view(np.uint8))
    pick = reset(o, None, setter, seed, arena_offset)
    return o, pick

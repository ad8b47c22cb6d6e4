"""The reference of the device obs builders RLGPU_OBS_DEFAULT and RLGPU_OBS_DEFAULT_PADDED: one copy, shared by
test_default_obs (CPU) and test_default_obs_gpu.

It restates RLGymCPP's DefaultObs::BuildObs / AddPlayerToObs (RG/ObsBuilders/DefaultObs.cpp:4-54), DefaultObsPadded::
BuildObs (DefaultObsPadded.cpp:4-68) and InvertPhys (RG/Gamestates/StateUtil.cpp) in numpy float32, operation by
operation, on the GameState records the engine hands out (rlgpu_envset_download_gamestates, rlgpu.state.GAMESTATE:
RocketSim's GetState units, i.e. the record's Bullet values times 50 rounded to float32).  It is a restatement of the
source, not of the kernel.

A row of player p (team = index & 1, inverted when orange):
    ball pos * posCoef, vel * velCoef, angVel * angVelCoef      9
    prevAction                                                  8
    (float)GetBoostPads(inv)[i]: boost_pads / boost_pads_inv   34
    AddPlayerToObs(self)                                       19
    teammates, then opponents, in state.players order          19 each
AddPlayerToObs: pos * posCoef, forward, up, vel * velCoef, angVel * angVelCoef, boost / 100, isOnGround,
HasFlipOrJump (Car.cpp:279-283), isDemoed.

DefaultObsPadded pads the teammate list to maxPlayers - 1 and the opponent list to maxPlayers blocks with zero blocks
and shuffles each.  The reference's std::shuffle on a process-global engine cannot be matched; the engine's contract
is the distribution (every order equally likely, independently per row) on a stateless stream, DESIGN.md section
6.16:
    key    = splitmix64(seed ^ splitmix64(4 << 48))                         (seed: the env set's)
    draw d = philox0(key, c0 = global player (arena_offset + arena) * 4 + p, c1 = (tick_count mod 2^30) << 2 | d)
    d = 0: the teammate list's swap i = 1 (a list of 2); d = 1, 2: the opponent list's i = 2 (a list of 3) and i = 1
    Fisher-Yates from the back: for i = len - 1 .. 1: j = (draw * (i + 1)) >> 32, swap(list[i], list[j])
The kernel keys the draws on the arena record's env.tick_count; this module reads the GameState's last_tick_count.
They are equal on every record that rows are built from: the step's builders and the reset both set
last_tick_count = tick_count before the obs rows (DESIGN.md section 6.16 states the invariant).
"""
import collections

import numpy as np

from state_setter_reference import philox0

F = np.float32
ADVANCED, DEFAULT, PADDED = 0, 1, 2
BLOCK = 19
HEAD = 9 + 8 + 34
SHUFFLE_STREAM = 4
M64 = (1 << 64) - 1

Spec = collections.namedtuple("Spec", "kind max_players pos_coef vel_coef ang_vel_coef")


def spec(kind, max_players=2, pos_coef=None, vel_coef=None, ang_vel_coef=None):
    """A builder: DefaultObs's constructor defaults are 1 / SIDE_WALL_X, BACK_WALL_Y, CEILING_Z, CAR_MAX_SPEED,
    CAR_MAX_ANG_VEL in float32 (DefaultObs.h:11-15, CommonValues.h)."""
    pos = (F(1) / F(4096), F(1) / F(5120), F(1) / F(2044)) if pos_coef is None else tuple(F(x) for x in pos_coef)
    vel = F(1) / F(2300) if vel_coef is None else F(vel_coef)
    ang = F(1) / F(5.5) if ang_vel_coef is None else F(ang_vel_coef)
    return Spec(kind, 2 if kind == DEFAULT else int(max_players), np.array(pos, F), vel, ang)


def width(s):
    return HEAD + BLOCK * 2 * s.max_players


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def shuffle_key(seed):
    return splitmix64((int(seed) & M64) ^ splitmix64(SHUFFLE_STREAM << 48))


def _fisher_yates(n, draws):
    """The lists' orders after the shuffle: perm[k, pos] = the item at position pos (items numbered in the order
    they were pushed).  draws: {i: uint32 array [K]} for i = n - 1 .. 1."""
    k = len(next(iter(draws.values()))) if draws else 0
    perm = np.tile(np.arange(n), (k, 1))
    rows = np.arange(k)
    for i in range(n - 1, 0, -1):
        j = ((draws[i].astype(np.uint64) * np.uint64(i + 1)) >> np.uint64(32)).astype(np.int64)
        a, b = perm[rows, i].copy(), perm[rows, j].copy()
        perm[rows, i], perm[rows, j] = b, a
    return perm


def shuffles(seed, player, tick, max_players):
    """(teammate order [K, max_players - 1], opponent order [K, max_players]) of the rows of global players
    `player` at tick counts `tick` (arrays [K])."""
    key = shuffle_key(seed)
    player = np.asarray(player, np.uint64)
    c1 = (np.asarray(tick, np.uint64) & np.uint64((1 << 30) - 1)) << np.uint64(2)
    draw = lambda d: philox0(key, player, c1 | np.uint64(d))  # noqa: E731
    nt, no = max_players - 1, max_players
    team = _fisher_yates(nt, {1: draw(0)} if nt == 2 else {}) if nt > 1 else np.zeros((len(player), nt), np.int64)
    opp = _fisher_yates(no, {2: draw(1), 1: draw(2)} if no == 3 else {1: draw(2)})
    return team, opp


def _inv(v, inv):
    v = np.array(v, F)
    if inv:
        v[0], v[1] = -v[0], -v[1]
    return v


def player_block(p, inv, s):
    """AddPlayerToObs on one PLAYER_STATE record."""
    c = p["car"]
    rot = np.asarray(c["rot"], F)  # rows: forward, right, up
    hfj = bool(c["is_on_ground"]) or (not c["has_flipped"] and not c["has_double_jumped"]
                                      and F(c["air_time_since_jump"]) < F(1.25))
    return np.concatenate([
        _inv(c["pos"], inv) * s.pos_coef, _inv(rot[0:3], inv), _inv(rot[6:9], inv), _inv(c["vel"], inv) * s.vel_coef,
        _inv(c["ang_vel"], inv) * s.ang_vel_coef,
        np.array([F(c["boost"]) / F(100), F(bool(c["is_on_ground"])), F(hfj), F(bool(c["is_demoed"]))], F)]).astype(F)


def build_rows(gs, s, seed=0, arena_offset=0):
    """The obs rows [4 * len(gs), width(s)] float32 of GAMESTATE records `gs`, and for PADDED the opponent orders
    taken, [4 * len(gs), max_players]."""
    n = len(gs)
    out = np.zeros((4 * n, width(s)), F)
    orders = np.zeros((4 * n, s.max_players), np.int64)
    if s.kind == PADDED:
        gp = (arena_offset + np.repeat(np.arange(n), 4)) * 4 + np.tile(np.arange(4), n)
        team_order, opp_order = shuffles(seed, gp, np.repeat(gs["last_tick_count"], 4), s.max_players)
    zero = np.zeros(BLOCK, F)
    for a in range(n):
        g = gs[a]
        for p in range(4):
            me = g["players"][p]
            inv = int(me["team"]) == 1
            ball = g["ball"]
            head = [_inv(ball["pos"], inv) * s.pos_coef, _inv(ball["vel"], inv) * s.vel_coef,
                    _inv(ball["ang_vel"], inv) * s.ang_vel_coef, np.asarray(me["prev_action"], F),
                    np.asarray(g["boost_pads_inv"] if inv else g["boost_pads"]).astype(F)]
            mates, opps = [], []
            for q in range(4):
                other = g["players"][q]
                if other["car_id"] == me["car_id"]:
                    continue
                (mates if other["team"] == me["team"] else opps).append(player_block(other, inv, s))
            if s.kind == PADDED:
                assert len(mates) <= s.max_players - 1 and len(opps) <= s.max_players
                mates += [zero] * (s.max_players - 1 - len(mates))
                opps += [zero] * (s.max_players - len(opps))
                r = 4 * a + p
                mates = [mates[i] for i in team_order[r]]
                opps = [opps[i] for i in opp_order[r]]
                orders[r] = opp_order[r]
            out[4 * a + p] = np.concatenate(head + [player_block(me, inv, s)] + mates + opps)
    return out, orders

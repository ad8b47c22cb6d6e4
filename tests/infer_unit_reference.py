"""The reference of the InferUnit row kernels for AdvancedObs and DefaultAction's masks: one copy, shared by
test_infer_unit (CPU, where it is checked against the CPU oracle env) and test_infer_unit_gpu.

It restates RLGymCPP's AdvancedObs::BuildObs / AddPlayerToObsFast (RG/ObsBuilders/AdvancedObs.cpp:72-270; the
constants of AdvancedObs.h:10-13 inside the member BuildObs, those of AdvancedObs.cpp:8-11 inside the file-static
AddPlayerToObsFast) and DefaultAction's tables and GetActionMask (RG/ActionParsers/DefaultAction.cpp:3-118) in numpy
float32, operation by operation, on GameState records (rlgpu.state.GAMESTATE: RocketSim's GetState units).  It is a
restatement of the source, not of the kernel: players are taken in state.players order, self is skipped by car_id, a
player's side is its team.

A row of player p (inverted when orange):
    ball pos / 5000, vel / 2300, angVel / 3                                         9
    prevAction                                                                      8
    pads[i] ? 1 : 1 / (1 + padTimers[i])   (GetBoostPads(inv), GetBoostPadTimers(inv))   34
    AddPlayerToObsFast(self), teammates, opponents                                 29 each
GetBoostPadTimers(inverted) returns the opposite array (GameState.h:60): timers_inv for a blue player.
"""
import numpy as np

F = np.float32
PLAYER = 29
WIDTH = 9 + 8 + 34 + 4 * PLAYER

# AdvancedObs.cpp:8-11 (AddPlayerToObsFast) and AdvancedObs.h:10-13 (BuildObs's ball)
POS, VEL, ANG, BOOST = F(1.0) / F(2300.0), F(1.0) / F(2300.0), F(1.0) / F(5.5), F(0.01)
BALL_POS, BALL_VEL, BALL_ANG = F(1) / F(5000.0), F(1) / F(2300.0), F(1) / F(3.0)


def _inv(v, inv):
    v = np.array(v, F)
    if inv:
        v[0], v[1] = -v[0], -v[1]
    return v


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def has_flip_or_jump(c):
    """Player::HasFlipOrJump (Car.cpp:279-283) on a CAR_STATE record."""
    return bool(c["is_on_ground"]) or (not c["has_flipped"] and not c["has_double_jumped"]
                                       and F(c["air_time_since_jump"]) < F(1.25))


def player_block(p, inv, ball_pos, ball_vel):
    """AddPlayerToObsFast on one PLAYER_STATE record; ball_pos / ball_vel already inverted."""
    c = p["car"]
    rot = np.asarray(c["rot"], F)  # rows: forward, right, up
    pos, vel, ang = _inv(c["pos"], inv), _inv(c["vel"], inv), _inv(c["ang_vel"], inv)
    f, r, u = _inv(rot[0:3], inv), _inv(rot[3:6], inv), _inv(rot[6:9], inv)
    rel, relv = ball_pos - pos, ball_vel - vel
    out = np.zeros(PLAYER, F)
    out[0:3] = pos * POS
    out[3:6] = f
    out[6:9] = u
    out[9:12] = vel * VEL
    out[12:15] = ang * ANG
    out[15:18] = [_dot(f, ang) * ANG, _dot(r, ang) * ANG, _dot(u, ang) * ANG]
    out[18:21] = [_dot(f, rel) * POS, _dot(r, rel) * POS, _dot(u, rel) * POS]
    out[21:24] = [_dot(f, relv) * VEL, _dot(r, relv) * VEL, _dot(u, relv) * VEL]
    out[24] = F(c["boost"]) * BOOST
    out[25] = F(bool(c["is_on_ground"]))
    out[26] = F(has_flip_or_jump(c))
    out[27] = F(bool(c["is_demoed"]))
    out[28] = F(bool(c["has_jumped"]))
    return out


def build_row(g, p):
    """AdvancedObs::BuildObs(state.players[p], state) on one GAMESTATE record."""
    me = g["players"][p]
    inv = int(me["team"]) == 1
    ball = g["ball"]
    bpos, bvel, bang = _inv(ball["pos"], inv), _inv(ball["vel"], inv), _inv(ball["ang_vel"], inv)
    pads = np.asarray(g["boost_pads_inv"] if inv else g["boost_pads"])
    timers = np.asarray(g["boost_pad_timers"] if inv else g["boost_pad_timers_inv"], F)
    with np.errstate(divide="ignore"):
        pad_obs = np.where(pads != 0, F(1.0), F(1.0) / (F(1.0) + timers)).astype(F)
    parts = [bpos * BALL_POS, bvel * BALL_VEL, bang * BALL_ANG, np.asarray(me["prev_action"], F), pad_obs,
             player_block(me, inv, bpos, bvel)]
    for same_team in (True, False):
        for q in range(len(g["players"])):
            other = g["players"][q]
            if other["car_id"] == me["car_id"]:
                continue
            if (other["team"] == me["team"]) == same_team:
                parts.append(player_block(other, inv, bpos, bvel))
    return np.concatenate(parts).astype(F)


def build_rows(gs, rows=None):
    """Rows [n, 167] of (state, player) pairs of GAMESTATE records `gs`; default every player of every state."""
    if rows is None:
        rows = [(a, p) for a in range(len(gs)) for p in range(4)]
    return np.stack([build_row(gs[a], p) for a, p in rows])


def action_table():
    """DefaultAction's constructor: (actions [90, 8], ground, air, jump, boost masks [90] each)."""
    rb, rf = (0.0, 1.0), (-1.0, 0.0, 1.0)
    acts = []
    for throttle in rf:
        for steer in rf:
            for boost in rb:
                for handbrake in rb:
                    if boost == 1 and throttle != 1:
                        continue
                    acts.append([throttle, steer, 0, steer, 0, 0, boost, handbrake])
    ng = len(acts)
    for pitch in rf:
        for yaw in rf:
            for roll in rf:
                for jump in rb:
                    for boost in rb:
                        if jump == 1 and yaw != 0:
                            continue
                        if pitch == roll and roll == jump and jump == 0:
                            continue
                        handbrake = float(jump == 1 and (pitch != 0 or yaw != 0 or roll != 0))
                        acts.append([boost, yaw, pitch, yaw, roll, jump, boost, handbrake])
    t = np.array(acts, F)
    n = len(t)
    ground, air, jumpm, boostm = (np.zeros(n, np.uint8) for _ in range(4))
    for i in range(n):
        thr, _, _, yaw, _, jump, boost, hb = t[i]
        if jump:
            jumpm[i] = 1
        if boost:
            boostm[i] = 1
        if i < ng:
            ground[i] = 1
        if i > ng and not jump:
            air[i] = 1
        if i < ng and thr == boost and (yaw != 0) == bool(hb):
            air[i] = 1
    return t, ground, air, jumpm, boostm


_TABLE = action_table()


def mask_row(g, p):
    """DefaultAction::GetActionMask(state.players[p], state)."""
    _, ground, air, jumpm, boostm = _TABLE
    c = g["players"][p]["car"]
    res = np.zeros(len(ground), np.uint8)
    res |= ground if c["is_on_ground"] else air
    if F(c["boost"]) == F(0):
        res &= ~boostm & 1
    turtled = bool(c["world_contact_has_contact"]) and F(c["world_contact_normal"][2]) > F(0.9)
    if has_flip_or_jump(c) or turtled:
        res |= jumpm
    return res


def mask_rows(gs, rows=None):
    if rows is None:
        rows = [(a, p) for a in range(len(gs)) for p in range(4)]
    return np.stack([mask_row(gs[a], p) for a, p in rows])

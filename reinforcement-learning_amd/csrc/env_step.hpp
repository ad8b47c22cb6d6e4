// env_step.hpp -- the env kernel (one launch = every arena of the set: StepFirstHalf / StepSecondHalf /
// resets / builders, env_kernel.hpp) and its launch arguments.
//
// Every translation unit that defines RLGPU_ENV_KERNEL (the kernel's name; RLGPU_ENV_COLLECT_KERNEL: the collection
// loop kernel's, at the end of this file) and RLGPU_ENV_ARITH (an
// RLGPU_ARITH_* mode, include/rlgpu_arith.h) gets the kernel specialised for that arithmetic: arith(A) is
// then a constant (env_device.hpp), so the other builds' LinearMath and solver-row branches fold away and
// do not hold registers (env_k0.hip, env_k1.hip, env_k2.hip).  Without RLGPU_ENV_KERNEL only StepArgs and
// ResetMode are declared (env.hip's host code).
#pragma once
#include "env_builders.hpp"

namespace rl {

// StepArgs::reset_mode: what the launch resets after (or instead of) its step
enum ResetMode : int {
    kResetNone = 0,
    kResetTerminated = 1,  // the fused step: arenas whose episode ended this step
    kResetSet = 2,         // EnvSet::Reset: arenas whose terminals[] code is set (and clears it)
    kResetMask = 3,        // ResetArena: arenas of reset_mask (null = all)
    kResetAll = 4,         // every arena (the EnvSet constructor)
    kRebuildObs = 5        // no reset: rebuild the obs / mask rows from the records
};

struct StepArgs {
    char* arenas;
    int n;
    int ticks_first;        // StepFirstHalf ticks (actionDelay), 0 = skip
    const int32_t* actions; // StepSecondHalf actions (null = skip second half)
    int ticks_second;       // tickSkip - actionDelay
    int build;              // run GameState / terminal / reward / obs builders
    int reset_mode;         // a ResetMode
    const uint8_t* reset_mask;
    float* obs;
    uint8_t* masks;
    float* rewards;
    uint8_t* terminals;
    float* last_rewards;
    float* trunc_obs;
    float* out_obs;        // experience append (rlgpu_step_outputs), each may be null
    uint8_t* out_masks;
    float* out_rew;
    int8_t* out_term;
    float* out_trunc;
    int max_episode_steps;
    uint64_t seed;
    unsigned long long* prof;  // [32] phase cycle counters or null
    MeshView mesh;
    double* metrics;           // [n][RLGPU_STEP_METRIC_SLOTS] StepCallback sums (build steps) or null
    int metrics_players;       // this call is one of ExampleMain's every-4th "expensive" calls
    const Plugins* plug;       // the set's reward / terminal registry (device)
    int arith;                 // RLGPU_ARITH_* (rlgpu_envset_config.arith): copied into Aux::arith at launch
    int arena_offset;          // global index of arena 0 (the arenas' Philox streams)
    float* reward_values;      // [players][nr] each reward's value before its weight, or null
    int pen_slots;             // deferred penetration queries whose GJK state is saved (kPenSave; tests: fewer)
};

// The launch arguments of the collection loop kernel (RLGPU_ENV_COLLECT_KERNEL below): the fused step of rollout
// row 0 as launch() fills it -- per step t the kernel moves `actions` and the out_* rows on by t rows of P players --
// and the policy forward of row 0 as infer::InferArgs bytes (ppo.hip fills them; env.hip does not see the type).
struct InferBlob {
    alignas(8) unsigned char b[512];
};
struct CollectArgs {
    StepArgs g;
    int T;             // steps
    int metric_calls;  // the set's StepCallback call counter at launch, mod 4 (step t is call metric_calls + t + 1)
    int64_t P;         // players per rollout row
    InferBlob inf;
    // null, or [workgroups][kSplitSlots] (zeroed by the caller): the launch runs the profiled instantiation, whose
    // workgroups add up where their steps' time went (rlgpu_envset_set_collect_split, tools/collect_loop_split.py)
    unsigned long long* split;
};
// CollectArgs::split, per workgroup: the sum over the T steps, in ticks of the 100 MHz wall clock as the workgroup's
// lane 0 reads it.  forward = staging (the obs and mask rows read back and converted) + the layers and the sampler;
// sync_a = the barrier after the forward (its action stores drain); load = the records staged into LDS up to their
// barrier; body = the env step up to the record write-back; store = the write-back's issue; sync_b = the barrier that
// ends the step (the stores of the step drain).
enum { kSplitStage = 0, kSplitForward, kSplitSyncA, kSplitLoad, kSplitBody, kSplitStore, kSplitSyncB, kSplitSlots = 8 };

#if defined(RLGPU_ENV_KERNEL) || defined(RLGPU_ENV_COLLECT_KERNEL)

// ExampleMain's StepCallback (src/ExampleMain.cpp:233-283) on this arena's GameState as the
// builders left it (after UpdateFromArena, before any reset), Report::AddAvg's fp64 totals kept per
// arena and player: slot RLGPU_SM_* x 4 + player.  Lane l = player l; lane 0 adds the per-state
// goal speed and the arena's count of player passes.  Vec::Length / Normalized / Dot / RS_MAX are
// restated in float (MathTypes.h:31-93, Framework.h:47); the totals are fp64 as Report::Avg.
DEV void step_metrics(ArenaLDS* A, int l, double* m, bool players) {
    if (players) {
        const rlgpu_car& c = A->s.cars[l];
        const v3 pos = ld3(c.body.pos) * kBT2UU, vel = ld3(c.body.vel) * kBT2UU;
        const v3 bp = ld3(A->s.ball.pos) * kBT2UU;
        const bool touched = A->a.touched[l] != 0;
        const v3 dir = rs_norm(bp - pos);
        const float toward = vel.x * dir.x + vel.y * dir.y + vel.z * dir.z;
        m[RLGPU_SM_IN_AIR * 4 + l] += c.is_on_ground ? 0.0 : 1.0;
        m[RLGPU_SM_BALL_TOUCH * 4 + l] += touched ? 1.0 : 0.0;
        m[RLGPU_SM_DEMOED * 4 + l] += c.is_demoed ? 1.0 : 0.0;
        m[RLGPU_SM_SPEED * 4 + l] += (double)rs_len(vel);
        m[RLGPU_SM_SPEED_TO_BALL * 4 + l] += (double)(0.f > toward ? 0.f : toward);
        m[RLGPU_SM_BOOST * 4 + l] += (double)c.boost;
        if (touched) m[RLGPU_SM_TOUCH_HEIGHT * 4 + l] += (double)bp.z;
    }
    if (l == 0) {
        if (players) m[RLGPU_SM_SLOT_PASSES] += 1.0;
        if (A->a.goal) {
            m[RLGPU_SM_SLOT_GOAL_SPEED] += (double)rs_len(ld3(A->s.ball.vel) * kBT2UU);
            m[RLGPU_SM_SLOT_GOALS] += 1.0;
        }
    }
}


// The boost-pad constants a lane tests every tick (pads l, l + 16, l + 32), held in registers for
// the whole launch instead of re-read from the constant buffer with lane-varying addresses in every
// tick's pad-collision phase.
constexpr int kPadsPerLane = (RLGPU_PADS + kTeam - 1) / kTeam;
struct PadRegs {
    int px[kPadsPerLane], py[kPadsPerLane];
    v3 pos[kPadsPerLane], bmin[kPadsPerLane], bmax[kPadsPerLane];
    float rad[kPadsPerLane];
};
DEV void load_pad_regs(PadRegs& R, int l) {
#pragma unroll
    for (int k = 0; k < kPadsPerLane; k++) {
        const int p = l + k * kTeam < RLGPU_PADS ? l + k * kTeam : 0;
        R.px[k] = C.pad_cell_x[p];
        R.py[k] = C.pad_cell_y[p];
        R.pos[k] = C.pad_pos_bt[p];
        R.bmin[k] = C.pad_box_min[p];
        R.bmax[k] = C.pad_box_max[p];
        R.rad[k] = (C.pad_big[p] ? 208.f : 144.f) * kUU2BT;
    }
}

// ------------------------------------------------------------------ one tick (Arena::Step body)
// Inlined into the tick loop.  Inlined, the compiler hoists the launch-invariant
// constant-buffer values of all phases out of the loop (408 VGPR + AGPR, one wave per SIMD);
// called (__noinline__) the kernel needs 248 VGPRs and could run two waves per SIMD, but measured
// slower: 870 -> 938 us per launch at 4 arenas per wave, and 2 arenas per wave (two waves per
// SIMD) 1.7x slower per arena.
DEV void tick(ArenaLDS* A, const MeshView& M, int l, bool valid, uint64_t seed, int arena, Prof& P, const PadRegs& R,
                          int nvalid) {
    if (valid) {  // per body / car on lanes 0-4: independent fields, read before the respawns below write
        rlgpu_arena_state& s = A->s;
        if (l == 0) {
            A->u.wc.njob = 0;  // this tick's wheel-ray cast jobs
            bool sleep = len2(ld3(s.ball.vel)) == 0 && len2(ld3(s.ball.angvel)) == 0;  // Arena.cpp:722-727
            s.ball_sleeping = sleep;
            A->a.ball_sleep = sleep;
            A->a.active[0] = 1;
        } else if (l < 5) {
            const int c = l - 1;
            A->a.active[c + 1] = !s.cars[c].is_demoed;
            float* ctl = s.cars[c].controls;  // CarControls::ClampFix
            for (int k = 0; k < 5; k++) ctl[k] = stdclamp(ctl[k], -1.f, 1.f);
        }
        if (l < 5) {
            A->a.snap_vel[l] = bvel(A, l);
            A->a.snap_ang[l] = bang(A, l);
        }
    }
    sync();
    if (valid && l == 0) {
        rlgpu_arena_state& s = A->s;
        // demo timer / respawn (Car.cpp:66-84), RNG draws in car order
        for (int c = 0; c < 4; c++) {
            rlgpu_car& cs = s.cars[c];
            if (cs.is_demoed) {
                cs.demo_respawn_timer = stdmax(cs.demo_respawn_timer - kTick, 0.f);
                if (cs.demo_respawn_timer == 0.f) {
                    int idx = (int)(rng_next(A, seed, arena) % 4u);
                    bool orange = c & 1;
                    v3 pos = v3{C.respawn_x[idx], C.respawn_y[idx] * (orange ? -1.f : 1.f), 36.f};
                    set_car_state(A, c, pos, C.respawn_rot[orange][idx], 100.f / 3.f, false);
                }
            }
        }
    }
    sync();
    P.mark(0);
    if (valid && !A->s.cars[l >> 2].is_demoed) wheel_phase(A, M, l >> 2, l & 3);
    sync();
    P.mark(1);
    wheel_casts(A - (threadIdx.x >> 4), nvalid);
    sync();
    P.mark(30);
    if (valid && !A->s.cars[l >> 2].is_demoed) wheel_phase_b(A, l >> 2, l & 3);
    sync();
    P.mark(31);
    if (valid && l < 4) car_phase_a(A, l);
    sync();
    P.mark(33);
    // Car::_UpdateWheels' per-wheel friction: lane 4 car + wheel
    if (valid && !A->s.cars[l >> 2].is_demoed) wheel_friction(A, l >> 2, l & 3);
    sync();
    P.mark(34);
    if (valid) {
        if (l < 4) {
            car_phase(A, l);
        } else {
            for (int p = l - 4; p < RLGPU_PADS; p += 12) {  // BoostPad::_PreTickUpdate
                rlgpu_pad& pd = A->s.pads[p];
                if (pd.cooldown > 0) pd.cooldown = stdmax(pd.cooldown - kTick, 0.f);
                pd.is_active = pd.cooldown == 0;
            }
        }
    }
    sync();
    P.mark(2);
    if (valid && l < 5) {  // applyGravity + predictUnconstraintMotion
        add_force(A, l, C.gravity * (l == 0 ? kBallMass : kCarMass));
        if (l == 0) {
            rlgpu_body* b = body(A, 0);
            st3(b->vel, ld3(b->vel) * C.ball_damp);
            st3(b->angvel, ld3(b->angvel) * 1.f);
            A->a.pred_pos[0] = bpos(A, 0) + bvel(A, 0) * kTick;
            A->a.pred_rot[0] = brot(A, 0);
        } else {
            integrate_transform(bpos(A, l), brot(A, l), bvel(A, l), bang(A, l), kTick, A->a.pred_pos[l], A->a.pred_rot[l],
                                arith(A));
        }
    }
    sync();
    P.mark(3);
    if (valid && l < 5) {  // updateAabbs: the broadphase AABB and home cell of body l (one lane per body)
        v3 mn, mx;
        broad_aabb(A, l, mn, mx);
        A->u.bp.mn[l] = mn;
        A->u.bp.mx[l] = mx;
        A->u.bp.cell[l] = bp_home(mn) + 1;
    }
    sync();
    if (valid && l == 0) {
        bp_update(A);  // btRSBroadphase::setAabb in body order
        bool awake = !A->a.ball_sleep;
        if (!awake) {
            const v3 m0 = A->u.bp.mn[0], m1 = A->u.bp.mx[0];
            for (int ci = 1; ci <= 4; ci++) {
                if (!A->a.active[ci]) continue;
                if (aabb_overlap(m0, m1, A->u.bp.mn[ci], A->u.bp.mx[ci])) awake = true;
            }
        }
        A->a.ball_awake = awake;
        A->a.ncand = 0;
        A->a.nq = 0;
    }
    if (threadIdx.x == 0) g_pen_save.n = 0;
    sync();
    P.mark(4);
    if (valid)
        // work items: the 5 body-vs-mesh pairs split into kMeshChunks parts each (the heavy items,
        // spread over distinct lanes first), then the 30 light pairs
        for (int item = l; item < 5 * kMeshChunks + 30; item += kTeam) {
            if (item < 5 * kMeshChunks) {
                narrow_pair(A, M, (item / kMeshChunks) * 5, item % kMeshChunks, kMeshChunks);
            } else {
                int j = item - 5 * kMeshChunks;  // 0..29 -> the plane and dynamic ranks
                narrow_pair(A, M, j < 20 ? (j / 4) * 5 + 1 + (j % 4) : 25 + (j - 20));
            }
        }
    sync();
    P.mark(22);
    narrow_queue(A - (threadIdx.x >> 4), nvalid, M);
    sync();
    P.mark(5);
    narrow_deferred(A - (threadIdx.x >> 4), nvalid, M);
    sync();
    P.mark(18);
    if (valid) sort_candidates(A, l);
    sync();
    if (valid && l == 0) {
        commit_contacts(A, M, &P);
        if (threadIdx.x == 0) P.mark(16);
    }
    sync();
    solve_lanes(A, l, valid, &P);
    sync();
    P.mark(6);
    if (valid && l < 5) {  // integrateTransforms (btDiscreteDynamicsWorld.cpp:889-985)
        bool act = l == 0 ? A->a.ball_awake != 0 : A->a.active[l] != 0;
        if (act) {
            rlgpu_body* b = body(A, l);
            if (l == 0) {
                st3(b->pos, ld3(b->pos) + ld3(b->vel) * kTick);
            } else {
                v3 np;
                m3 nr;
                integrate_transform(ld3(b->pos), ldm(b->rot), ld3(b->vel), ld3(b->angvel), kTick, np, nr, arith(A));
                st3(b->pos, np);
                stm(b->rot, nr);
            }
            update_inertia(A, l);
        }
        A->a.force[l] = zero3();
        A->a.torque[l] = zero3();
    }
    sync();
    P.mark(7);
    if (valid && l < 4) {  // Car::_PostTickUpdate + _FinishPhysicsTick (Car.cpp:133-193)
        rlgpu_car& cs = A->s.cars[l];
        if (!cs.is_demoed) {
            rlgpu_body* b = &cs.body;
            float sp2 = len2(ld3(b->vel) * kBT2UU);
            if (cs.is_supersonic && cs.supersonic_time < 1.f)
                cs.is_supersonic = sp2 >= 2100.f * 2100.f;
            else
                cs.is_supersonic = sp2 >= 2200.f * 2200.f;
            if (cs.is_supersonic)
                cs.supersonic_time += kTick;
            else
                cs.supersonic_time = 0;
            if (cs.car_contact_cooldown > 0) cs.car_contact_cooldown = stdmax(cs.car_contact_cooldown - kTick, 0.f);
            for (int k = 0; k < 8; k++) cs.last_controls[k] = cs.controls[k];
            v3 cache = ld3(cs.vel_impulse_cache);
            v3 v = ld3(b->vel), w = ld3(b->angvel);
            if (!is_zero(cache)) {
                v += cache;
                st3(cs.vel_impulse_cache, zero3());
            }
            const float maxv = 2300.f * kUU2BT;
            if (len2(v) > maxv * maxv) v = bt_normalize(v, arith(A)) * maxv;  // vel.normalized() (Car.cpp:183-186)
            if (len2(w) > 5.5f * 5.5f) w = bt_normalize(w, arith(A)) * 5.5f;
            st3(b->vel, v);
            st3(b->angvel, w);
        }
    }
    sync();
    P.mark(8);
    if (valid) {  // BoostPadGrid::CheckCollision per pad (BoostPadGrid.cpp:5-25, BoostPad.cpp:61-86)
        // per-car eligibility and 3x3 grid-cell window, computed once (not per pad)
        int cx0[4], cx1[4], cy0[4], cy1[4];
        v3 cp[4];
#pragma unroll
        for (int ci = 0; ci < 4; ci++) {
            const rlgpu_car& cs = A->s.cars[ci];
            v3 cpos = ld3(cs.body.pos);
            v3 pos_uu = cpos * kBT2UU;
            cp[ci] = cpos;
            bool ok = !(cs.is_demoed || cs.boost >= 100) && !(pos_uu.z > 95.f + 250.f);
            int ix = (int)(pos_uu.x / 1024 + 4), iy = (int)(pos_uu.y / 1024 + 5);
            cx0[ci] = ok ? (ix - 1 > 0 ? ix - 1 : 0) : 1 << 20;  // empty window when not eligible
            cx1[ci] = ix + 1 < 7 ? ix + 1 : 7;
            cy0[ci] = iy - 1 > 0 ? iy - 1 : 0;
            cy1[ci] = iy + 1 < 9 ? iy + 1 : 9;
        }
#pragma unroll
        for (int k = 0; k < kPadsPerLane; k++) {
            const int p = l + k * kTeam;
            if (p >= RLGPU_PADS) break;
            const int px = R.px[k], py = R.py[k];
            const v3 ppos = R.pos[k];
            const float rad = R.rad[k];
            const uint32_t prev_locked = A->s.pads[p].prev_locked_car_id;
            int locked = -1;
#pragma unroll
            for (int ci = 0; ci < 4; ci++) {
                if (px < cx0[ci] || px > cx1[ci] || py < cy0[ci] || py > cy1[ci]) continue;
                v3 cpos = cp[ci];
                bool col = false;
                if (prev_locked == (uint32_t)(ci + 1)) {
                    v3 mn, mx;
                    body_aabb(ci + 1, cpos, ldm(A->s.cars[ci].body.rot), mn, mx);
                    const v3 bmin = R.bmin[k], bmax = R.bmax[k];
                    col = (bmax.x > mn.x && bmax.y > mn.y && bmax.z > mn.z) && (bmin.x < mx.x && bmin.y < mx.y && bmin.z < mx.z);
                } else {
                    float dx = cpos.x - ppos.x, dy = cpos.y - ppos.y;
                    if (dx * dx + dy * dy < rad * rad) col = fabsf(cpos.z - ppos.z) < (95.f * kUU2BT);
                }
                if (col) locked = ci;
            }
            A->a.locked[p] = locked;
        }
    }
    sync();
    P.mark(9);
    // BoostPad::_PostTickUpdate (BoostPad.cpp:88-105): each pad's own state on the lane that tested it (pads
    // l, l + 16, l + 32), then the pickups' boost in pad order on the arena's lane 0 (a car may pick two pads)
    uint64_t picked[kPadsPerLane];
#pragma unroll
    for (int k = 0; k < kPadsPerLane; k++) {
        const int p = l + k * kTeam;
        bool pick = false;
        if (valid && p < RLGPU_PADS) {
            rlgpu_pad& pd = A->s.pads[p];
            const int lk = A->a.locked[p];
            if (lk >= 0 && pd.is_active) {
                pick = true;
                pd.is_active = 0;
                pd.cooldown = R.rad[k] > 144.f * kUU2BT ? 10.f : 4.f;  // a big pad (pad_big: radius 208)
            }
            pd.prev_locked_car_id = lk >= 0 ? (uint32_t)(lk + 1) : 0u;
        }
        picked[k] = __ballot(pick);
    }
    if (valid && l == 0) {
        const int team = (int)(threadIdx.x >> 4);
#pragma unroll
        for (int k = 0; k < kPadsPerLane; k++)
            for (uint32_t bits = (uint32_t)(picked[k] >> (16 * team)) & 0xffffu; bits; bits &= bits - 1u) {
                const int p = __ffs(bits) - 1 + k * kTeam;
                rlgpu_car& cs = A->s.cars[A->a.locked[p]];
                cs.boost = stdmin(cs.boost + (C.pad_big[p] ? 100.f : 12.f), 100.f);
            }
        rlgpu_body* b = &A->s.ball;  // Ball::_FinishPhysicsTick (Ball.cpp:112-138)
        v3 v = ld3(b->vel), w = ld3(b->angvel);
        v3 cache = ld3(A->s.ball_vel_impulse_cache);
        if (!is_zero(cache)) {
            v += cache;
            st3(A->s.ball_vel_impulse_cache, zero3());
        }
        const float maxv = 6000.f * kUU2BT;
        if (len2(v) > maxv * maxv) v = bt_normalize(v, arith(A)) * maxv;  // vel.normalized() (Ball.cpp:128-131)
        if (len2(w) > 6.f * 6.f) w = bt_normalize(w, arith(A)) * 6.f;
        st3(b->vel, v);
        st3(b->angvel, w);
        A->s.env.tick_count++;
    }
    sync();
    P.mark(10);
}

// copy the 4 obs rows (and mask rows) of this arena from LDS to [players x obs_w] outputs (the rows are packed at the
// set's width in LDS too: one contiguous copy)
DEV void copy_rows(ArenaLDS* A, const Plugins* B, int l, int arena, float* obs, uint8_t* masks) {
    if (obs) {
        const int w4 = 4 * B->obs_w;
        const float* src = &A->u.out.obs[0][0];
        float* dst = obs + (size_t)arena * w4;
        for (int k = l; k < w4; k += kTeam) dst[k] = src[k];
    }
    if (masks) {
        const uint8_t* msrc = &A->u.out.masks[0][0];
        uint8_t* mdst = masks + (size_t)arena * 4 * RLGPU_ACTIONS;
        for (int k = l; k < 4 * RLGPU_ACTIONS; k += kTeam) mdst[k] = msrc[k];
    }
}

#ifdef RLGPU_ENV_KERNEL
#define RLGPU_BODY_STAMP(k)
__global__ void __launch_bounds__(kWG) RLGPU_ENV_KERNEL(StepArgs g) {
    __shared__ ArenaLDS lds[kArenas];
#include "env_step_body.inc"
}
#undef RLGPU_BODY_STAMP
#endif

#ifdef RLGPU_ENV_COLLECT_KERNEL
// The collection loop: one launch collects the whole rollout.  A workgroup owns its kArenas arenas and their 16
// player rows for all T steps and never waits for another workgroup: per step it runs the policy forward of its own
// rows of rollout row t on its one wave (infer::wave_infer, the fused inference kernel's arithmetic; the unit that
// defines RLGPU_ENV_COLLECT_KERNEL, env_collect_k0.hip, includes infer_kernels.hpp first), then the env step of its
// arenas (env_step_body.inc), which appends row t + 1.  What a step reads was written by this workgroup (its rows of the rollout, its records) or is
// constant during the launch (weights, mesh), so the steps of different workgroups need no order among them.  The
// inference buffers alias the arena staging area: between two steps the records are in HBM.
//
// The forward and the step body are functions of their own.  Between two steps almost nothing is live, so a call there
// costs little, and a called function gets a register allocation of its own: inlined into one loop, the body's
// launch-invariant values stay in registers across the forward and the forward's weight fragments across the body,
// and the kernel spills (profiles/collect_loop_codegen.txt).  RLGPU_COLLECT_CALLS says which
// of the two are called (bit 0: the forward, bit 1: the body), RLGPU_COLLECT_BATCH whether the forward stages its rows
// with batched loads (infer::wave_infer); the defaults are what measured best, the command line may set others.
// A called function reads the launch arguments where the kernel does, in the kernel argument segment (CollectArgs is
// the kernel's only parameter, so it starts the segment: collect_args), and the staging area by its name: both keep
// their address spaces, which a pointer parameter would lose.
#ifndef RLGPU_COLLECT_CALLS
#define RLGPU_COLLECT_CALLS 3
#endif
#ifndef RLGPU_COLLECT_BATCH
#define RLGPU_COLLECT_BATCH 1
#endif
#ifndef RLGPU_COLLECT_FN_ATTR  // further attributes of the called functions
#define RLGPU_COLLECT_FN_ATTR
#endif
#if RLGPU_COLLECT_CALLS & 1
#define RLGPU_COLLECT_FWD __device__ __noinline__ RLGPU_COLLECT_FN_ATTR
#else
#define RLGPU_COLLECT_FWD DEV
#endif
#if RLGPU_COLLECT_CALLS & 2
#define RLGPU_COLLECT_BODY __device__ __noinline__ RLGPU_COLLECT_FN_ATTR
#else
#define RLGPU_COLLECT_BODY DEV
#endif

static __shared__ ArenaLDS g_collect_lds[kArenas];
// The launch arguments as a called function finds them.  The kernel argument segment's own address is null inside a
// called function (only kernels get it); the address of the implicit arguments is passed on, and they follow the
// explicit ones at the next multiple of 8 bytes.
static_assert(sizeof(CollectArgs) % 8 == 0, "the implicit kernel arguments start where CollectArgs ends");
DEV const CollectArgs& collect_args() {
    typedef const __attribute__((address_space(4))) char* KernargBytes;
    return *(const CollectArgs*)((KernargBytes)__builtin_amdgcn_implicitarg_ptr() - sizeof(CollectArgs));
}

// The profiled instantiation's clock (CollectArgs::split): mark(k) adds the time since the previous mark to the
// workgroup's slot k.  An add that returns nothing: the wave does not wait for it.  The default instantiation's clock
// is empty: it holds nothing, is passed in no register and leaves no instruction.
template <bool ON>
struct SplitClock;
template <>
struct SplitClock<false> {
    static constexpr bool kOn = false;
    DEV void mark(int) {}
};
template <>
struct SplitClock<true> {
    static constexpr bool kOn = true;
    unsigned long long* slot;
    unsigned long long last;
    DEV void mark(int k) {
        const unsigned long long now = wall_clock64();
        if (threadIdx.x == 0) atomicAdd(slot + k, now - last);
        last = wall_clock64();
    }
};

// step t's policy forward of the workgroup's rows of rollout row t
template <bool F16, bool SPLIT>
RLGPU_COLLECT_FWD SplitClock<SPLIT> collect_forward(int t, SplitClock<SPLIT> clk) {
    const CollectArgs& c = collect_args();
    const infer::InferArgs& a = *reinterpret_cast<const infer::InferArgs*>(c.inf.b);
    infer::WaveLDS& S = *reinterpret_cast<infer::WaveLDS*>(g_collect_lds);
    const int64_t P = c.P, r0 = (int64_t)blockIdx.x * infer::WR;
    const int rows = (int)(P - r0 < infer::WR ? P - r0 : infer::WR), A = a.width[a.nl];
    const int64_t row = (int64_t)t * P + r0;  // this workgroup's first row of rollout row t
    // rows of t > 0 were stored by this workgroup in the previous trip: the barrier that ended it made them visible
    infer::wave_infer<F16, mlp::ACT_LEAKY, RLGPU_COLLECT_BATCH != 0>(a, S, a.X + row * a.in, a.masks + row * A, rows, a.row0 + r0,
                                                                a.step + t, a.row_sel ? a.row_sel + r0 : nullptr, a.act + row,
                                                                a.logp ? a.logp + row : nullptr, nullptr, (int)threadIdx.x, &clk);
    clk.mark(kSplitForward);
    return clk;
}

// step t's env step of the workgroup's arenas, which appends rollout row t + 1
template <bool SPLIT>
RLGPU_COLLECT_BODY SplitClock<SPLIT> collect_body(int t, SplitClock<SPLIT> clk) {
    const CollectArgs& c = collect_args();
    ArenaLDS(&lds)[kArenas] = g_collect_lds;
    StepArgs s = c.g;
    const int64_t tp = (int64_t)t * c.P;
    s.actions = c.g.actions + tp;
    if (s.out_obs) s.out_obs = c.g.out_obs + tp * c.g.plug->obs_w;
    if (s.out_masks) s.out_masks = c.g.out_masks + tp * RLGPU_ACTIONS;
    if (s.out_rew) s.out_rew = c.g.out_rew + tp;
    if (s.out_term) s.out_term = c.g.out_term + tp;
    if (s.out_trunc) s.out_trunc = c.g.out_trunc + tp * c.g.plug->obs_w;
    // ExampleMain's every-4th-call flag: the set's call counter at launch plus this step (env.hip launch())
    if (s.metrics) s.metrics_players = (c.metric_calls + t + 1) % 4 == 0;
#define RLGPU_BODY_STAMP(k) clk.mark(k);
    {
        const StepArgs& g = s;
#include "env_step_body.inc"
    }
#undef RLGPU_BODY_STAMP
    clk.mark(kSplitStore);
    return clk;
}

template <bool F16, bool SPLIT>
__global__ void __launch_bounds__(kWG) RLGPU_ENV_COLLECT_KERNEL(CollectArgs c) {
    static_assert(sizeof(infer::WaveLDS) <= sizeof(ArenaLDS) * kArenas, "the inference buffers fit the arena staging area");
    static_assert(sizeof(infer::InferArgs) <= sizeof(c.inf) && alignof(infer::InferArgs) <= alignof(InferBlob), "InferBlob");
    static_assert(infer::WR == 4 * kArenas, "a workgroup's players are one wave's rows");
    SplitClock<SPLIT> clk;
    if constexpr (SPLIT) {
        clk.slot = c.split + (size_t)blockIdx.x * kSplitSlots;
        clk.last = wall_clock64();
    }
    for (int t = 0; t < c.T; t++) {
        clk = collect_forward<F16, SPLIT>(t, clk);
        sync();  // the actions are stored (the step reads them back), the inference buffers are free
        clk.mark(kSplitSyncA);
        clk = collect_body<SPLIT>(t, clk);
        sync();  // the records and the rollout rows are stored; the staging area is free for the next forward
        clk.mark(kSplitSyncB);
    }
}
#endif  // RLGPU_ENV_COLLECT_KERNEL
#endif  // RLGPU_ENV_KERNEL || RLGPU_ENV_COLLECT_KERNEL

}  // namespace rl

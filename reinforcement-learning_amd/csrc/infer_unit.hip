// infer_unit.hip -- deployment inference (include/rlgpu_infer_unit.h, GGL::InferUnit): from host GameState records
// to parsed actions.  Two kernels:
//   iu::gs_rows        the obs rows and DefaultAction masks of (state, player) pairs, to device arrays;
//   iu::gs_infer_wave  one launch per call (on request, rlgpu_infer_unit_set_one_launch): a 64-lane workgroup builds
//                      up to 16 rows and masks into LDS, runs infer::wave_infer on them (the collection loop's one-wave forward, unchanged) and writes the
//                      action index, the log prob and DefaultAction's table row of each.
// A row's elements are the env kernel's expressions (env_builders.hpp: PView, add_player_obs,
// add_player_default_obs, inv_if) on a PView filled from the record instead of the arena; the unit is compiled
// without FMA contraction like the env kernel, so the rows are the env set's bit for bit.  The policy forward is
// compiled as in ppo.hip, contraction on (env_collect_k0.hip's arrangement).
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rlgpu_detmath.h"
#include "../../include/rlgpu_infer_unit.h"
#include "common.hpp"
#pragma clang fp contract(fast)
namespace {
#include "infer_kernels.hpp"
}
#pragma clang fp contract(off)
#include "env_builders.hpp"

namespace iu {
using rl::PView;
using rl::Plugins;
using rl::v3;

struct Args {
    const rlgpu_gamestate* states;
    const int32_t* state_of_row;   // [n]
    const int32_t* player_of_row;  // [n]
    int n;
    int64_t row0;                  // the global number of row 0: DefaultObsPadded's shuffle stream, the sampler's row
    const Plugins* B;              // the obs builder (obs_* fields)
    const uint8_t* mask_bits;      // [RLGPU_ACTIONS] EnvConst::mask_bits
    const float* table;            // [RLGPU_ACTIONS][8] DefaultAction's table
    float* obs;                    // gs_rows: [n][obs_w]
    uint8_t* masks;                // gs_rows: [n][RLGPU_ACTIONS]
    int32_t* act;                  // [n]
    float* logp;                   // [n]
    float* actions;                // [n][8]
};

// Player::UpdateFromCar's fields as the builders read them (rl::view_player on the record): pos / vel are uu already
// (host/gamestate.cpp's fp32 x 50), rot's rows are forward, right, up, the side is the player's team
DEV PView view_player_gs(const rlgpu_player_state& p) {
    const rlgpu_car_state& c = p.car;
    PView v;
    v.pos = rl::ld3(c.pos);
    v.vel = rl::ld3(c.vel);
    v.ang = rl::ld3(c.ang_vel);
    v.fwd = rl::ld3(c.rot);
    v.right = rl::ld3(c.rot + 3);
    v.up = rl::ld3(c.rot + 6);
    v.boost = c.boost;
    v.on_ground = c.is_on_ground;
    v.hfj = c.is_on_ground || (!c.has_flipped && !c.has_double_jumped && c.air_time_since_jump < 1.25f);  // Car.cpp:279-283
    v.demoed = c.is_demoed;
    v.has_jumped = c.has_jumped;
    v.is_flipping = c.is_flipping;
    v.orange = p.team != 0;
    v.world_contact = c.world_contact_has_contact;
    v.wc_z = c.world_contact_normal[2];
    return v;
}

// The obs rows (stride B->obs_w) and masks (stride RLGPU_ACTIONS) of rows [r0, r0 + rows), rows <= 16, on the 64 lanes
// of a workgroup: lane 4 r + j writes row r's player block j (self, teammate, first opponent, second opponent in
// state.players order); the head, the pads and the mask bytes are strided over the lanes, as advanced_obs_rows /
// default_obs_rows deal them over an arena's 16.
DEV void build_rows(const Args& u, int r0, int rows, float* obs, uint8_t* masks, int l) {
    const Plugins* B = u.B;
    const int w = B->obs_w, kind = B->obs_kind, mp = B->obs_max_players;
    if ((l >> 2) < rows) {
        const int r = l >> 2, j = l & 3, i = r0 + r;
        const rlgpu_gamestate& g = u.states[u.state_of_row[i]];
        const int me = u.player_of_row[i];
        const int team = g.players[me].team;
        const uint32_t id = g.players[me].car_id;
        const bool inv = team == 1;
        int mate = me, opp0 = -1, opp1 = me;  // two per team (checked on the host)
        for (int q = 0; q < RLGPU_CARS; q++) {
            if (g.players[q].car_id == id) continue;
            if (g.players[q].team == team) mate = q;
            else if (opp0 < 0) opp0 = q;
            else opp1 = q;
        }
        if (opp0 < 0) opp0 = me;
        const int who = j == 0 ? me : (j == 1 ? mate : (j == 2 ? opp0 : opp1));
        const PView pv = view_player_gs(g.players[who]);
        float* o = obs + r * w + 51;
        if (kind == RLGPU_OBS_ADVANCED) {
            const v3 bp = rl::inv_if(rl::ld3(g.ball.pos), inv), bv = rl::inv_if(rl::ld3(g.ball.vel), inv);
            rl::add_player_obs(o + 29 * j, pv, inv, bp, bv);
        } else {
            // the row's two lists after DefaultObsPadded's shuffles (default_obs_rows): the
            // draws are a function of (key, the row's global number, the state's tick count, draw index)
            int t0 = 0, o0 = 0, o1 = 1;
            if (kind == RLGPU_OBS_DEFAULT_PADDED) {
                const uint64_t key = (uint64_t)B->obs_key[0] | (uint64_t)B->obs_key[1] << 32;
                const uint32_t c0 = (uint32_t)(u.row0 + i), c1 = (uint32_t)g.last_tick_count << 2;
                if (mp == 3) {
                    if ((((uint64_t)rl::philox0(key, c0, c1 | 0u) * 2u) >> 32) == 0) t0 = 1;  // i = 1
                    const int s = (int)(((uint64_t)rl::philox0(key, c0, c1 | 1u) * 3u) >> 32);  // i = 2
                    if (s == 0) o0 = 2;
                    if (s == 1) o1 = 2;
                }
                if ((((uint64_t)rl::philox0(key, c0, c1 | 2u) * 2u) >> 32) == 0) {  // i = 1
                    const int t = o0;
                    o0 = o1;
                    o1 = t;
                }
            }
            int slot = 0;  // the block's 19-float slot after the head: self, teammates, opponents
            if (j == 1) slot = 1 + (t0 == 0 ? 0 : 1);
            if (j >= 2) slot = mp + (o0 == j - 2 ? 0 : (o1 == j - 2 ? 1 : 2));
            rl::add_player_default_obs(o + 19 * slot, pv, inv, B);
            if (mp == 3 && j < 2) {  // the lists' zero blocks: lane j = 0 the teammates', j = 1 the opponents'
                const int z = j == 0 ? 1 + (t0 == 1 ? 0 : 1) : mp + (o0 == 2 ? 0 : (o1 == 2 ? 1 : 2));
                float* zo = o + 19 * z;
                for (int k = 0; k < 19; k++) zo[k] = 0.f;
            }
        }
    }
    // ball (AdvancedObs.h:10-13 scales / DefaultObs's coefficients) and previous action: rows x 17 elements
    for (int e = l; e < rows * 17; e += 64) {
        const int r = e / 17, k = e - 17 * (e / 17), i = r0 + r;
        const rlgpu_gamestate& g = u.states[u.state_of_row[i]];
        const rlgpu_player_state& p = g.players[u.player_of_row[i]];
        float* o = obs + r * w;
        if (k < 9) {
            const int q = k / 3, c = k - 3 * (k / 3);  // q: position, velocity, angular velocity
            const float* src = q == 0 ? g.ball.pos : (q == 1 ? g.ball.vel : g.ball.ang_vel);
            float x = src[c];
            if (p.team == 1 && c < 2) x = -x;  // inv_if
            float sc;
            if (kind == RLGPU_OBS_ADVANCED) sc = q == 0 ? 1 / 5000.f : (q == 1 ? 1 / 2300.f : 1 / 3.f);
            else sc = q == 0 ? B->obs_pos_coef[c] : (q == 1 ? B->obs_vel_coef : B->obs_ang_vel_coef);
            o[k] = x * sc;
        } else {
            o[k] = p.prev_action[k - 9];
        }
    }
    // boost pads: rows x 34 elements.  GetBoostPadTimers(inverted) returns the opposite array (GameState.h:60)
    for (int e = l; e < rows * RLGPU_PADS; e += 64) {
        const int r = e / RLGPU_PADS, k = e - RLGPU_PADS * (e / RLGPU_PADS), i = r0 + r;
        const rlgpu_gamestate& g = u.states[u.state_of_row[i]];
        const bool inv = g.players[u.player_of_row[i]].team == 1;
        const bool active = (inv ? g.boost_pads_inv[k] : g.boost_pads[k]) != 0;
        float x;
        if (kind == RLGPU_OBS_ADVANCED) {
            const float timer = inv ? g.boost_pad_timers[k] : g.boost_pad_timers_inv[k];
            x = active ? 1.0f : 1.0f / (1.0f + timer);
        } else {
            x = active ? 1.0f : 0.0f;
        }
        obs[r * w + 17 + k] = x;
    }
    // DefaultAction::GetActionMask: rows x 90 bytes, action_mask_rows' rule on the record's flags
    for (int e = l; e < rows * RLGPU_ACTIONS; e += 64) {
        const int r = e / RLGPU_ACTIONS, k = e - RLGPU_ACTIONS * (e / RLGPU_ACTIONS), i = r0 + r;
        const rlgpu_car_state& c = u.states[u.state_of_row[i]].players[u.player_of_row[i]].car;
        const bool hfj = c.is_on_ground || (!c.has_flipped && !c.has_double_jumped && c.air_time_since_jump < 1.25f);
        const bool turtled = c.world_contact_has_contact && c.world_contact_normal[2] > 0.9f;
        const uint32_t f = (c.is_on_ground ? 1 : 0) | (c.boost == 0 ? 2 : 0) | ((hfj || turtled) ? 4 : 0);
        const uint32_t bits = u.mask_bits[k];
        uint32_t m = (f & 1) ? (bits & 1) : ((bits >> 1) & 1);  // ground / air table
        if (f & 2) m &= ~(bits >> 3);                           // no boost: the boost actions off
        if (f & 4) m |= (bits >> 2) & 1;                         // can jump (or turtled): the jump actions on
        masks[r * RLGPU_ACTIONS + k] = (uint8_t)(m & 1);
    }
}

__global__ void __launch_bounds__(64) gs_rows(Args u) {
    const int r0 = blockIdx.x * infer::WR, rows = min(infer::WR, u.n - r0);
    build_rows(u, r0, rows, u.obs + (int64_t)r0 * u.B->obs_w, u.masks + (int64_t)r0 * RLGPU_ACTIONS, (int)threadIdx.x);
}

// ActionParser::ParseAction of DefaultAction: the table row of each index
__global__ void parse_actions(Args u) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < u.n * 8) u.actions[e] = u.table[u.act[e >> 3] * 8 + (e & 7)];
}

template <bool F16>
__global__ void __launch_bounds__(64) gs_infer_wave(Args u, infer::InferArgs a) {
    __shared__ infer::WaveLDS S;
    __shared__ float X[infer::WR * RLGPU_OBS];
    __shared__ uint8_t M[infer::WR * RLGPU_ACTIONS];
    __shared__ int32_t act[infer::WR];
    __shared__ float logp[infer::WR];
    const int l = (int)threadIdx.x, r0 = blockIdx.x * infer::WR, rows = min(infer::WR, u.n - r0);
    build_rows(u, r0, rows, X, M, l);
    __syncthreads();
    // a.row0 is the handle's sample_row_offset (ppo_wave_args' rows start there)
    infer::wave_infer<F16, mlp::ACT_LEAKY>(a, S, X, M, rows, a.row0 + u.row0 + r0, a.step, nullptr, act, logp, nullptr, l);
    __syncthreads();
    for (int e = l; e < rows * 8; e += 64) u.actions[(int64_t)r0 * 8 + e] = u.table[act[e >> 3] * 8 + (e & 7)];
    if (l < rows) {
        u.act[r0 + l] = act[l];
        u.logp[r0 + l] = logp[l];
    }
}

}  // namespace iu

// ------------------------------------------------------------------ C ABI
// Ownership: the tables and the builder record are made by create and live as long as the unit; the staging buffers
// (one device input block, one device output block, the two-step path's row buffers, one pinned host block each way)
// grow on demand.  Device memory goes through rlgpu::dev_alloc / dev_free; free_unit is the only way a unit dies.
struct rlgpu_infer_unit {
    rlgpu_ppo* policy = nullptr;
    bool want_one_launch = false;  // rlgpu_infer_unit_set_one_launch
    rl::Plugins plugins{};
    rl::Plugins* d_plugins = nullptr;
    uint8_t* d_mask_bits = nullptr;
    float* d_table = nullptr;
    char* d_in = nullptr;    // states | state_of_row | player_of_row
    size_t in_cap = 0;
    char* d_out = nullptr;   // act | logp | actions
    size_t out_cap = 0;
    float* d_obs = nullptr;  // two-step path
    uint8_t* d_masks = nullptr;
    size_t rows_cap = 0;
    char* h_in = nullptr;    // pinned
    size_t h_in_cap = 0;
    char* h_out = nullptr;   // pinned
    size_t h_out_cap = 0;
};

namespace {

void free_unit(rlgpu_infer_unit* u) {
    if (!u) return;
    for (void* p : {(void*)u->d_plugins, (void*)u->d_mask_bits, (void*)u->d_table, (void*)u->d_in, (void*)u->d_out,
                    (void*)u->d_obs, (void*)u->d_masks})
        rlgpu::dev_free(p);
    if (u->h_in) (void)hipHostFree(u->h_in);
    if (u->h_out) (void)hipHostFree(u->h_out);
    delete u;
}

template <class T>
void grow_dev(T*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return;
    rlgpu::dev_free(p);
    p = nullptr;
    cap = 0;
    p = static_cast<T*>(rlgpu::dev_alloc(bytes));
    cap = bytes;
}
void grow_pinned(char*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return;
    if (p) RLGPU_CHECK_HIP(hipHostFree(p));
    p = nullptr;
    cap = 0;
    RLGPU_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&p), bytes, hipHostMallocDefault));
    cap = bytes;
}
size_t round_up(size_t b) { return (b + 4095) / 4096 * 4096; }

void check_rows(const char* fn, const rlgpu_gamestate* st, int32_t n_states, const int32_t* sor, const int32_t* por, int32_t n) {
    const std::string f = std::string(fn) + ": ";
    RLGPU_REQUIRE(n > 0, f + "n must be > 0, got " + std::to_string(n));
    RLGPU_REQUIRE(n <= (1 << 24), f + "n = " + std::to_string(n) + " rows in one call (at most 2^24)");
    RLGPU_REQUIRE(n_states > 0, f + "n_states must be > 0, got " + std::to_string(n_states));
    RLGPU_REQUIRE(st && sor && por, f + "null argument");
    for (int32_t s = 0; s < n_states; s++) {
        int per_team[2] = {0, 0};
        for (int p = 0; p < RLGPU_CARS; p++) {
            const int t = st[s].players[p].team;
            RLGPU_REQUIRE(t == 0 || t == 1, f + "state " + std::to_string(s) + ": player " + std::to_string(p) + " has team " +
                                                std::to_string(t) + " (0 blue, 1 orange)");
            per_team[t]++;
            for (int q = 0; q < p; q++)
                RLGPU_REQUIRE(st[s].players[q].car_id != st[s].players[p].car_id,
                              f + "state " + std::to_string(s) + ": players " + std::to_string(q) + " and " + std::to_string(p) +
                                  " share car_id " + std::to_string(st[s].players[p].car_id) + " (duplicate car_id)");
        }
        RLGPU_REQUIRE(per_team[0] == 2, f + "state " + std::to_string(s) + " has " + std::to_string(per_team[0]) + " blue and " +
                                            std::to_string(per_team[1]) + " orange players: two per team (2v2) only");
    }
    for (int32_t i = 0; i < n; i++) {
        RLGPU_REQUIRE(sor[i] >= 0 && sor[i] < n_states, f + "state_of_row[" + std::to_string(i) + "] = " + std::to_string(sor[i]) +
                                                            " is outside the " + std::to_string(n_states) + " states");
        RLGPU_REQUIRE(por[i] >= 0 && por[i] < RLGPU_CARS,
                      f + "player_of_row[" + std::to_string(i) + "] = " + std::to_string(por[i]) + " is outside 0..3");
    }
}

bool one_launch(const rlgpu_infer_unit* u) { return u->want_one_launch && rlgpu_ppo_wave_infer(u->policy, 0) != 0; }

// stage the call's inputs and enqueue their upload; returns the kernels' arguments (outputs unset)
iu::Args upload(rlgpu_infer_unit* u, const rlgpu_gamestate* st, int32_t n_states, const int32_t* sor, const int32_t* por, int32_t n,
                int64_t row0, hipStream_t s) {
    const size_t sb = (size_t)n_states * sizeof(rlgpu_gamestate), ib = (size_t)n * sizeof(int32_t), total = sb + 2 * ib;
    grow_pinned(u->h_in, u->h_in_cap, round_up(total));
    grow_dev(u->d_in, u->in_cap, round_up(total));
    std::memcpy(u->h_in, st, sb);
    std::memcpy(u->h_in + sb, sor, ib);
    std::memcpy(u->h_in + sb + ib, por, ib);
    RLGPU_CHECK_HIP(hipMemcpyAsync(u->d_in, u->h_in, total, hipMemcpyHostToDevice, s));
    iu::Args a{};
    a.states = reinterpret_cast<const rlgpu_gamestate*>(u->d_in);
    a.state_of_row = reinterpret_cast<const int32_t*>(u->d_in + sb);
    a.player_of_row = reinterpret_cast<const int32_t*>(u->d_in + sb + ib);
    a.n = n;
    a.row0 = row0;
    a.B = u->d_plugins;
    a.mask_bits = u->d_mask_bits;
    a.table = u->d_table;
    return a;
}

}  // namespace

extern "C" int rlgpu_infer_unit_config_size(void) { return (int)sizeof(rlgpu_infer_unit_config); }

extern "C" int rlgpu_infer_unit_create(const rlgpu_infer_unit_config* cfg, rlgpu_ppo* policy, rlgpu_infer_unit** out) {
    rlgpu_infer_unit* u = nullptr;
    const int rc = rlgpu::guarded([&] {
        RLGPU_REQUIRE(cfg && policy && out, "rlgpu_infer_unit_create: null argument");
        u = new rlgpu_infer_unit;
        u->policy = policy;
        // the builder, validated as rlgpu_envset_create validates it (unknown builder / maxPlayers: RLGPU_ERR_UNSUPPORTED)
        rlgpu::obs_builder_plugins(cfg->obs_builder, cfg->obs_max_players, cfg->obs_pos_coef, cfg->obs_vel_coef,
                                   cfg->obs_ang_vel_coef, cfg->obs_seed, &u->plugins);
        int obs = 0, actions = 0;
        rlgpu::ppo_widths(policy, &obs, &actions);
        RLGPU_REQUIRE(u->plugins.obs_w == obs, "rlgpu_infer_unit_create: the obs builder makes rows of " +
                                                   std::to_string(u->plugins.obs_w) + " floats and the policy handle's obs_size is " +
                                                   std::to_string(obs));
        RLGPU_REQUIRE(actions == RLGPU_ACTIONS, "rlgpu_infer_unit_create: the policy handle's num_actions is " + std::to_string(actions) +
                                                    " and DefaultAction has " + std::to_string(RLGPU_ACTIONS));
        float table[RLGPU_ACTIONS][8];
        uint8_t bits[RLGPU_ACTIONS];
        rlgpu::default_action_tables(&table[0][0], bits);
        u->d_plugins = static_cast<rl::Plugins*>(rlgpu::dev_alloc(sizeof(rl::Plugins)));
        u->d_mask_bits = static_cast<uint8_t*>(rlgpu::dev_alloc(sizeof bits));
        u->d_table = static_cast<float*>(rlgpu::dev_alloc(sizeof table));
        RLGPU_CHECK_HIP(hipMemcpy(u->d_plugins, &u->plugins, sizeof(rl::Plugins), hipMemcpyHostToDevice));
        RLGPU_CHECK_HIP(hipMemcpy(u->d_mask_bits, bits, sizeof bits, hipMemcpyHostToDevice));
        RLGPU_CHECK_HIP(hipMemcpy(u->d_table, table, sizeof table, hipMemcpyHostToDevice));
        *out = u;
    });
    if (rc != RLGPU_OK) free_unit(u);
    return rc;
}

extern "C" int rlgpu_infer_unit_destroy(rlgpu_infer_unit* u) {
    return rlgpu::guarded([&] { free_unit(u); });
}

extern "C" int rlgpu_infer_unit_obs_size(rlgpu_infer_unit* u) { return u ? u->plugins.obs_w : -1; }

extern "C" int rlgpu_infer_unit_set_one_launch(rlgpu_infer_unit* u, int32_t on) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(u, "rlgpu_infer_unit_set_one_launch: null unit");
        u->want_one_launch = on != 0;
    });
}

extern "C" int rlgpu_infer_unit_one_launch(rlgpu_infer_unit* u) { return u && one_launch(u); }

extern "C" int rlgpu_infer_unit_check_rows(const rlgpu_gamestate* h_states, int32_t n_states, const int32_t* h_state_of_row,
                                           const int32_t* h_player_of_row, int32_t n) {
    return rlgpu::guarded([&] { check_rows("rlgpu_infer_unit_check_rows", h_states, n_states, h_state_of_row, h_player_of_row, n); });
}

extern "C" int rlgpu_infer_unit_build_rows(rlgpu_infer_unit* u, const rlgpu_gamestate* h_states, int32_t n_states,
                                           const int32_t* h_state_of_row, const int32_t* h_player_of_row, int32_t n, int64_t row0,
                                           float* d_obs, uint8_t* d_masks, void* stream) {
    return rlgpu::guarded([&] {
        check_rows("rlgpu_infer_unit_build_rows", h_states, n_states, h_state_of_row, h_player_of_row, n);
        RLGPU_REQUIRE(row0 >= 0, "rlgpu_infer_unit_build_rows: row0 must be >= 0");
        RLGPU_REQUIRE(u && d_obs && d_masks, "rlgpu_infer_unit_build_rows: null argument");
        hipStream_t s = rlgpu::as_stream(stream);
        iu::Args a = upload(u, h_states, n_states, h_state_of_row, h_player_of_row, n, row0, s);
        a.obs = d_obs;
        a.masks = d_masks;
        hipLaunchKernelGGL(iu::gs_rows, dim3(rlgpu::ceil_div(n, infer::WR)), dim3(64), 0, s, a);
        RLGPU_CHECK_HIP(hipGetLastError());
        RLGPU_CHECK_HIP(hipStreamSynchronize(s));  // the pinned block is free for the next call
    });
}

extern "C" int rlgpu_infer_unit_infer(rlgpu_infer_unit* u, const rlgpu_gamestate* h_states, int32_t n_states,
                                      const int32_t* h_state_of_row, const int32_t* h_player_of_row, int32_t n, int64_t row0,
                                      int32_t deterministic, float temperature, uint64_t rng_step, int32_t* h_action_index,
                                      float* h_logp, float* h_actions, void* stream) {
    return rlgpu::guarded([&] {
        RLGPU_REQUIRE(std::isfinite(temperature) && temperature > 0.f,
                      "rlgpu_infer_unit_infer: temperature must be finite and > 0, got " + std::to_string(temperature));
        check_rows("rlgpu_infer_unit_infer", h_states, n_states, h_state_of_row, h_player_of_row, n);
        RLGPU_REQUIRE(row0 >= 0, "rlgpu_infer_unit_infer: row0 must be >= 0");
        RLGPU_REQUIRE(u && h_action_index && h_actions, "rlgpu_infer_unit_infer: null argument");
        hipStream_t s = rlgpu::as_stream(stream);
        iu::Args a = upload(u, h_states, n_states, h_state_of_row, h_player_of_row, n, row0, s);
        const size_t ab = (size_t)n * sizeof(int32_t), lb = (size_t)n * sizeof(float), total = ab + lb + 8 * lb;
        grow_dev(u->d_out, u->out_cap, round_up(total));
        grow_pinned(u->h_out, u->h_out_cap, round_up(total));
        a.act = reinterpret_cast<int32_t*>(u->d_out);
        a.logp = reinterpret_cast<float*>(u->d_out + ab);
        a.actions = reinterpret_cast<float*>(u->d_out + ab + lb);
        if (one_launch(u)) {
            infer::InferArgs ia;
            bool f16 = false;
            rlgpu::ppo_wave_args(u->policy, nullptr, nullptr, n, deterministic, rng_step, nullptr, nullptr, &ia, sizeof ia, &f16);
            ia.temp = temperature;
            const dim3 grid(rlgpu::ceil_div(n, infer::WR));
            if (f16) hipLaunchKernelGGL(iu::gs_infer_wave<true>, grid, dim3(64), 0, s, a, ia);
            else hipLaunchKernelGGL(iu::gs_infer_wave<false>, grid, dim3(64), 0, s, a, ia);
            RLGPU_CHECK_HIP(hipGetLastError());
        } else {
            const size_t w = (size_t)u->plugins.obs_w;
            if ((size_t)n > u->rows_cap) {  // both row buffers, or neither
                size_t c0 = 0, c1 = 0;
                const size_t want = ((size_t)n + 63) / 64 * 64;
                rlgpu::dev_free(u->d_obs);
                rlgpu::dev_free(u->d_masks);
                u->d_obs = nullptr;
                u->d_masks = nullptr;
                u->rows_cap = 0;
                grow_dev(u->d_obs, c0, want * w * sizeof(float));
                grow_dev(u->d_masks, c1, want * RLGPU_ACTIONS);
                u->rows_cap = want;
            }
            a.obs = u->d_obs;
            a.masks = u->d_masks;
            hipLaunchKernelGGL(iu::gs_rows, dim3(rlgpu::ceil_div(n, infer::WR)), dim3(64), 0, s, a);
            RLGPU_CHECK_HIP(hipGetLastError());
            rlgpu::ppo_infer_actions_temp(u->policy, a.obs, a.masks, n, row0, deterministic, temperature, rng_step, a.act, a.logp, s);
            hipLaunchKernelGGL(iu::parse_actions, dim3(rlgpu::ceil_div((int64_t)n * 8, 256)), dim3(256), 0, s, a);
            RLGPU_CHECK_HIP(hipGetLastError());
        }
        RLGPU_CHECK_HIP(hipMemcpyAsync(u->h_out, u->d_out, total, hipMemcpyDeviceToHost, s));
        RLGPU_CHECK_HIP(hipStreamSynchronize(s));
        std::memcpy(h_action_index, u->h_out, ab);
        if (h_logp) std::memcpy(h_logp, u->h_out + ab, lb);
        std::memcpy(h_actions, u->h_out + ab + lb, 8 * lb);
    });
}

/*
 * rlgpu_infer_unit.h -- C ABI of deployment inference: actions for (player, GameState) pairs.
 *
 * Replaces GGL::InferUnit (GigaLearnCPP/src/public/GigaLearnCPP/Util/InferUnit.{h,cpp}): for every row, a
 * (state, player) pair, the unit builds the obs row (AdvancedObs, DefaultObs or DefaultObsPadded) and DefaultAction's
 * mask from the host GameState record, runs shared head -> policy, takes the argmax or samples at the call's
 * temperature, and returns the action index, its log prob and DefaultAction's parsed action (8 floats: throttle,
 * steer, pitch, yaw, roll, jump, boost, handbrake).
 *
 * The records are rlgpu_gamestate (rlgpu_gamestate.h): RocketSim's GetState units.  Player order in a row is the
 * reference's (AdvancedObs.cpp:246-263, DefaultObs.cpp:19-54): self, the teammates in state.players order, the
 * opponents in state.players order; self is skipped by car_id and a player's side is its `team`, never its index.
 * 2v2 only: every state holds two players per team.
 *
 * A call is one upload, the row kernel, the policy handle's own inference path at the call's temperature (the fused
 * kernel, the layered kernels or the fp32 forward, whatever the handle runs), a small parse kernel and one download.
 * On request (rlgpu_infer_unit_set_one_launch), and where the policy runs on the one-wave inference kernel
 * (rlgpu_ppo_wave_infer: LeakyReLU / ReLU, widths <= 512, 16-bit inference, RLGPU_FUSED_INFER not 0), the three
 * kernels are one launch (rows -> forward -> sampler -> parsed action).  Both paths give the same bits.
 *
 * Sampling is the engine's: Philox key = the policy handle's seed, counter = (row0 + i + the handle's
 * sample_row_offset, rng_step).  The reference draws from libtorch's global generator; here two units with the same
 * seed and the same calls give the same actions.
 */
#ifndef RLGPU_INFER_UNIT_H
#define RLGPU_INFER_UNIT_H

#include <stdint.h>
#include "rlgpu_core.h"
#include "rlgpu_gamestate.h"
#include "rlgpu_ppo.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rlgpu_infer_unit rlgpu_infer_unit;

typedef struct {
    int32_t obs_builder, obs_max_players;                  /* as rlgpu_envset_config */
    float obs_pos_coef[3], obs_vel_coef, obs_ang_vel_coef; /* all 0 = the builder's defaults */
    uint64_t obs_seed;                                     /* DefaultObsPadded's shuffle key: an env set's seed
                                                              reproduces that set's rows (row0 + i = its player) */
} rlgpu_infer_unit_config;

/* The unit borrows `policy` (the caller keeps it alive and loads its parameters: rlgpu_ppo_buffers +
 * rlgpu_ppo_refresh_half; its critic is unused).  Refused by name before any device work: an obs builder whose
 * width is not the handle's obs_size, num_actions != 90, an unknown builder or maxPlayers. */
int rlgpu_infer_unit_create(const rlgpu_infer_unit_config* cfg, rlgpu_ppo* policy, rlgpu_infer_unit** out);
int rlgpu_infer_unit_destroy(rlgpu_infer_unit* u);
int rlgpu_infer_unit_obs_size(rlgpu_infer_unit* u);
/* The one-launch path is off by default (it measured slower than the two-step path at every row count, DESIGN.md
 * section 11): on != 0 asks for it; it runs where rlgpu_ppo_wave_infer(policy, 0) holds. */
int rlgpu_infer_unit_set_one_launch(rlgpu_infer_unit* u, int32_t on);
/* 1: the next call is one launch; 0: the two-step path (read per call: RLGPU_FUSED_INFER) */
int rlgpu_infer_unit_one_launch(rlgpu_infer_unit* u);
/* sizeof(rlgpu_infer_unit_config), for binding checks */
int rlgpu_infer_unit_config_size(void);

/* The argument checks of build_rows / infer alone (no device work): a state whose four players are not two per team,
 * duplicate car_ids, a player_of_row outside 0..3, a state_of_row outside the states, n <= 0. */
int rlgpu_infer_unit_check_rows(const rlgpu_gamestate* h_states, int32_t n_states, const int32_t* h_state_of_row,
                                const int32_t* h_player_of_row, int32_t n);

/* Rows only, to device arrays: d_obs [n][obs_size] f32, d_masks [n][90].  Row i is player
 * players[h_player_of_row[i]] of h_states[h_state_of_row[i]]; row0 + i is its number in DefaultObsPadded's shuffle
 * stream.  Returns after the stream has drained. */
int rlgpu_infer_unit_build_rows(rlgpu_infer_unit* u, const rlgpu_gamestate* h_states, int32_t n_states,
                                const int32_t* h_state_of_row, const int32_t* h_player_of_row, int32_t n,
                                int64_t row0, float* d_obs, uint8_t* d_masks, void* stream);

/* InferUnit::BatchInferActions: host in, host out, returns after the stream has drained.  temperature: finite and
 * > 0, used in place of the handle's policy_temperature.  h_logp may be NULL; h_actions [n][8]. */
int rlgpu_infer_unit_infer(rlgpu_infer_unit* u, const rlgpu_gamestate* h_states, int32_t n_states,
                           const int32_t* h_state_of_row, const int32_t* h_player_of_row, int32_t n, int64_t row0,
                           int32_t deterministic, float temperature, uint64_t rng_step, int32_t* h_action_index,
                           float* h_logp, float* h_actions, void* stream);

#ifdef __cplusplus
}
#endif
#endif

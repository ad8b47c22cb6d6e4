/*
 * rlgpu_learner.h -- C ABI of the C++ host Learner (reinforcement-learning_amd/host/): the
 * GigaLearnCPP training loop for one GPU rank, every array resident in HBM.
 *
 * Replaces (GigaLearnCPP):
 *   GGL::Learner(EnvCreateFn, LearnerConfig, StepCallbackFn) / Start()
 *                                   src/public/GigaLearnCPP/Learner.h:11-45, Learner.cpp:482-1056
 *     collection   InferActions -> EnvSet step -> trajectory append        Learner.cpp:669-861
 *     consumption  InferCriticBatched, truncation values, GAE::Compute,
 *                  return-std WelfordStat over sampled returns             Learner.cpp:863-990
 *     learning     PPOLearner::Learn (epochs x shuffled batches x minibatches,
 *                  batch advantage normalisation, clip_grad_norm_, AdamW)   PPOLearner.cpp:278-581
 *   GGL::ExperienceBuffer           src/private/GigaLearnCPP/PPO/ExperienceBuffer.{h,cpp}
 *   GGL::WelfordStat                src/private/GigaLearnCPP/Util/WelfordStat.h:7-67
 *   GGL::LearnerConfig / PPOLearnerConfig (hot-path subset, ExampleMain values as defaults)
 *                                   src/public/GigaLearnCPP/LearnerConfig.h, PPO/PPOLearnerConfig.h,
 *                                   src/ExampleMain.cpp:340-430
 *
 * The C++ API (namespaces GGL / RLGC, host/learner.hpp) is the product host code; this C ABI
 * exposes it to other languages (the Python mirror rlgpu/learner.py, bench.py).
 *
 * Multi-GPU: one Learner per rank, arenas sharded (rank r owns its own num_arenas).  The
 * exchanges go through the caller-supplied rlgpu_collective (bench.py binds it to
 * torch.distributed, i.e. RCCL over xGMI on MI355X): the flat fp32 gradient all-reduce (sum)
 * before clip_grad_norm_ (PPOLearner.cpp:521-526), the fp64 batch-advantage moments
 * (PPOLearner.cpp:360-371) and the return samples of the WelfordStat (Learner.cpp:959-967).
 *
 * Return 0 or a negative rlgpu_status (rlgpu_core.h); rlgpu_last_error() has the message.
 */
#ifndef RLGPU_LEARNER_H
#define RLGPU_LEARNER_H

#include <stdint.h>
#include "rlgpu_core.h"
#include "rlgpu_env.h"
#include "rlgpu_ppo.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    /* env (EnvSetConfig + LearnerConfig::tickSkip / actionDelay, ExampleMain.cpp:356-358) */
    int32_t num_arenas;            /* arenas of THIS rank */
    int32_t tick_skip;             /* 8 */
    int32_t action_delay;          /* 7 */
    uint64_t seed;                 /* LearnerConfig::randomSeed (123) */
    float max_episode_duration;    /* seconds (300, ExampleMain) -> 300 * 120 / tickSkip steps */
    /* experience / PPO (PPOLearnerConfig, ExampleMain.cpp:404-430) */
    int32_t rollout_len;           /* T env steps per iteration and rank (tsPerItr = T * 4 * arenas) */
    int32_t epochs;                /* 2 */
    int32_t mini_batch_size;       /* 50000 (per rank) */
    int64_t batch_size;            /* global batch; 0 = the whole iteration (batchSize = tsPerItr) */
    int32_t overbatching;          /* 1 */
    float gamma, gae_lambda;       /* 0.99, 0.95 */
    float clip_range;              /* 0.2 */
    float entropy_scale;           /* 0.035 */
    float policy_lr, critic_lr;    /* 2.5e-4 */
    float reward_clip_range;       /* 200 */
    int32_t return_samples;        /* 150 (Learner.cpp:959-967) */
    int32_t policy_layers[RLGPU_MAX_LAYERS];
    int32_t n_policy_layers;
    int32_t critic_layers[RLGPU_MAX_LAYERS];
    int32_t n_critic_layers;
    int32_t deterministic;         /* LearnerConfig::deterministic */
    int32_t train_gemm;            /* rlgpu_ppo_config.train_gemm */
    int32_t infer_fp16;            /* rlgpu_ppo_config.infer_fp16 (C5: fp16 inference) */
    int32_t frame_stack;           /* K >= 2: the policy / critic see the last K AdvancedObs frames
                                      concatenated (BASELINE config C4; a build extension -- the
                                      reference has no frame stacking); 0 / 1 = off */
    /* sharding */
    int32_t rank, world;
    /* arena meshes (rlgpu_envset_config.mesh_*; NULL = built-in synthetic arena) */
    const float* mesh_tris;
    int32_t mesh_ntris;
    int32_t mesh_objects;
    const int32_t* mesh_object_ntris;
    /* PPOLearnerConfig::sharedHead (rlgpu_ppo_config.shared_layers); n_shared_layers = 0: none */
    int32_t shared_layers[RLGPU_MAX_LAYERS];
    int32_t n_shared_layers;
    /* the EnvCreateFn's reward / terminal lists (rlgpu_envset_config.rewards / terminals; NULL =
     * ExampleMain's), host memory copied at create */
    const rlgpu_reward_spec* rewards;
    int32_t n_rewards;
    const rlgpu_terminal_spec* terminals;
    int32_t n_terminals;
    /* EnvCreateResult::stateSetter of the training arenas (rlgpu_envset_config.state_setter, _flags and the
     * CombinedState list, passed to the env set as they are; 0 = KickoffState).  The list is host memory
     * copied at create. */
    int32_t state_setter;
    int32_t state_setter_flags;
    const rlgpu_state_setter_spec* state_setters;
    int32_t n_state_setters;
    /* EnvCreateResult::obsBuilder of the training arenas (rlgpu_envset_config.obs_builder ..., passed to the env
     * set as they are; all zero = AdvancedObs).  The builder's width (rlgpu_obs_builder_size) times frame_stack
     * is the models' input width; an old-version, guiding or teacher policy must have it. */
    int32_t obs_builder;
    int32_t obs_max_players;
    float obs_pos_coef[3];
    float obs_vel_coef, obs_ang_vel_coef;
    /* Experience scheduling.  RLGPU_EXP_ROLLOUT (0, default): a fixed [T, P] rollout trained in full,
     * the unfinished tail bootstrapped from V(obs_T) (the engine's fast path, BASELINE configs).
     * RLGPU_EXP_TRAJECTORIES (1): the reference's -- steps are kept per player until the trajectory
     * ends, only complete trajectories are trained (in the order they end: combinedTraj), unfinished ones
     * carry over to the next iteration, and collection runs until ts_per_itr steps of complete
     * trajectories are held (Learner.cpp:504-547,823-861), then GAE runs over the trajectories with
     * their truncation values (GAE.cpp:7-208) -- needs max_episode_duration > 0. */
    int32_t experience_mode;
    int64_t ts_per_itr;            /* PPOLearnerConfig::tsPerItr (mode 1); 0 = rollout_len * 4 * num_arenas */
    int32_t experience_capacity;   /* mode 1: store rows (steps kept per player); 0 = maxEpisodeLength +
                                      2 * ceil(ts_per_itr / players) + 64.  Collection also stops when
                                      the store would overwrite a live step (documented divergence). */
    int32_t arith;                 /* rlgpu_envset_config.arith: the reference build's Bullet arithmetic
                                      (include/rlgpu_arith.h; 0 = build.ps1's MSVC x64) */
    int32_t activation;            /* PartialModelConfig::activationType of every model (rlgpu_ppo.h):
                                      RLGPU_ACT_LEAKY_RELU (0, torch::nn::LeakyReLU, slope 0.01), RLGPU_ACT_RELU,
                                      RLGPU_ACT_SIGMOID or RLGPU_ACT_TANH */
    int32_t no_layer_norm;         /* 1: PartialModelConfig::addLayerNorm = false for every model (hidden layers
                                      are Linear -> activation); 0 (a zero-initialised config): LayerNorm on */
    int32_t optimizer;             /* PartialModelConfig::optimType of every model (Models.h:40-56):
                                      RLGPU_OPT_ADAMW (0, libtorch AdamW: weight decay 1e-2), RLGPU_OPT_ADAM
                                      (libtorch Adam: no weight decay), RLGPU_OPT_ADAGRAD, RLGPU_OPT_RMSPROP or
                                      RLGPU_OPT_MAGSGD (rlgpu_ppo.h: rlgpu_ppo_set_optimizer, applied to every
                                      model) */
    int32_t collect_groups;        /* the rollout collection's arena groups, each stepped and inferred on its own
                                      stream and its own partition of the device's CUs, so one group's launch tail
                                      overlaps the others' work (same results bit for bit); 0 = automatic (2 groups
                                      from 4096 arenas on, else one); 1 = one launch per step; G = 2, 4, 8 or 16
                                      when the policy runs on the fused inference kernel, without host plugins or
                                      frame stacking, 4 G | num_arenas and the device is a 256-CU MI355X; one
                                      launch per step otherwise; -1 = the collection loop: the whole rollout in
                                      one launch (rlgpu_envset_collect_loop, same results bit for bit) in every
                                      iteration where it is eligible -- no host plugins, frame stacking, trajectory
                                      mode or old version playing, and the entry's own conditions -- and the
                                      automatic choice's path otherwise.  The report then has env_launch_arenas =
                                      num_arenas and env_kernel_ms (min / median / max alike) = the launch's time /
                                      rollout_len, the in-workgroup inference included.  With obs standardisation
                                      on (rlgpu_learner_set_obs_standardization) every value takes one launch per
                                      step: each step's statistic draws rows of all arenas */
    float policy_temperature;      /* rlgpu_ppo_config.policy_temperature (PPOLearnerConfig::policyTemperature):
                                      collection, old versions and Learn alike; 0 = 1 */
    int32_t mask_entropy;          /* rlgpu_ppo_config.mask_entropy (PPOLearnerConfig::maskEntropy) */
} rlgpu_learner_config;

enum { RLGPU_EXP_ROLLOUT = 0, RLGPU_EXP_TRAJECTORIES = 1 };

/* Fills ExampleMain's values (src/ExampleMain.cpp:340-430) for a C2 rank: 4096 arenas, T = 128,
 * [512, 512] actor / critic (BASELINE config C2, no shared head), world 1.  ExampleMain's own
 * topology -- shared head [384, 384], policy / critic [384] x 3 as its log prints it
 * (run_out.log:25-28) -- is what host/example_main.cpp (rlgpu_train) selects. */
int rlgpu_learner_default_config(rlgpu_learner_config* cfg);
/* sizeof(rlgpu_learner_config), for language bindings to check their mirror of the struct against. */
int32_t rlgpu_learner_config_size(void);

/* Collectives for world > 1, called synchronously from the learner's host thread (the learner's
 * stream is synchronised before each call).  Return 0 on success. */
typedef struct {
    void* user;
    int (*allreduce_sum_f32)(void* user, float* d_buf, int64_t n);           /* device buffer, in place */
    int (*allreduce_sum_f64)(void* user, double* h_buf, int64_t n);          /* host buffer, in place */
    int (*allgather_f32)(void* user, const float* h_in, int64_t n, float* h_out); /* host, out [world * n] */
} rlgpu_collective;

/* The collective over a native RCCL communicator (one rank per GPU, RCCL over xGMI; host/
 * rccl_collective.cpp): the gradient all-reduce is enqueued on `stream` (the learner's), the fp64
 * moments and return samples are staged through the device.  Rank 0 makes the 128-byte unique id and
 * the launcher hands it to every rank (rlgpu_train: a file; Python: any side channel); every rank then
 * calls create with its rank and the world size (ncclCommInitRank, collective across the ranks).
 * destroy frees the communicator and zeroes the struct. */
#define RLGPU_RCCL_ID_BYTES 128
int rlgpu_rccl_unique_id(uint8_t* out, int32_t out_bytes);
int rlgpu_rccl_collective_create(const uint8_t* id, int32_t rank, int32_t world, void* stream, rlgpu_collective* out);
int rlgpu_rccl_collective_destroy(rlgpu_collective* c);

/* Device views of the rollout (ExperienceBuffer) in HBM, [T, P] time-major, P = 4 * num_arenas.
 * W = obs_width = RLGPU_OBS * max(1, frame_stack). */
typedef struct {
    float* obs;          /* [T + 1][P][W] */
    uint8_t* masks;      /* [T + 1][P][RLGPU_ACTIONS] */
    int32_t* actions;    /* [T][P] */
    float* logp;         /* [T][P] */
    float* rewards;      /* [T][P] */
    int8_t* terms;       /* [T][P] trajectory codes 0 / 1 NORMAL / 2 TRUNCATED */
    float* trunc_obs;    /* [T][P][W] */
    float* values;       /* [T + 1][P] */
    float* trunc_vals;   /* [T][P] (rows with code 2) */
    float* adv;          /* [T][P] */
    float* target;       /* [T][P] */
    float* ret;          /* [T][P] */
    int32_t T, P;
    int32_t obs_width;   /* W */
} rlgpu_rollout_view;

/* The trained batch of RLGPU_EXP_TRAJECTORIES (valid after consume, until the next collect): the
 * complete trajectories of the iteration concatenated in the order they ended (combinedTraj), their
 * critic values / GAE outputs, the truncation list (nextTruncStates and their values, in the same
 * order), and the trajectory records. */
typedef struct {
    float* obs;          /* [num_rows][obs_width] */
    uint8_t* masks;      /* [num_rows][RLGPU_ACTIONS] */
    int32_t* actions;
    float* logp, *rewards;
    int8_t* terms;       /* 0 inside a trajectory, its code (1 / 2) on its last step */
    float* values, *adv, *target, *ret;
    int64_t num_rows;
    float* trunc_obs;    /* [num_truncs][obs_width] */
    float* trunc_vals;   /* [num_truncs] */
    int64_t num_truncs;
    int32_t *seg_player, *seg_start, *seg_len, *seg_code, *seg_tidx; /* [num_segments] */
    int64_t* seg_off;    /* first row of each trajectory in the batch */
    int64_t num_segments;
    int32_t store_rows;  /* the per-player step store's rows (circular) */
    int32_t steps;       /* env steps collected this iteration */
    int64_t first_step;  /* global index of its first step; store row = step % store_rows */
} rlgpu_batch_view;

/* Host-side statistics (checkpoint RUNNING_STATS.json, Learner.cpp:224-279). */
typedef struct {
    int64_t total_steps;        /* timesteps of the current policy's players, all ranks */
    int64_t iteration;
    int64_t return_n;           /* WelfordStat of sampled returns */
    double return_mean, return_m2;
    int64_t rng_step;           /* action-sampling counter */
} rlgpu_learner_stats;

typedef struct {
    double collect_s, consume_s, learn_s;   /* host wall time of the phases (stream-synchronised) */
    double env_kernel_ms;                   /* mean fused env-step time (HIP events), if timing is on */
    int64_t env_steps;                      /* env steps of this rank this iteration */
    double learn_issue_s;                   /* host time to enqueue the learn phase (before its sync):
                                               close to learn_s means the phase is launch-bound */
    double collect_issue_s;                 /* the same for the collection phase */
    int32_t env_launch_arenas;              /* arenas per timed env launch (num_arenas / collection groups) */
    double env_kernel_min_ms;               /* fastest / median / slowest timed env launch of the iteration */
    double env_kernel_median_ms;
    double env_kernel_max_ms;
} rlgpu_learner_report;

typedef struct rlgpu_learner rlgpu_learner;

int rlgpu_learner_create(const rlgpu_learner_config* cfg, const rlgpu_collective* coll, void* stream,
                         rlgpu_learner** out);
int rlgpu_learner_destroy(rlgpu_learner* h);
/* The owned env set and PPO handles (valid until destroy). */
int rlgpu_learner_handles(rlgpu_learner* h, rlgpu_envset** env, rlgpu_ppo** ppo);
int rlgpu_learner_rollout(rlgpu_learner* h, rlgpu_rollout_view* out);
/* The trained batch of RLGPU_EXP_TRAJECTORIES (RLGPU_ERR_STATE in the rollout mode). */
int rlgpu_learner_batch(rlgpu_learner* h, rlgpu_batch_view* out);

/* One iteration = collect + consume + learn + finish (Learner::Start loop body). */
int rlgpu_learner_iterate(rlgpu_learner* h, rlgpu_learner_report* rep);
/* The phases separately (enqueued on the learner's stream; consume and learn synchronise where
 * the host needs device results). */
int rlgpu_learner_collect(rlgpu_learner* h);
int rlgpu_learner_consume(rlgpu_learner* h);
int rlgpu_learner_learn(rlgpu_learner* h);
/* Next rollout starts from the last obs; counters (total steps of the current policy's players). */
int rlgpu_learner_finish_iteration(rlgpu_learner* h);

/* Self-play (Learner.cpp:587-627,733-767): team 0 / 1 acts with the old version set through
 * rlgpu_ppo_set_version (its rows are simulated but not trained or counted); -1 = off. */
int rlgpu_learner_set_old_team(rlgpu_learner* h, int32_t team);

/* Guiding policy (PPOLearnerConfig::useGuidingPolicy / guidingStrength, PPOLearner.cpp:35-38,458-468): d_policy_params
 * is the frozen policy's flat fp32 parameters in rlgpu_ppo_set_guide's layout (the policy's, then the shared head's);
 * every later learn phase runs one guide pass over the rows it trains on (T * P rows of the rollout, or the combined
 * batch's in RLGPU_EXP_TRAJECTORIES) and adds guiding_strength * mean |guide probs - probs| to every minibatch's loss
 * (rlgpu_ppo_minibatch_guided; metric RLGPU_M_GUIDING_LOSS).  Collection is untouched.  guiding_strength finite and
 * >= 0; RLGPU_ERR_UNSUPPORTED with fp32 inference.  guide_logits: a read-only view of the last learn phase's guide
 * logits, [rows][RLGPU_ACTIONS] in the 16-bit inference format (NULL / 0 before the first guided learn). */
int rlgpu_learner_set_guide(rlgpu_learner* h, const float* d_policy_params, float guiding_strength);
int rlgpu_learner_guide_logits(rlgpu_learner* h, const uint16_t** d_logits, int64_t* rows);

/* Transfer learning (Learner::StartTransferLearn, Learner.cpp:299-480; TransferLearnConfig.h): distil an old policy -- the
 * teacher, an ordinary rlgpu_ppo handle built from the old policy / shared-head configuration with obs_size = RLGPU_OBS
 * and num_actions = RLGPU_ACTIONS, its parameters loaded by the caller -- into the learner's policy (and shared head).
 * set_teacher borrows the handle (the caller keeps it alive and destroys it after the learner; NULL removes it).
 * transfer_iterate is one iteration of the reference's loop:
 *   collect    the rollout the usual way, on whichever collection path is eligible, the current policy sampling the
 *              actions; the batch is the rollout's rollout_len * players rows (the caller sizes rollout_len as
 *              ceil(batchSize / players)); there is no consume phase (no critic pass, no GAE);
 *   teacher    one rlgpu_ppo_teacher_probs pass over rows [0, T * P) of the rollout's obs / masks;
 *   epochs     cfg->epochs times: rlgpu_ppo_transfer_chunk over the whole batch in chunks of the handle's max_rows (no
 *              minibatches: the chunks sum to the whole-batch gradient), then rlgpu_ppo_transfer_step(cfg->lr);
 *   finish     as rlgpu_learner_finish_iteration (counters, the next rollout starts from the last obs).
 * The critic, its moments and its optimiser step count do not move.  Metrics (rlgpu_learner_metrics; the count
 * advances by one per transfer iteration): RLGPU_M_TL_OLD_ENTROPY, and from epoch 0 RLGPU_M_TL_LOSS, RLGPU_M_TL_ACCURACY
 * and RLGPU_M_ENTROPY, each the whole batch's mean; RLGPU_M_TL_UPDATE_MAGNITUDE ("Policy Update Magnitude") is written,
 * not summed.  Reset the metrics between ordinary and transfer iterations: both use RLGPU_M_ENTROPY and the count.
 * The report has collect_s and learn_s (the teacher pass, the epochs and the finish); consume_s is 0.
 * Supported teacher at this level: the engine's own obs builder and action parser (whatever width the env emits), any
 * architecture.  RLGPU_ERR_STATE without a teacher; RLGPU_ERR_INVALID_ARG for loss_exponent < 1 (rlgpu_ppo_transfer_chunk);
 * RLGPU_ERR_UNSUPPORTED, each named in the message, for
 *   world > 1            the whole-batch mean and the policy-only step are not reduced over ranks,
 *   frame_stack > 1      the teacher would need its own frame history,
 *   RLGPU_EXP_TRAJECTORIES  the batch is the rollout's rows,
 *   obs standardisation  the teacher would need the raw rows,
 *   deterministic        the reference samples the batch's actions,
 *   an old team set      the batch is collected by the current policy alone. */
typedef struct {
    float lr;             /* TransferLearnConfig::lr (3e-4) */
    int32_t epochs;       /* 5 */
    int32_t use_kl;       /* useKLDiv: |o log(o / c)| instead of |o - c| */
    float loss_scale;     /* 500 */
    float loss_exponent;  /* 1; finite and >= 1 */
} rlgpu_transfer_config;
int rlgpu_learner_set_teacher(rlgpu_learner* h, rlgpu_ppo* teacher);
int rlgpu_learner_transfer_iterate(rlgpu_learner* h, const rlgpu_transfer_config* cfg, rlgpu_learner_report* rep);

/* Obs standardisation (LearnerConfig::standardizeObs / minObsSTD / maxObsMeanRange / maxObsSamples; Learner.cpp:679-693,
 * Util/WelfordStat.h:69-243).  Every obs set the policy is about to see -- row 0, then each step's appended row -- takes
 * one rlgpu_obs_stat_step on the learner's stream: a BatchedWelfordStat over the obs columns (int64 count, fp64 means and
 * m2) is incremented from S = min(players, max_samples) rows drawn with replacement, then every row becomes
 * x * inv[j] + shift[j] in fp32 (untouched while count < 2).  The rewritten rows feed the policy (an old version too)
 * and are what the critic and the learn phase train on; the truncation rows (trunc_obs) and the skill matches stay raw,
 * as in the reference.  The collection then runs one launch per step (rlgpu_learner_config.collect_groups).
 * min_std finite and > 0, max_mean_range finite and >= 0, max_samples >= 1 (RLGPU_ERR_INVALID_ARG); RLGPU_ERR_UNSUPPORTED
 * with frame_stack > 1 or world > 1; RLGPU_ERR_STATE, like set_obs_stat, once the first collection has started (row 0 has
 * then been taken with the state there was).  enable = 0 turns it off (the other arguments are ignored).
 * get / set_obs_stat: the statistic ([RLGPU_OBS] doubles each; RUNNING_STATS.json "obs_stat": means, vars = m2, count);
 * RLGPU_ERR_STATE while the feature is off.  get synchronises the learner's stream. */
int rlgpu_learner_set_obs_standardization(rlgpu_learner* h, int32_t enable, float min_std, float max_mean_range,
                                          int32_t max_samples);
int rlgpu_learner_get_obs_stat(rlgpu_learner* h, int64_t* count, double* means, double* m2s);
int rlgpu_learner_set_obs_stat(rlgpu_learner* h, int64_t count, const double* means, const double* m2s);

/* The building blocks of the above.  A state of `width` columns is one device block of rlgpu_obs_stat_bytes(width)
 * bytes, 8-byte aligned: int64 count, double mean[width], double m2[width], then scratch every step rewrites (the fp32
 * coefficient table and its "active" word); zero-filled it is a fresh BatchedWelfordStat, and the first 8 + 16 * width
 * bytes are all a resumed run needs.
 * rlgpu_obs_stat_step: one reference step on d_obs [rows][width] (4-byte aligned), in place, two launches on `stream`.
 * Increment: for i in 0 .. S - 1, S = min(rows, max_samples), row r_i = rlgpu_obs_sample_rows(seed, count, ...)[i]; per
 * column delta = (double)x - mean, deltaN = delta / (double)(count + 1), mean += deltaN, m2 += (delta * deltaN) *
 * (double)count; count++ after each row.  Normalise (count >= 2): var = m2 / (count - 1), std = var > 0 ? sqrt(var) : 1,
 * inv = 1.0f / (float)max(std, min_std), shift = -(float)clamp(mean, -max_mean_range, max_mean_range) * inv, then
 * x = x * inv + shift -- no operation contracted, each rounds on its own.
 * rlgpu_obs_sample_rows (host, no GPU): the n rows drawn when the state's count is `count`: draw i is the first output
 * word u of Philox4x32-10 at counter count + i under a key derived from seed and stream tag 3 (disjoint from the
 * sampler's, the arenas' and rlgpu_host_uniform's streams), row = (uint64(u) * rows) >> 32. */
int64_t rlgpu_obs_stat_bytes(int32_t width);
int rlgpu_obs_stat_step(void* d_state, float* d_obs, int32_t rows, int32_t width, uint64_t seed, int32_t max_samples,
                        float max_mean_range, float min_std, void* stream);
int rlgpu_obs_sample_rows(uint64_t seed, int64_t count, int32_t rows, int32_t n, int32_t* out);

/* Host plugins and a StepCallbackFn inside the collection loop (Learner.cpp:676-861; EnvSet.cpp:163-255).
 * With a hook set, every collection step runs: the env step WITHOUT resetting terminated arenas, then
 * fn(user, RLGPU_HOOK_AFTER_STEP) -- the env set (rlgpu_learner_handles) holds the post-step, pre-reset state;
 * the hook may download GameStates, run user plugins and rewrite the env's rewards [players] / terminals
 * [arenas] buffers (device, rlgpu_envset_buffers) -- then the trajectory codes (the merged terminal, else the
 * max-episode-length truncation), rewards and truncation rows are appended, every arena whose terminal is
 * set is reset (rlgpu_envset_reset), fn(user, RLGPU_HOOK_AFTER_RESET) runs (the plugins' Reset on the new
 * states), and the post-reset obs / masks are appended.  fn returns 0, else the iteration fails with
 * RLGPU_ERR_STATE.  fn == NULL restores the fused step.  Without host changes the two paths are
 * bit-identical. */
enum { RLGPU_HOOK_AFTER_STEP = 0, RLGPU_HOOK_AFTER_RESET = 1 };
typedef int (*rlgpu_step_hook_fn)(void* user, int32_t phase);
int rlgpu_learner_set_step_hook(rlgpu_learner* h, rlgpu_step_hook_fn fn, void* user);

/* Gradient tap (monitoring / tests; PPOLearner.cpp:990-1000's point between the all-reduce and
 * clip_grad_norm_): after each batch's gradients are summed over the ranks and before they are clipped
 * and stepped, fn receives the device pointer of the flat fp32 gradient [n] (the stream synchronised; the
 * buffer is read-only for fn), the epoch and the batch's index within it.  A non-zero return fails the
 * iteration.  fn null removes the tap. */
typedef int (*rlgpu_grad_hook_fn)(void* user, const float* grads, int64_t n, int32_t epoch, int32_t batch);
int rlgpu_learner_set_grad_hook(rlgpu_learner* h, rlgpu_grad_hook_fn fn, void* user);

int rlgpu_learner_get_stats(rlgpu_learner* h, rlgpu_learner_stats* out);
int rlgpu_learner_set_stats(rlgpu_learner* h, const rlgpu_learner_stats* in);
/* PPO report metrics accumulated since the last reset (PPOLearner.cpp:537-566): h_out receives
 * RLGPU_NUM_METRICS sums (rlgpu_ppo.h RLGPU_M_*), *count the number of minibatches summed. */
int rlgpu_learner_metrics(rlgpu_learner* h, float* h_out, int64_t* count, int32_t reset);
/* ExampleMain's StepCallback metrics over the collection steps since the last reset (enabled at
 * create; rlgpu_envset_step_metrics of the owned env set): Report::Avg totals / counts of the
 * RLGPU_NUM_STEP_METRICS keys (rlgpu_step_metric_name). */
int rlgpu_learner_step_metrics(rlgpu_learner* h, double* h_total, uint64_t* h_count, int32_t reset);
/* Record HIP events around every fused env step (rlgpu_learner_report.env_kernel_ms). */
int rlgpu_learner_set_env_timing(rlgpu_learner* h, int32_t enable);

/* Host building blocks, exported for tests (no GPU needed). */
/* ExperienceBuffer::GetAllBatchesShuffled batch boundaries (ExperienceBuffer.cpp:117-162): writes up
 * to max_ranges [start, end) pairs into out (2 * max_ranges int64), returns the count (>= 0). */
int64_t rlgpu_batch_ranges(int64_t exp_size, int64_t batch_size, int32_t overbatching, int64_t* out,
                           int64_t max_ranges);
/* WelfordStat::Increment over n floats (fp64 state in/out: count, mean, m2). */
int rlgpu_welford_add(int64_t* count, double* mean, double* m2, const float* xs, int64_t n);
/* WelfordStat::GetSTD (1 when count < 2 or variance <= 0). */
double rlgpu_welford_std(int64_t count, double m2);
/* Global batch-advantage (mean, unbiased std) from all-reduced fp64 moments (sum, sum of squares,
 * count) -- the multi-rank form of PPOLearner.cpp:360-371. */
int rlgpu_moments_mean_std(const double* moments3, float* out2);
/* The return-sample indices of one iteration: n draws in [0, range) from a counter-based
 * generator keyed by (seed, rank, iteration) -- every language binding reproduces the same draws. */
int rlgpu_sample_indices(uint64_t seed, int32_t rank, int64_t iteration, int64_t range, int32_t n, int64_t* out);
/* The host picks of self-play and the skill matches (RocketSim::Math::RandFloat / RandInt in the reference:
 * Learner.cpp:589-600, PolicyVersionManager.cpp:181-186): a counter-based uniform in [0, 1) of (seed, stream,
 * counter), so every binding (the C++ trainer facade, Python) makes the same picks.  Streams in use: 1 = the
 * self-play draw of iteration i at counters 3 i .. 3 i + 2 (old-version chance, version, team); 2 = skill run r
 * at 2 r, 2 r + 1 (version, new team). */
double rlgpu_host_uniform(uint64_t seed, uint64_t stream, uint64_t counter);
/* The return-sample rows of one iteration, drawn only from steps of FINISHED trajectories -- the
 * reference samples tReturns of combinedTraj, which holds complete trajectories only
 * (Learner.cpp:823-861, 959-967).  ends[p] = the last step t of column p whose trajectory code is
 * nonzero (-1: no trajectory of p ends inside the rollout, or p is not sampled); the eligible rows
 * are (t, p) with t <= ends[p], whose discounted returns run to their trajectory's end.  Draws
 * min(n, #eligible) rows uniformly with replacement (torch::randint, Learner.cpp:963) from the
 * rlgpu_sample_indices sequence; writes row indices t * P + p to out and their count to *n_out. */
int rlgpu_sample_finished_rows(uint64_t seed, int32_t rank, int64_t iteration, const int32_t* ends, int32_t P,
                               int32_t n, int64_t* out, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif

// common.hpp -- shared host helpers for the rlgpu C ABI implementation.
// Error handling mirrors the reference's throw-on-error (RG_ERR_CLOSE,
// GigaLearnCPP/RLGymCPP/src/RLGymCPP/Framework.h:16-21) but converts to the
// int-status + thread-local-message convention of include/rlgpu_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../include/rlgpu_core.h"

namespace rlgpu {

void set_last_error(const std::string& msg);

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define RLGPU_CHECK_HIP(expr)                                                                \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            throw ::rlgpu::Error(RLGPU_ERR_HIP, std::string(#expr " failed: ") +             \
                                                    hipGetErrorString(_e));                  \
    } while (0)

#define RLGPU_REQUIRE(cond, msg)                                                             \
    do {                                                                                     \
        if (!(cond)) throw ::rlgpu::Error(RLGPU_ERR_INVALID_ARG, std::string(msg));          \
    } while (0)

// Run a body, converting exceptions into a status code (no exception crosses the ABI).
template <class F>
inline int guarded(F&& f) {
    try {
        f();
        return RLGPU_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("host allocation failed");
        return RLGPU_ERR_OOM;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return RLGPU_ERR_STATE;
    }
}

// The one place that allocates and frees persistent device memory (the env set's, the PPO handle's and the host
// Learner's buffers): hipMalloc / hipFree, counted for rlgpu_live_device_allocations.  dev_alloc throws an Error
// on failure; dev_free takes null.  Stream-ordered temporaries of a single call and per-device static scratch are
// not persistent in this sense and stay outside.
void* dev_alloc(size_t bytes);
void dev_free(void* p);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline unsigned ceil_div(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

// infer_act.hip: one launch of the fused inference kernel's SIGMOID / TANH instance (infer::mlp_infer<f16, act>)
// with the infer::InferArgs at args (bytes = its size, checked)
void launch_mlp_infer_act(int act, bool f16, unsigned blocks, hipStream_t s, const void* args, size_t bytes);
// infer_wave.hip: one launch of the one-wave form (infer::mlp_infer_wave<f16>, LeakyReLU / ReLU), 16 rows per workgroup
void launch_mlp_infer_wave(bool f16, unsigned blocks, hipStream_t s, const void* args, size_t bytes);

// transfer.hip: the transfer-learning kernels (transfer_kernels.hpp), launched for ppo.hip's entry points.
// teacher_probs over n rows of f32 logits [n][A_old]: clamped masked softmax, its entropy / total_rows added into the
// metric slot, the optional gather by map [n][A] into probs [n][A], the gathered row's argmax.
struct TeacherProbsArgs {
    const float* logits;
    const uint8_t* masks;
    int n, A_old;
    const int32_t* map;  // null: A = A_old, no gather
    int A;
    float temp;
    int mask_entropy;
    int64_t total_rows;
    float* probs;
    int32_t* argmax;
    float* metrics;
};
void launch_teacher_probs(const TeacherProbsArgs& a, hipStream_t s);
// transfer_loss over the n rows idx[start .. start + n) (idx null: identity) of a batch of total_rows rows: dlogits rows of
// ldd floats, bias partials [transfer_loss_blocks(n)][A], the H3 max |dlogits| (amax null outside H3), the metric sums
struct TransferLossArgs {
    const float* logits;
    const uint8_t* masks;
    const float* target;
    const int32_t* target_argmax;
    const int32_t* idx;
    int64_t start;
    int n, A;
    float temp;
    int mask_entropy;
    int64_t total_rows;
    int use_kl;
    float loss_scale, exponent;
    float* dlogits;
    int ldd;
    float* metrics;
    float* bias_part;
    float* amax;
};
int transfer_loss_blocks(int n);
void launch_transfer_loss(const TransferLossArgs& a, hipStream_t s);
// adamw's arithmetic without a clip coefficient on one span of n parameters; zeroes g
void launch_adam_models(float* p, float* g, float* m, float* v, int64_t n, float decay_mul, float beta1, float beta2,
                        float step_size, float bc2_sqrt, float eps, hipStream_t s);
// one unclipped step of a non-Adam optimizer (kind: RLGPU_OPT_ADAGRAD / _RMSPROP / _MAGSGD; ppo::optim_step) on one span
// of n parameters, v the span's exp_avg_sq; zeroes g.  MagSGD reduces ||g|| first: part512 is 512 floats of scratch and
// norm one float, both untouched by the other kinds
void launch_optim_models(int kind, float* p, float* g, float* v, int64_t n, float lr, float* part512, float* norm,
                         hipStream_t s);
// *out = ||a - b|| over n floats (part512: 512 floats of scratch)
void launch_diff_norm(const float* a, const float* b, int64_t n, float* part512, float* out, hipStream_t s);

}  // namespace rlgpu

// ppo.hip, for env.hip's collection loop (rlgpu_envset_collect_loop): whether the policy runs on the one-wave
// inference kernel with these obs / action widths, and the infer::InferArgs bytes (blob, at most cap) of its sampling
// forward over rollout row 0 -- n rows of d_obs / d_masks, global rows from the handle's sample_row_offset, the draw
// of rng_step -- with *f16 its 16-bit format.
struct rlgpu_ppo;
namespace rlgpu {
bool ppo_wave_policy(rlgpu_ppo* h, int obs_size, int num_actions);
void ppo_wave_args(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, int64_t n, int deterministic, uint64_t rng_step,
                   int32_t* d_actions, float* d_logp, void* blob, size_t cap, bool* f16);
// ppo.hip, for infer_unit.hip (rlgpu_infer_unit_*): the handle's obs / action widths, and the handle's own sampling
// path (fused, layered or fp32, in chunks of max_rows) over n rows numbered from row0 + sample_row_offset with
// `temperature` in place of the handle's policy_temperature
void ppo_widths(rlgpu_ppo* h, int* obs_size, int* num_actions);
void ppo_infer_actions_temp(rlgpu_ppo* h, const float* d_obs, const uint8_t* d_masks, int64_t n, int64_t row0,
                            int deterministic, float temperature, uint64_t rng_step, int32_t* d_actions, float* d_logp,
                            hipStream_t s);
}  // namespace rlgpu

// env.hip, for infer_unit.hip: a config's obs builder as the kernels read it (the obs_* fields of rl::Plugins at
// `plugins`, validated as rlgpu_envset_create validates them; seed keys DefaultObsPadded's shuffles), and
// DefaultAction's table [RLGPU_ACTIONS][8] with its mask bits [RLGPU_ACTIONS] (rl::EnvConst::action / mask_bits)
namespace rlgpu {
void obs_builder_plugins(int kind, int max_players, const float pos_coef[3], float vel_coef, float ang_vel_coef, uint64_t seed,
                         void* plugins);
void default_action_tables(float* action, uint8_t* mask_bits);
}  // namespace rlgpu

// learner.hpp -- C++ host API of the MI355X rollout engine: the GigaLearnCPP Learner /
// ExperienceBuffer / WelfordStat and the RLGymCPP EnvSet surface over the rlgpu C ABI.
//
// This is the host code the reference's src/ExampleMain.cpp drops onto (host/example_main.cpp
// mirrors it).  Every C-ABI status is turned back into std::runtime_error, so the reference's
// try/catch (Learner.cpp:466-474, ExampleMain.cpp:603-612) keeps its behaviour.
//
// Ownership: every device buffer of this side is a DevArray member (of ExperienceBuffer, TrajectoryStore,
// PPOLearnerGPU or the Learner), the pinned counters and the env / PPO handles are unique_ptrs.  Nothing is freed
// by name: members go in reverse declaration order, the handles declared before (so destroyed after) the buffers
// a kernel of theirs may still read, and a constructor that throws releases what it had acquired.
//
// Reference map (GigaLearnCPP/RLGymCPP, paths as SURVEY.md):
//   RLGC::EnvSetGPU      RG/EnvSet/EnvSet.h:67-124        (EnvSet: StepFirstHalf / StepSecondHalf /
//                                                           Sync / Reset / ResetArena / state)
//   GGL::WelfordStat     GL/private/GigaLearnCPP/Util/WelfordStat.h:7-67
//   GGL::ExperienceBuffer GL/private/GigaLearnCPP/PPO/ExperienceBuffer.{h,cpp} ([T, P] in HBM)
//   GGL::PPOLearnerGPU   GL/private/GigaLearnCPP/PPO/PPOLearner.{h,cpp}
//   GGL::Learner         GL/public/GigaLearnCPP/Learner.{h,cpp}
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rlgpu_env.h"
#include "../../include/rlgpu_gae.h"
#include "../../include/rlgpu_learner.h"
#include "../../include/rlgpu_ppo.h"

namespace RLGC {

inline void RlgpuCheck(int st, const char* what) {
    if (st != RLGPU_OK) throw std::runtime_error(std::string(what) + ": " + rlgpu_last_error());
}

// RLGC::EnvSet on the device (EnvSet.h:67-124): the ExampleMain plugin set built in.
class EnvSetGPU {
public:
    EnvSetGPU(const rlgpu_envset_config& cfg, hipStream_t stream);

    void StepFirstHalf(bool async = true);                        // EnvSet.cpp:113-130
    void StepSecondHalf(const int32_t* d_actions, bool async);    // EnvSet.cpp:132-273
    void Step(const int32_t* d_actions, const rlgpu_step_outputs* out);  // fused + reset + append
    void Sync();                                                  // EnvSet.h:107
    void Reset();                                                 // EnvSet.cpp:331-354
    void ResetArenas(const uint8_t* d_mask);                      // EnvSet.cpp:275-329

    rlgpu_envset* handle() const { return h_.get(); }
    const rlgpu_envset_buffers& state() const { return state_; }  // EnvSet::state (device views)

private:
    struct Destroy {
        void operator()(rlgpu_envset* h) const { rlgpu_envset_destroy(h); }
    };
    std::unique_ptr<rlgpu_envset, Destroy> h_;
    rlgpu_envset_buffers state_{};
    hipStream_t stream_;
};

}  // namespace RLGC

namespace lk {
struct TrajRecs;  // csrc/learner_kernels.hpp
}

namespace GGL {

using RLGC::RlgpuCheck;

// WelfordStat.h:7-67: fp64 running mean / variance in the reference's update order.
struct WelfordStat {
    int64_t count = 0;
    double mean = 0, m2 = 0;
    void Increment(const float* xs, int64_t n);
    double GetMean() const { return count < 2 ? 0.0 : mean; }
    double GetSTD() const;
};

// (mean, unbiased std) from fp64 (sum, sum of squares, count): PPOLearner.cpp:360-371 over ranks
void MomentsMeanStd(const double* m3, float* out2);

// ExperienceBuffer::GetAllBatchesShuffled boundaries (ExperienceBuffer.cpp:117-162).
std::vector<std::pair<int64_t, int64_t>> BatchRanges(int64_t expSize, int64_t batchSize, bool overbatching);

// The one owner of device memory on this side: an array that grows on demand and frees itself (move-only).
// Allocation and release go through rlgpu::dev_alloc / dev_free (csrc/common.hpp), which count them.
template <class T>
struct DevArray {
    T* p = nullptr;
    int64_t cap = 0;  // elements (the block carries 16 bytes of padding beyond them)
    DevArray() = default;
    DevArray(DevArray&& o) noexcept { *this = std::move(o); }
    DevArray& operator=(DevArray&& o) noexcept {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevArray();
    // At least n elements: nothing when n <= cap, else a new block of max(n, 1.5 cap), zero-filled and / or holding
    // the old contents on request (both on s), and the old block freed once s has drained.  A failure leaves the
    // array as it was.
    void Reserve(int64_t n, hipStream_t s, bool keep = false, bool zero = false);
};

// hipHostMalloc'd memory in a unique_ptr
struct PinnedFree {
    void operator()(void* p) const;
};

// The rollout ([T, P] time-major) in HBM; every collected step is trained in the iteration that
// collected it (the unfinished tail bootstrapped from V(obs_T), DESIGN.md Deviations 5).
// In RLGPU_EXP_TRAJECTORIES the same arrays are a circular per-player step store of T rows (obs row r
// = the state the step at row r acted on) and the outputs (values, GAE, truncation rows) live in the
// combined batch instead (rollout_outputs = false).
struct ExperienceBuffer {
    int T = 0, P = 0, W = 0;  // W: obs row width (the env set's obs width x frames)
    rlgpu_rollout_view v{};  // views of the arrays below
    DevArray<float> obs, logp, rewards, truncObs, values, truncVals, adv, target, ret;
    DevArray<uint8_t> masks;
    DevArray<int32_t> actions;
    DevArray<int8_t> terms;
    void Allocate(int T, int P, int W, hipStream_t s, bool rollout_outputs = true);  // zero-filled
};

// RLGPU_EXP_TRAJECTORIES state: per-player trajectories, this iteration's records, truncation list and
// the combined batch (the reference's combinedTraj)
struct TrajectoryStore {
    int Tmax = 0, maxLen = 0;
    int64_t tsPerItr = 0;
    int64_t step = 0;           // global step counter (store row = step % Tmax)
    int64_t firstStep = 0;      // this iteration's first step
    int steps = 0;              // steps collected this iteration
    int lastOldTeam = -1;
    DevArray<int32_t> start, len, trnew;  // [P]
    DevArray<int64_t> counters;           // lk::kTcCount
    std::unique_ptr<int64_t[], PinnedFree> hcounters;  // pinned host copy
    DevArray<int32_t> rp, rstart, rlen, rcode, rtidx;
    DevArray<int64_t> roff;
    DevArray<float> truncObs, truncVals;
    DevArray<float> cObs, cLogp, cRews, cVals, cAdv, cTarget, cRet;
    DevArray<uint8_t> cMasks;
    DevArray<int32_t> cActs;
    DevArray<int8_t> cTerms;
    DevArray<float> truncStage;  // [P][W] stacked pre-reset rows (frame stacking), else empty
    int64_t nrec = 0, ntrunc = 0, nrows = 0;
    lk::TrajRecs Records() const;  // this iteration's records (rp .. roff) as the kernels take them
};

// PPOLearner (PPOLearner.h:41-59) over rlgpu_ppo.
class PPOLearnerGPU {
public:
    PPOLearnerGPU(const rlgpu_ppo_config& cfg, hipStream_t stream);

    void InferActions(const float* d_obs, const uint8_t* d_masks, int n, bool deterministic, uint64_t step,
                      int32_t* d_actions, float* d_logp, const uint8_t* d_old_rows = nullptr);
    void InferCritic(const float* d_obs, int64_t n, float* d_values);
    void AdvantageStats(const float* d_adv, int64_t n);  // (mean, unbiased std) -> adv_stats
    void Minibatch(const float* d_obs, const uint8_t* d_masks, const int32_t* d_actions, const float* d_logp,
                   const float* d_adv, const float* d_target, const int32_t* d_index, int64_t start, int n,
                   int64_t batch, const uint16_t* d_guide_logits = nullptr, float guiding_strength = 0.f);
    void OptimizerStep();
    int64_t minibatches = 0;  // summed into metrics() since the last reset

    rlgpu_ppo* handle() const { return h_.get(); }
    float* grads() const { return grads_; }
    int64_t num_params() const { return nparams_; }
    float* adv_stats() const { return adv_stats_.p; }
    float* metrics() const { return metrics_.p; }

private:
    struct Destroy {
        void operator()(rlgpu_ppo* h) const { rlgpu_ppo_destroy(h); }
    };
    std::unique_ptr<rlgpu_ppo, Destroy> h_;  // before the arrays: a failed allocation unwinds it
    hipStream_t stream_;
    float* grads_ = nullptr;
    int64_t nparams_ = 0;
    DevArray<float> adv_stats_;  // [2]
    DevArray<float> metrics_;    // [RLGPU_NUM_METRICS]
};

// GGL::Learner (Learner.h:11-45): one rank's training loop.
class Learner {
public:
    Learner(const rlgpu_learner_config& cfg, const rlgpu_collective* coll, hipStream_t stream);
    ~Learner();
    Learner(const Learner&) = delete;
    Learner& operator=(const Learner&) = delete;

    void Collect();           // Learner.cpp:669-861
    void Consume();           // Learner.cpp:863-990
    void Learn();             // PPOLearner::Learn, PPOLearner.cpp:278-581
    void FinishIteration();   // obs[0] <- obs[T], step counters
    rlgpu_learner_report Iterate();
    void Start(int64_t iterations);  // Learner::Start loop (Learner.cpp:482-1056), a fixed count
    // Learner::StartTransferLearn's iteration (Learner.cpp:330-462): collect with the current policy, one teacher pass
    // over the rollout's T * P rows, tc.epochs times [every chunk, then the policy-only step], finish.  The teacher is
    // borrowed (SetTeacher); rlgpu_learner_transfer_iterate documents what is refused.
    void SetTeacher(rlgpu_ppo* teacher) { teacher_ = teacher; }
    rlgpu_learner_report TransferIterate(const rlgpu_transfer_config& tc);

    void SetOldTeam(int team) { oldTeam_ = team; }
    // PPOLearnerConfig::useGuidingPolicy: the guide's flat fp32 parameters (rlgpu_ppo_set_guide's layout) and
    // guidingStrength; every later Learn adds the guiding term
    void SetGuide(const float* d_policy_params, float strength);
    const uint16_t* guideLogits() const { return guideLogits_.p; }
    int64_t guideRows() const { return guideRows_; }
    void SetGradHook(rlgpu_grad_hook_fn fn, void* user) {
        gradHook_ = fn;
        gradHookUser_ = user;
    }
    void SetStepHook(rlgpu_step_hook_fn fn, void* user) {
        hook_ = fn;
        hookUser_ = user;
    }
    void SetEnvTiming(bool on) { envTiming_ = on; }
    // LearnerConfig::standardizeObs / minObsSTD / maxObsMeanRange / maxObsSamples (Learner.cpp:679-693): every obs set
    // the policy sees first increments a BatchedWelfordStat from min(P, maxSamples) drawn rows and is then rewritten in
    // place; the truncation rows stay raw, as in the reference.  Before the first collection only.
    void SetObsStandardization(bool enable, float minStd, float maxMeanRange, int maxSamples);
    void GetObsStat(int64_t* count, double* means, double* m2s);  // [obs width] each; synchronises
    void SetObsStat(int64_t count, const double* means, const double* m2s);

    const rlgpu_learner_config& config() const { return cfg_; }
    RLGC::EnvSetGPU& env() { return *env_; }
    PPOLearnerGPU& ppo() { return *ppo_; }
    ExperienceBuffer& exp() { return exp_; }
    rlgpu_learner_stats stats;
    WelfordStat returnStat;

private:
    void StepEnv(const int32_t* d_actions, const rlgpu_step_outputs& o);
    void ActAndStep(size_t row, size_t next, float* trunc, float* truncStacked, hipEvent_t* timing);
    void EnsureEvents(size_t count);
    void AllReduceGrads(int epoch, int batch);
    void BatchAdvantageStats(const float* d_adv, const int32_t* d_idx, int64_t n);
    void CollectTrajectories();
    void ConsumeTrajectories();
    std::vector<float> GatherReturns(const float* d_ret, const int64_t* idx, size_t m);
    void FeedReturnStat(const float* d_ret, const std::vector<int64_t>& idx, int32_t m);
    bool trajMode() const { return cfg_.experience_mode == RLGPU_EXP_TRAJECTORIES; }
    hipStream_t s_;
    rlgpu_learner_config cfg_;
    rlgpu_collective coll_{};
    bool hasColl_ = false;
    // the env set and the PPO handle come before every buffer below, `traj` included: members go in reverse
    // order, so the kernels of either that may still read a buffer are gone (hipFree synchronises) before it
    std::unique_ptr<RLGC::EnvSetGPU> env_;
    std::unique_ptr<PPOLearnerGPU> ppo_;
    ExperienceBuffer exp_;
    int oldTeam_ = -1;
    bool envTiming_ = false;
    rlgpu_step_hook_fn hook_ = nullptr;  // host plugins / StepCallbackFn (rlgpu_learner_set_step_hook)
    void* hookUser_ = nullptr;
    rlgpu_grad_hook_fn gradHook_ = nullptr;
    void* gradHookUser_ = nullptr;
    int K_ = 1;                 // frames stacked (config C4)
    int OBS_ = RLGPU_OBS;       // the env set's obs row width (its obs builder's; a rollout row is OBS_ x K_ wide)
    DevArray<float> hist_;      // [K-1][P][OBS_] frame history
    // obs standardisation: the statistic and the coefficient table it yields, in one block (empty while off)
    DevArray<char> obsStat_;    // lk::obs_stat_bytes(OBS_): count, means, m2, then coef [2][OBS_] and the active word
    bool obsStd_ = false;
    bool row0Raw_ = false;      // rollout / store row 0 still holds the env's raw initial obs
    bool collected_ = false;    // the first collection has started
    float obsMinStd_ = 0.1f, obsMeanRange_ = 3.f;
    int obsSamples_ = 100;
    void StandardizeObs(float* d_rows);  // one reference step on [P][OBS_] rows: increment, then normalise
    std::vector<hipEvent_t> ev_;
    // the rollout collection in arena groups (rlgpu_learner_config.collect_groups): one stream per group, each on
    // its own CU partition (host/cu_partition.hpp), joined to s_ by events at the phase's start and end
    std::vector<hipStream_t> gs_;
    std::vector<hipEvent_t> gsEnd_;
    hipEvent_t gsStart_ = nullptr;
    int gsRefused_ = 0;  // the group count whose partition streams could not be made (not tried again)
    int CollectGroups() const;
    bool EnsureGroupStreams(int G);
    int collectGroupsUsed_ = 1;
    void CollectGrouped(int G);
    // the rollout collection in one launch (collect_groups = -1; rlgpu_envset_collect_loop)
    bool collectLoopUsed_ = false;
    bool CollectLoopOk() const;
    void CollectLoop();
    // device scratch
    DevArray<uint8_t> oldRows_[2];
    // the rows that act with the old version this iteration (self-play), or null
    const uint8_t* OldRows() const { return oldTeam_ >= 0 ? oldRows_[oldTeam_].p : nullptr; }
    DevArray<int32_t> trainRows_;
    // the shuffle, its row-selected form and the gathered batch advantages: the same row count each (T * P; Learn
    // grows them to the combined batch in the trajectory mode, whose row count has no fixed bound)
    DevArray<int32_t> perm_, permRows_;
    DevArray<float> badv_;
    // the guiding policy's 16-bit logits of the rows Learn trains on ([T * P][ACT], or the combined batch's rows in
    // the trajectory mode), written once per Learn before the epoch loop; empty without a guide
    DevArray<uint16_t> guideLogits_;
    int64_t guideRows_ = 0;
    float guideStrength_ = 0.f;
    bool hasGuide_ = false;
    void NeedLearnRows(int64_t n, const char* what) const;
    // transfer learning: the borrowed teacher handle, its target probabilities [T * P][ACT] and argmax [T * P] of the
    // rollout's rows, and the policy model's snapshot (reserved by the first transfer iteration; empty otherwise)
    rlgpu_ppo* teacher_ = nullptr;
    DevArray<float> tlProbs_, tlSnapshot_;
    DevArray<int32_t> tlArgmax_;
    DevArray<int32_t> truncRows_, truncCount_;
    DevArray<char> selScratch_;
    size_t selBytes_ = 0;
    DevArray<float> truncObsC_, truncValC_;  // the truncated rows' obs gathered for the critic, and their values
    DevArray<int64_t> sampleIdx_;
    DevArray<float> samples_;
    DevArray<int32_t> ends_;  // [P] last trajectory end per column (return sampling)
    std::vector<int32_t> hostEnds_;
    DevArray<double> mom_;       // [3] + scratch
    DevArray<float> clipSums_;   // [2] GAE clip-portion partial sums
  public:
    TrajectoryStore traj;      // RLGPU_EXP_TRAJECTORIES
};

}  // namespace GGL

// InferUnit.hpp -- GGL::InferUnit (GigaLearnCPP/Util/InferUnit.{h,cpp}) on the MI355X engine: actions of a trained
// policy for (Player, GameState) pairs, over include/rlgpu_infer_unit.h.
//
//   InferUnit(obsBuilder, obsSize, actionParser, sharedHeadConfig, policyConfig, modelsFolder, useGPU = true)
//   InferAction(player, state, deterministic, temperature)
//   BatchInferActions(players, states, deterministic, temperature)
//
// The obs builder and the action parser are recognised by exact dynamic type, as EnvSetGPU.hpp recognises them
// (AdvancedObs / DefaultObs / DefaultObsPadded, DefaultAction: the kernels' own); anything else, useGPU = false
// and an obsSize that is not the builder's width are refused by name.  The models are <modelsFolder>/POLICY.lt and,
// with a shared head, SHARED_HEAD.lt, read by the loader of the guiding policy (GigaLearn.hpp); a missing file is an
// error naming it.  A folder whose RUNNING_STATS.json holds an obs statistic (standardizeObs) is refused: the unit
// does not standardise.
//
// Deviations from the reference.  It samples from libtorch's global generator; here the draw of row i of call k is a
// function of (seed, i, k): two units with the same seed and the same calls give the same actions.  Its forward is
// fp32 (InferActionsFromModels with halfPrec = false); here the default is the engine's bf16 inference, what the
// policy acted with while it was trained; halfPrecision = false selects the fp32 forward.
#pragma once
#include "../../include/rlgpu_infer_unit.h"
#include "GigaLearn.hpp"

namespace GGL {

namespace detail {
inline void St(float* f, const RLGC::Vec& v) {
    f[0] = v.x;
    f[1] = v.y;
    f[2] = v.z;
}
inline void StRot(float* m, const RLGC::RotMat& r) {
    St(m, r.forward);
    St(m + 3, r.right);
    St(m + 6, r.up);
}

// The record of a GameState: the inverse of RLGC::FillGameState (EnvSetGPU.hpp)
inline void ToRecord(const RLGC::GameState& gs, rlgpu_gamestate& g) {
    std::memset(&g, 0, sizeof g);
    if (gs.players.size() != RLGPU_CARS)
        throw std::invalid_argument("InferUnit: a GameState of " + std::to_string(gs.players.size()) +
                                    " players (the engine's builders are 2v2: 4 players)");
    auto pads = [&](const auto& v, auto* dst, const char* what) {
        if (v.size() != RLGPU_PADS)
            throw std::invalid_argument(std::string("InferUnit: GameState::") + what + " has " + std::to_string(v.size()) +
                                        " entries, not " + std::to_string(RLGPU_PADS));
        for (int i = 0; i < RLGPU_PADS; i++) dst[i] = v[i];
    };
    pads(gs.boostPads, g.boost_pads, "boostPads");
    pads(gs.boostPadsInv, g.boost_pads_inv, "boostPadsInv");
    pads(gs.boostPadTimers, g.boost_pad_timers, "boostPadTimers");
    pads(gs.boostPadTimersInv, g.boost_pad_timers_inv, "boostPadTimersInv");
    g.delta_time = gs.deltaTime;
    g.goal_scored = gs.goalScored;
    g.last_touch_car_id = gs.lastTouchCarID;
    g.last_tick_count = gs.lastTickCount;
    St(g.ball.pos, gs.ball.pos);
    StRot(g.ball.rot, gs.ball.rotMat);
    St(g.ball.vel, gs.ball.vel);
    St(g.ball.ang_vel, gs.ball.angVel);
    for (int i = 0; i < RLGPU_CARS; i++) {
        const RLGC::Player& p = gs.players[i];
        rlgpu_player_state& s = g.players[i];
        rlgpu_car_state& c = s.car;
        St(c.pos, p.pos);
        StRot(c.rot, p.rotMat);
        St(c.vel, p.vel);
        St(c.ang_vel, p.angVel);
        c.is_on_ground = p.isOnGround;
        for (int w = 0; w < 4; w++) c.wheels_with_contact[w] = p.wheelsWithContact[w];
        c.has_jumped = p.hasJumped;
        c.has_double_jumped = p.hasDoubleJumped;
        c.has_flipped = p.hasFlipped;
        St(c.flip_rel_torque, p.flipRelTorque);
        c.jump_time = p.jumpTime;
        c.flip_time = p.flipTime;
        c.is_flipping = p.isFlipping;
        c.is_jumping = p.isJumping;
        c.air_time = p.airTime;
        c.air_time_since_jump = p.airTimeSinceJump;
        c.boost = p.boost;
        c.time_spent_boosting = p.timeSpentBoosting;
        c.is_supersonic = p.isSupersonic;
        c.supersonic_time = p.supersonicTime;
        c.handbrake_val = p.handbrakeVal;
        c.is_auto_flipping = p.isAutoFlipping;
        c.auto_flip_timer = p.autoFlipTimer;
        c.auto_flip_torque_scale = p.autoFlipTorqueScale;
        c.world_contact_has_contact = p.worldContact.hasContact;
        St(c.world_contact_normal, p.worldContact.contactNormal);
        c.car_contact_other_car_id = p.carContact.otherCarID;
        c.car_contact_cooldown_timer = p.carContact.cooldownTimer;
        c.is_demoed = p.isDemoed;
        c.demo_respawn_timer = p.demoRespawnTimer;
        c.ball_hit_is_valid = p.ballHitInfo.isValid;
        St(c.ball_hit_relative_pos_on_ball, p.ballHitInfo.relativePosOnBall);
        St(c.ball_hit_ball_pos, p.ballHitInfo.ballPos);
        St(c.ball_hit_extra_hit_vel, p.ballHitInfo.extraHitVel);
        c.ball_hit_tick_count_when_hit = (int64_t)p.ballHitInfo.tickCountWhenHit;
        c.ball_hit_tick_count_when_extra_impulse_applied = (int64_t)p.ballHitInfo.tickCountWhenExtraImpulseApplied;
        const float lc[8] = {p.lastControls.throttle, p.lastControls.steer, p.lastControls.pitch, p.lastControls.yaw,
                             p.lastControls.roll, (float)p.lastControls.jump, (float)p.lastControls.boost,
                             (float)p.lastControls.handbrake};
        std::memcpy(c.last_controls, lc, sizeof lc);
        s.index = i;
        s.car_id = p.carId;
        s.team = (int32_t)p.team;
        s.events[0] = p.eventState.goal;
        s.events[1] = p.eventState.save;
        s.events[2] = p.eventState.assist;
        s.events[3] = p.eventState.shot;
        s.events[4] = p.eventState.shotPass;
        s.events[5] = p.eventState.bump;
        s.events[6] = p.eventState.bumped;
        s.events[7] = p.eventState.demo;
        s.events[8] = p.eventState.demoed;
        s.ball_touched_step = p.ballTouchedStep;
        s.ball_touched_tick = p.ballTouchedTick;
        for (int k = 0; k < 8; k++) s.prev_action[k] = p.prevAction[k];
    }
}
}  // namespace detail

class InferUnit {
public:
    RLGC::ObsBuilder* obsBuilder;
    int obsSize;
    RLGC::ActionParser* actionParser;
    bool useGPU;

    // seed: the sampler's Philox key and DefaultObsPadded's shuffle key; halfPrecision: see the header comment
    InferUnit(RLGC::ObsBuilder* obsBuilder, int obsSize, RLGC::ActionParser* actionParser, PartialModelConfig sharedHeadConfig,
              PartialModelConfig policyConfig, std::filesystem::path modelsFolder, bool useGPU = true, uint64_t seed = 0,
              bool halfPrecision = true)
        : obsBuilder(obsBuilder), obsSize(obsSize), actionParser(actionParser), useGPU(useGPU) {
        using namespace RLGC;
        if (!obsBuilder || !actionParser) throw std::invalid_argument("InferUnit: null obs builder or action parser");
        if (!useGPU) throw std::invalid_argument("InferUnit: useGPU = false (the engine has no CPU inference path)");
        if (typeid(*actionParser) != typeid(DefaultAction))
            throw std::invalid_argument(std::string("InferUnit: action parser ") + typeid(*actionParser).name() +
                                        " has no device code (DefaultAction only)");
        rlgpu_infer_unit_config uc{};
        const std::type_info& t = typeid(*obsBuilder);
        if (t == typeid(AdvancedObs)) {
            uc.obs_builder = RLGPU_OBS_ADVANCED;
        } else if (t == typeid(DefaultObs) || t == typeid(DefaultObsPadded)) {
            const DefaultObs* d = static_cast<const DefaultObs*>(obsBuilder);
            uc.obs_builder = t == typeid(DefaultObsPadded) ? RLGPU_OBS_DEFAULT_PADDED : RLGPU_OBS_DEFAULT;
            if (t == typeid(DefaultObsPadded)) uc.obs_max_players = static_cast<const DefaultObsPadded*>(obsBuilder)->maxPlayers;
            for (int i = 0; i < 3; i++) uc.obs_pos_coef[i] = d->posCoef[i];
            uc.obs_vel_coef = d->velCoef;
            uc.obs_ang_vel_coef = d->angVelCoef;
        } else {
            throw std::invalid_argument(std::string("InferUnit: obs builder ") + t.name() +
                                        " has no device code (AdvancedObs, DefaultObs or DefaultObsPadded only)");
        }
        uc.obs_seed = seed;
        const int width = rlgpu_obs_builder_size(uc.obs_builder, uc.obs_max_players);
        if (width < 0) throw std::invalid_argument(std::string("InferUnit: ") + rlgpu_last_error());
        if (width != obsSize)
            throw std::invalid_argument("InferUnit: obsSize " + std::to_string(obsSize) + " is not the obs builder's width " +
                                        std::to_string(width));
        if (!policyConfig.IsValid()) throw std::invalid_argument("InferUnit: the policy config has no layers");
        const bool shared = sharedHeadConfig.IsValid();
        if (shared && (sharedHeadConfig.activationType != policyConfig.activationType ||
                       sharedHeadConfig.addLayerNorm != policyConfig.addLayerNorm))
            throw std::invalid_argument("InferUnit: the shared head and the policy differ in activationType or addLayerNorm "
                                        "(the engine's models share both)");
        if (std::filesystem::exists(modelsFolder / "RUNNING_STATS.json") &&
            detail::ReadFile(modelsFolder / "RUNNING_STATS.json").find("\"obs_stat\"") != std::string::npos)
            throw std::invalid_argument("InferUnit: " + modelsFolder.string() + " was trained with standardizeObs (its "
                                        "RUNNING_STATS.json holds an obs_stat), and the unit does not standardise observations");

        rlgpu_ppo_config c{};
        c.obs_size = obsSize;
        c.num_actions = RLGPU_ACTIONS;
        auto layers = [](const PartialModelConfig& m, int32_t* dst, int32_t& n, const char* what) {
            if (m.layerSizes.size() > RLGPU_MAX_LAYERS)
                throw std::invalid_argument(std::string("InferUnit: more than 8 layers in the ") + what + " config");
            n = (int32_t)m.layerSizes.size();
            for (int i = 0; i < n; i++) dst[i] = m.layerSizes[i];
        };
        layers(policyConfig, c.policy_layers, c.n_policy_layers, "policy");
        if (shared) layers(sharedHeadConfig, c.shared_layers, c.n_shared_layers, "shared head");
        c.critic_layers[0] = 8;  // the handle wants a critic; the unit never runs it
        c.n_critic_layers = 1;
        const ModelActivationType at = policyConfig.activationType;
        c.activation = at == ModelActivationType::RELU      ? RLGPU_ACT_RELU
                       : at == ModelActivationType::SIGMOID ? RLGPU_ACT_SIGMOID
                       : at == ModelActivationType::TANH    ? RLGPU_ACT_TANH
                                                            : RLGPU_ACT_LEAKY_RELU;
        c.layer_norm = policyConfig.addLayerNorm;
        c.leaky_slope = 0.01f;
        c.policy_lr = c.critic_lr = 1e-4f;
        c.beta1 = 0.9f;
        c.beta2 = 0.999f;
        c.eps = 1e-8f;
        c.clip_range = 0.2f;
        c.max_grad_norm = 0.5f;
        c.max_rows = 4096;
        c.seed = seed;
        c.train_gemm = RLGPU_GEMM_F16X3;
        c.infer_fp16 = halfPrecision ? RLGPU_INFER_BF16 : RLGPU_INFER_F32;
        RLGC::RlgpuCheck(rlgpu_ppo_create(&c, &ppo_), "InferUnit: models");
        try {
            const char* an = at == ModelActivationType::RELU      ? "relu"
                             : at == ModelActivationType::SIGMOID ? "sigmoid"
                             : at == ModelActivationType::TANH    ? "tanh"
                                                                  : "leaky_relu";
            const int feat = shared ? sharedHeadConfig.layerSizes.back() : obsSize;
            std::vector<ModelSpec> models{{0, "policy", feat, RLGPU_ACTIONS, policyConfig.layerSizes, policyConfig.addLayerNorm, an}};
            if (shared) models.push_back({2, "shared_head", obsSize, 0, sharedHeadConfig.layerSizes, policyConfig.addLayerNorm, an});
            float* params = nullptr;
            float* grads = nullptr;
            int64_t total = 0;
            RLGC::RlgpuCheck(rlgpu_ppo_buffers(ppo_, &params, &grads, &total), "InferUnit: buffers");
            for (const ModelSpec& m : models) {  // Learner::LoadGuidingPolicy's loader
                const std::filesystem::path p = modelsFolder / m.FileName();
                if (!std::filesystem::exists(p)) throw std::runtime_error("InferUnit: " + p.string() + " does not exist");
                const auto tmp = detail::TempFile("infer_unit.f32");
                std::vector<std::string> a{"model-load", p.string(), tmp.string()};
                for (auto& s : m.HelperShape()) a.push_back(s);
                detail::RunHelper(a);
                const std::string raw = detail::ReadFile(tmp);
                std::filesystem::remove(tmp);
                int64_t off = 0, cnt = 0;
                RLGC::RlgpuCheck(rlgpu_ppo_model_range(ppo_, m.index, &off, &cnt), "InferUnit: model range");
                if ((int64_t)raw.size() != cnt * 4)
                    throw std::runtime_error("InferUnit: " + p.string() + " has different size than the configured model");
                detail::HipOk(hipMemcpy(params + off, raw.data(), raw.size(), hipMemcpyHostToDevice), "InferUnit: parameters");
            }
            RLGC::RlgpuCheck(rlgpu_ppo_refresh_half(ppo_, nullptr), "InferUnit: refresh");
            detail::HipOk(hipDeviceSynchronize(), "InferUnit: refresh");
            RLGC::RlgpuCheck(rlgpu_infer_unit_create(&uc, ppo_, &unit_), "InferUnit");
        } catch (...) {
            rlgpu_ppo_destroy(ppo_);
            throw;
        }
    }
    InferUnit(const InferUnit&) = delete;
    InferUnit& operator=(const InferUnit&) = delete;
    ~InferUnit() {
        if (unit_) rlgpu_infer_unit_destroy(unit_);
        if (ppo_) rlgpu_ppo_destroy(ppo_);
    }

    // the one-launch kernel instead of rows + inference + parse (off by default; rlgpu_infer_unit_set_one_launch)
    void SetOneLaunch(bool on) { RLGC::RlgpuCheck(rlgpu_infer_unit_set_one_launch(unit_, on), "InferUnit"); }
    bool OneLaunch() const { return rlgpu_infer_unit_one_launch(unit_) != 0; }

    RLGC::Action InferAction(const RLGC::Player& player, const RLGC::GameState& state, bool deterministic, float temperature = 1) {
        return BatchInferActions({player}, {state}, deterministic, temperature)[0];
    }

    std::vector<RLGC::Action> BatchInferActions(const std::vector<RLGC::Player>& players, const std::vector<RLGC::GameState>& states,
                                                bool deterministic, float temperature = 1) {
        if (players.empty() || players.size() != states.size())
            throw std::invalid_argument("InferUnit: " + std::to_string(players.size()) + " players for " +
                                        std::to_string(states.size()) + " states (one state per player, at least one)");
        const int n = (int)players.size();
        recs_.resize(n);
        stateOfRow_.resize(n);
        playerOfRow_.resize(n);
        for (int i = 0; i < n; i++) {
            detail::ToRecord(states[i], recs_[i]);
            stateOfRow_[i] = i;
            playerOfRow_[i] = -1;
            for (int q = 0; q < RLGPU_CARS; q++)
                if (states[i].players[q].carId == players[i].carId) playerOfRow_[i] = q;
            if (playerOfRow_[i] < 0)
                throw std::invalid_argument("InferUnit: player " + std::to_string(i) + " (carId " + std::to_string(players[i].carId) +
                                            ") is not in its GameState");
        }
        index_.resize(n);
        parsed_.resize((size_t)n * 8);
        RLGC::RlgpuCheck(rlgpu_infer_unit_infer(unit_, recs_.data(), n, stateOfRow_.data(), playerOfRow_.data(), n, 0,
                                                deterministic ? 1 : 0, temperature, calls_++, index_.data(), nullptr,
                                                parsed_.data(), nullptr),
                         "InferUnit");
        std::vector<RLGC::Action> out(n);
        for (int i = 0; i < n; i++)
            for (int k = 0; k < 8; k++) out[i][k] = parsed_[(size_t)i * 8 + k];
        return out;
    }

    const std::vector<int32_t>& LastActionIndices() const { return index_; }

private:
    rlgpu_ppo* ppo_ = nullptr;
    rlgpu_infer_unit* unit_ = nullptr;
    uint64_t calls_ = 0;
    std::vector<rlgpu_gamestate> recs_;
    std::vector<int32_t> stateOfRow_, playerOfRow_, index_;
    std::vector<float> parsed_;
};

}  // namespace GGL

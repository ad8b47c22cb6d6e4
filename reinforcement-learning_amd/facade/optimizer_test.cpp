// optimizer_test.cpp -- ModelConfig::optimType through the trainer facade (tests/test_optimizer_facade.py).
//
//   optimizer_test refuse             (CPU) ValidateConfig: every ModelOptimType passes when all models share it, and a
//                                     config whose models differ is refused by name.
//   optimizer_test train NAME DIR     (GPU) a GGL::Learner whose models all use optimType NAME (adamw, adam, adagrad,
//                                     rmsprop, magsgd) constructs, runs one iteration that moves every model's
//                                     parameters to finite values, and saves a checkpoint under DIR; a second Learner
//                                     loads it and holds the same parameters.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "GigaLearn.hpp"

using namespace RLGC;

static int g_fail = 0;
#define CHECK(c, ...)                                        \
    do {                                                     \
        if (!(c)) {                                          \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            g_fail++;                                        \
        }                                                    \
    } while (0)

static EnvCreateResult DeviceEnv(int) {
    EnvCreateResult r;
    r.rewards = {{new VelocityPlayerToBallReward(), 4.f}, {new ZeroSumReward(new GoalReward(), 1), 150}};
    r.terminalConditions = {new NoTouchCondition(8), new GoalScoreCondition()};
    r.actionParser = new DefaultAction();
    r.obsBuilder = new AdvancedObs();
    r.stateSetter = new KickoffState();
    return r;
}

static GGL::LearnerConfig Config(GGL::ModelOptimType t) {
    using namespace GGL;
    LearnerConfig cfg = {};
    cfg.numGames = 4;
    cfg.randomSeed = 7;
    cfg.ppo.tsPerItr = 8 * 4 * cfg.numGames;
    cfg.ppo.batchSize = cfg.ppo.tsPerItr;
    cfg.ppo.miniBatchSize = cfg.ppo.tsPerItr;
    cfg.ppo.maxEpisodeDuration = 2.0;
    cfg.ppo.sharedHead.layerSizes = {64};
    cfg.ppo.policy.layerSizes = {64};
    cfg.ppo.critic.layerSizes = {64};
    for (PartialModelConfig* m : {&cfg.ppo.policy, &cfg.ppo.critic, &cfg.ppo.sharedHead}) {
        m->activationType = ModelActivationType::LEAKY_RELU;
        m->optimType = t;
    }
    cfg.checkpointFolder.clear();
    cfg.trainAgainstOldVersions = false;
    cfg.sendMetrics = false;
    return cfg;
}

static int Refuse() {
    using namespace GGL;
    for (ModelOptimType t : {ModelOptimType::ADAM, ModelOptimType::ADAMW, ModelOptimType::ADAGRAD, ModelOptimType::RMSPROP,
                             ModelOptimType::MAGSGD}) {
        try {
            Learner::ValidateConfig(Config(t));
        } catch (const std::exception& e) {
            CHECK(false, "optimType %d refused: %s", (int)t, e.what());
        }
    }
    LearnerConfig mixed = Config(ModelOptimType::MAGSGD);
    mixed.ppo.critic.optimType = ModelOptimType::ADAMW;
    std::string what;
    try {
        Learner::ValidateConfig(mixed);
    } catch (const std::invalid_argument& e) {
        what = e.what();
    }
    CHECK(what.find("every model must use the same optimType") != std::string::npos, "mixed optimTypes: \"%s\"", what.c_str());
    std::printf("refuse: %s\n", g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
}

static int Train(const std::string& name, const char* dir) {
    using namespace GGL;
    ModelOptimType t;
    if (name == "adamw") t = ModelOptimType::ADAMW;
    else if (name == "adam") t = ModelOptimType::ADAM;
    else if (name == "adagrad") t = ModelOptimType::ADAGRAD;
    else if (name == "rmsprop") t = ModelOptimType::RMSPROP;
    else if (name == "magsgd") t = ModelOptimType::MAGSGD;
    else return 2;
    LearnerConfig cfg = Config(t);
    cfg.checkpointFolder = dir;
    cfg.tsPerSave = 1ll << 40;  // Save() is called here, not by Iterate
    LearnerGPUOptions o;
    o.quitKeyThread = false;
    o.displayReport = false;
    std::vector<std::vector<float>> after;
    {
        Learner A(DeviceEnv, cfg, nullptr, o);
        std::vector<std::vector<float>> before;
        for (auto& m : A.models) before.push_back(A.ModelParams(m.index));
        Report r;
        A.Iterate(r);
        for (size_t k = 0; k < A.models.size(); k++) {
            const std::vector<float> p = A.ModelParams(A.models[k].index);
            size_t moved = 0, finite = 0;
            for (size_t i = 0; i < p.size(); i++) {
                moved += p[i] != before[k][i];
                finite += std::isfinite(p[i]) ? 1 : 0;
            }
            CHECK(finite == p.size(), "%s: %zu of %zu parameters are not finite", A.models[k].name, p.size() - finite, p.size());
            CHECK(moved > p.size() / 2, "%s: only %zu of %zu parameters moved", A.models[k].name, moved, p.size());
            after.push_back(p);
        }
        A.Save();
    }
    Learner B(DeviceEnv, cfg, nullptr, o);  // the constructor loads the checkpoint
    for (size_t k = 0; k < B.models.size(); k++) {
        const std::vector<float> p = B.ModelParams(B.models[k].index);
        CHECK(p.size() == after[k].size() && !std::memcmp(p.data(), after[k].data(), p.size() * 4),
              "%s: the loaded parameters differ from the saved ones", B.models[k].name);
    }
    std::printf("train %s: %s\n", name.c_str(), g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "refuse")) return Refuse();
        if (argc >= 4 && !std::strcmp(argv[1], "train")) return Train(argv[2], argv[3]);
    } catch (const std::exception& e) {
        std::printf("FAIL: exception %s\n", e.what());
        return 1;
    }
    std::printf("usage: optimizer_test refuse | train NAME DIR\n");
    return 2;
}

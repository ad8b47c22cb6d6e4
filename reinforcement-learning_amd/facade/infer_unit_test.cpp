// infer_unit_test.cpp -- GGL::InferUnit through the compat include path, as a bot's code sees it
// (tests/test_infer_unit_gpu.py):
//   rlgpu_infer_unit_test run <models folder> <states file> <policy layers a,b,..> <shared head layers a,b,.. | ->
//       reads rlgpu_gamestate records, prints InferAction of player 2 of state 3 and BatchInferActions of every
//       player of every state (deterministic), as "one: 8 floats" / "row i: 8 floats";
//   rlgpu_infer_unit_test refuse <models folder>
//       prints the message of every refused construction.
#include <GigaLearnCPP/Util/InferUnit.h>
#include <RLGymCPP/ActionParsers/DefaultAction.h>
#include <RLGymCPP/OBSBuilders/AdvancedObs.h>
#include <RLGymCPP/OBSBuilders/DefaultObs.h>

#include <cstdio>
#include <fstream>
#include <sstream>

namespace {
std::vector<int> Layers(const std::string& s) {
    std::vector<int> v;
    if (s == "-") return v;
    std::stringstream ss(s);
    std::string tok;
    while (std::getline(ss, tok, ',')) v.push_back(std::stoi(tok));
    return v;
}
void Print(const char* tag, int i, const RLGC::Action& a) {
    std::printf("%s %d:", tag, i);
    for (size_t k = 0; k < RLGC::Action::ELEM_AMOUNT; k++) std::printf(" %g", (double)a[k]);
    std::printf("\n");
}
class MyObs : public RLGC::AdvancedObs {};

template <class F>
void Refused(const char* what, F&& f) {
    try {
        f();
        std::printf("%s: accepted\n", what);
    } catch (const std::exception& e) {
        std::printf("%s: %s\n", what, e.what());
    }
}
}  // namespace

int main(int argc, char** argv) {
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        GGL::PartialModelConfig policy, shared;
        policy.activationType = shared.activationType = GGL::ModelActivationType::LEAKY_RELU;
        RLGC::AdvancedObs obs;
        RLGC::DefaultAction parser;
        if (mode == "refuse" && argc == 3) {
            policy.layerSizes = {32};
            MyObs mine;
            RLGC::DefaultObs dflt;
            Refused("custom obs builder", [&] { GGL::InferUnit(&mine, 167, &parser, shared, policy, argv[2]); });
            Refused("useGPU false", [&] { GGL::InferUnit(&obs, 167, &parser, shared, policy, argv[2], false); });
            Refused("wrong obsSize", [&] { GGL::InferUnit(&dflt, 167, &parser, shared, policy, argv[2]); });
            Refused("missing model", [&] { GGL::InferUnit(&obs, 167, &parser, shared, policy, argv[2]); });
            return 0;
        }
        if (mode != "run" || argc != 6) {
            std::fprintf(stderr, "usage: rlgpu_infer_unit_test run <folder> <states> <policy layers> <shared layers | -> | refuse <folder>\n");
            return 2;
        }
        policy.layerSizes = Layers(argv[4]);
        shared.layerSizes = Layers(argv[5]);
        std::ifstream f(argv[3], std::ios::binary);
        std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (raw.empty() || raw.size() % sizeof(rlgpu_gamestate)) throw std::runtime_error("bad states file");
        const size_t ns = raw.size() / sizeof(rlgpu_gamestate);
        std::vector<RLGC::GameState> states(ns);
        for (size_t s = 0; s < ns; s++) {
            rlgpu_gamestate g;
            std::memcpy(&g, raw.data() + s * sizeof g, sizeof g);
            RLGC::FillGameState(states[s], g, nullptr, false);
        }
        GGL::InferUnit unit(&obs, 167, &parser, shared, policy, argv[2], true, 5);
        std::printf("one launch: %d\n", (int)unit.OneLaunch());
        Print("one", 0, unit.InferAction(states[3].players[2], states[3], true, 1.0f));
        std::vector<RLGC::Player> ps;
        std::vector<RLGC::GameState> ss;
        for (size_t s = 0; s < ns; s++)
            for (const RLGC::Player& p : states[s].players) {
                ps.push_back(p);
                ss.push_back(states[s]);
            }
        const std::vector<RLGC::Action> acts = unit.BatchInferActions(ps, ss, true, 1.0f);
        for (size_t i = 0; i < acts.size(); i++) Print("row", (int)i, acts[i]);
        RLGC::Player ghost = ps[0];
        ghost.carId = 77;
        Refused("absent player", [&] { unit.InferAction(ghost, states[0], true, 1.0f); });
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "infer_unit_test: %s\n", e.what());
        return 1;
    }
}

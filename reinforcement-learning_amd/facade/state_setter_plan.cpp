// rlgpu_state_setter_plan -- prints what the facade makes of EnvCreateResult::stateSetter (EnvSetGPU.hpp
// TranslatePlugins): one "name: setter T flags F children N" line per case, then a "  child i: type T weight W
// flags F" line per CombinedState child; a refused setter prints "name: refused: <message>".  No GPU needed.
// Cases: kickoff, fuzzed, the 8 RandomState flag sets, a CombinedState of three children, arenas whose lists
// differ (RequireSamePlan), and what stays refused: a nested CombinedState, a user setter class, too many
// children, a bad weight.
#include <cstdio>
#include <memory>

#include "EnvSetGPU.hpp"

using namespace RLGC;

namespace {
class UserSetter : public StateSetter {};

void Print(const char* name, StateSetter* s) {
    EnvCreateResult r;
    r.stateSetter = s;
    try {
        const PluginPlan p = TranslatePlugins(r);
        std::printf("%s: setter %d flags %d children %d\n", name, p.stateSetter, p.stateSetterFlags, (int)p.stateSetters.size());
        for (size_t i = 0; i < p.stateSetters.size(); i++)
            std::printf("  child %d: type %d weight %.9g flags %d\n", (int)i, p.stateSetters[i].type,
                        (double)p.stateSetters[i].weight, p.stateSetters[i].flags);
        rlgpu_envset_config c{};
        p.FillStateSetter(c);
        if (c.state_setter != p.stateSetter || c.n_state_setters != (int)p.stateSetters.size() ||
            (c.n_state_setters > 0) != (c.state_setters != nullptr))
            std::printf("%s: config fill mismatch\n", name);
    } catch (const std::invalid_argument& e) {
        std::printf("%s: refused: %s\n", name, e.what());
    }
}
}  // namespace

int main() {
    KickoffState kick;
    FuzzedKickoffState fuzz;
    UserSetter user;
    Print("kickoff", &kick);
    Print("fuzzed", &fuzz);
    for (int f = 0; f < 8; f++) {
        RandomState r((f & 1) != 0, (f & 2) != 0, (f & 4) != 0);
        char name[32];
        std::snprintf(name, sizeof name, "random%d", f);
        Print(name, &r);
    }
    RandomState air(true, true, false);
    CombinedState three({{&kick, 1.f}, {&air, 2.f}, {&fuzz, 0.5f}});
    Print("combined3", &three);
    CombinedState nested({{&kick, 1.f}, {&three, 1.f}});
    Print("nested", &nested);
    Print("user", &user);
    CombinedState withUser({{&kick, 1.f}, {&user, 1.f}});
    Print("combined_user", &withUser);
    std::vector<std::pair<StateSetter*, float>> nine(RLGPU_MAX_STATE_SETTERS + 1, {&kick, 1.f});
    CombinedState many(nine);
    Print("combined9", &many);
    try {
        CombinedState bad({{&kick, 1.f}, {&air, -1.f}});
        std::printf("bad_weight: accepted\n");
    } catch (const std::invalid_argument& e) {
        std::printf("bad_weight: refused: %s\n", e.what());
    }
    try {
        CombinedState none({});
        std::printf("empty: accepted\n");
    } catch (const std::invalid_argument& e) {
        std::printf("empty: refused: %s\n", e.what());
    }
    // arenas whose lists differ: the weights, the flags, the child count
    const auto same = [](StateSetter* a, StateSetter* b) {
        EnvCreateResult ra, rb;
        ra.stateSetter = a;
        rb.stateSetter = b;
        try {
            RequireSamePlan(TranslatePlugins(ra), TranslatePlugins(rb), 1);
            return true;
        } catch (const std::invalid_argument&) {
            return false;
        }
    };
    RandomState ground(true, true, true);
    CombinedState three2({{&kick, 1.f}, {&air, 2.f}, {&fuzz, 0.5f}});
    CombinedState weights({{&kick, 1.f}, {&air, 3.f}, {&fuzz, 0.5f}});
    CombinedState flags({{&kick, 1.f}, {&ground, 2.f}, {&fuzz, 0.5f}});
    CombinedState two({{&kick, 1.f}, {&air, 2.f}});
    std::printf("same: equal %d weights %d flags %d count %d random_flags %d kickoff_vs_random %d\n", (int)same(&three, &three2),
                (int)same(&three, &weights), (int)same(&three, &flags), (int)same(&three, &two), (int)same(&air, &ground),
                (int)same(&kick, &air));
    return 0;
}

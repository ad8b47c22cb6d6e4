// rlgpu_obs_builder_plan -- prints what the facade makes of EnvCreateResult::obsBuilder (EnvSetGPU.hpp
// TranslatePlugins through EnvSetGPU::CreateEnvs, an EnvCreateFn called once per arena): one "name: kind K width W
// max_players M coef a b c d e" line per case; a refused builder prints "name: refused: <message>".  No GPU needed.
// Cases: no builder, AdvancedObs, DefaultObs with the default and with other coefficients, DefaultObsPadded(2) and
// (3), and what stays refused: DefaultObsPadded(1) and (4), a user's subclass of DefaultObs (an AddPlayerToObs
// override), a user's ObsBuilder class, arenas whose builders differ.
#include <cstdio>
#include <functional>

#include "EnvSetGPU.hpp"

using namespace RLGC;

namespace {
class UserDefaultObs : public DefaultObs {};  // stands for an AddPlayerToObs override
class UserObs : public ObsBuilder {};

void Print(const char* name, const std::function<ObsBuilder*(int)>& make) {
    EnvSetConfig c{};
    c.envCreateFn = [&](int index) {
        EnvCreateResult r;
        r.obsBuilder = make(index);
        return r;
    };
    c.numArenas = 2;
    c.tickSkip = 8;
    c.actionDelay = 7;
    std::vector<EnvCreateResult> results;
    try {
        const PluginPlan p = EnvSetGPU::CreateEnvs(c, results);
        rlgpu_envset_config e{};
        p.FillObsBuilder(e);
        std::printf("%s: kind %d width %d max_players %d coef %.9g %.9g %.9g %.9g %.9g\n", name, e.obs_builder, p.obsSize,
                    e.obs_max_players, (double)e.obs_pos_coef[0], (double)e.obs_pos_coef[1], (double)e.obs_pos_coef[2],
                    (double)e.obs_vel_coef, (double)e.obs_ang_vel_coef);
    } catch (const std::invalid_argument& x) {
        std::printf("%s: refused: %s\n", name, x.what());
    }
    for (auto& r : results) delete r.obsBuilder;
}
}  // namespace

int main() {
    Print("none", [](int) { return (ObsBuilder*)nullptr; });
    Print("advanced", [](int) { return new AdvancedObs(); });
    Print("default", [](int) { return new DefaultObs(); });
    Print("default_coef", [](int) { return new DefaultObs(Vec(1 / 4000.f, 1 / 5000.f, 1 / 2000.f), 1 / 2000.f, 0.25f); });
    Print("padded2", [](int) { return new DefaultObsPadded(2); });
    Print("padded3", [](int) { return new DefaultObsPadded(3); });
    Print("padded1", [](int) { return new DefaultObsPadded(1); });
    Print("padded4", [](int) { return new DefaultObsPadded(4); });
    Print("subclass", [](int) { return new UserDefaultObs(); });
    Print("user", [](int) { return new UserObs(); });
    Print("differ", [](int i) { return i ? (ObsBuilder*)new DefaultObsPadded(2) : (ObsBuilder*)new DefaultObs(); });
    Print("differ_coef", [](int i) { return new DefaultObs(Vec(1 / 4096.f, 1 / 5120.f, 1 / 2044.f), i ? 0.5f : 1 / 2300.f); });
    return 0;
}

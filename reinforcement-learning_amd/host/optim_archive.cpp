// optim_archive.cpp -- <NAME>_OPTIM.lt, the reference's optimizer checkpoint (GGL::Model::Save / Load,
// GigaLearnCPP/src/private/GigaLearnCPP/Util/Models.cpp:116-126,168-186): written and read by libtorch's
// own torch::optim::AdamW::save / load through a torch::serialize archive, exactly as the reference
// does, so the file is byte-for-byte the format its Model::Load expects (state keyed by parameter
// address, mapped back by parameter order on load).  Built against the libtorch of the installed
// PyTorch (plumbing); rlgpu/checkpoint.py drives it.
//
// It also writes and reads the model archives <NAME>.lt (GGL::Model::Save / Load, Models.cpp:116-166): the
// Sequential GGL::Model builds (Models.cpp:7-33: per hidden layer Linear, LayerNorm unless addLayerNorm is false,
// the activation of AddActivationFunc; then the output Linear unless out is 0, the shared head's addOutputLayer =
// false) saved with torch::save(seq, stream) and
// read with torch::load(seq, stream), with Model::Load's parameter-size check.
//
// usage: rlgpu_optim_lt save <out.lt> <state.f32> <step> <lr> <beta1> <beta2> <eps> <weight_decay> <shape>... [--optimizer NAME]
//        rlgpu_optim_lt load <in.lt> <state.f32> <shape>... [--optimizer NAME]
//        rlgpu_optim_lt model-save <out.lt> <params.f32> <obs> <out> <h1> [h2 ...] [--no-layer-norm] [--activation NAME]
//        rlgpu_optim_lt model-load <in.lt> <params.f32> <obs> <out> <h1> [h2 ...] [--no-layer-norm] [--activation NAME]
//   --no-layer-norm: ModelConfig::addLayerNorm = false (no LayerNorm modules: the module indices, the archive's
//   keys, shift); --activation relu | leaky_relu (default) | sigmoid | tanh: the archive holds no trace of it.
//   params.f32: the model's parameters flat in parameters() order (model-load writes them).
//   shape: dimensions joined by 'x' (e.g. 384x167), one per model parameter in parameters() order;
//   state.f32: every parameter's exp_avg (flat, parameter order), then every exp_avg_sq.  load writes
//   it preceded by the step as an int64 (0 and zero moments for parameters without state).
//   --optimizer adamw | adam | adagrad | rmsprop | magsgd (MakeOptimizer, Models.h:40-56; default adamw, and adam is
//   written and read as adamw, as it always was): the libtorch class that writes / reads the archive.  state.f32 keeps
//   its layout: torch::optim::Adagrad's sum and RMSprop's square_avg (no momentum, not centered: those buffers stay
//   undefined) are the second half, the first half zeros; torch::optim::SGD at momentum 0 (MagSGD is an SGD) has no
//   state -- its file is still written, so Model::Load finds one -- and loads as step 0 and zeros.
#include <torch/torch.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

namespace {

std::vector<int64_t> parse_shape(const std::string& s) {
    std::vector<int64_t> d;
    size_t p = 0;
    while (p <= s.size()) {
        size_t q = s.find('x', p);
        if (q == std::string::npos) q = s.size();
        d.push_back(std::stoll(s.substr(p, q - p)));
        p = q + 1;
    }
    return d;
}

std::vector<torch::Tensor> make_params(char** shapes, int n) {
    std::vector<torch::Tensor> ps;
    for (int i = 0; i < n; i++) ps.push_back(torch::zeros(parse_shape(shapes[i])));
    return ps;
}

torch::nn::Sequential make_model(int obs, int out, const std::vector<int>& layers, bool layer_norm, const std::string& act) {
    torch::nn::Sequential seq;
    int last = obs;
    for (int h : layers) {
        seq->push_back(torch::nn::Linear(last, h));
        if (layer_norm) seq->push_back(torch::nn::LayerNorm(torch::nn::LayerNormOptions({(int64_t)h})));
        last = h;
        if (act == "relu") seq->push_back(torch::nn::ReLU());  // AddActivationFunc (Models.cpp:17-23)
        else if (act == "sigmoid") seq->push_back(torch::nn::Sigmoid());
        else if (act == "tanh") seq->push_back(torch::nn::Tanh());
        else seq->push_back(torch::nn::LeakyReLU());
    }
    if (out > 0) seq->push_back(torch::nn::Linear(last, out));
    return seq;
}

std::vector<int64_t> seq_sizes(torch::nn::Sequential& seq) {  // GetSeqSizes (Models.cpp:79-87)
    std::vector<int64_t> r;
    for (size_t i = 0; i < seq->size(); i++)
        for (auto& p : seq[i]->parameters()) r.push_back(p.numel());
    return r;
}

int model_mode(bool save, int argc, char** argv) {
    if (argc < 7) return 2;
    std::vector<int> layers;
    bool layer_norm = true;
    std::string act = "leaky_relu";
    for (int i = 6; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--no-layer-norm") layer_norm = false;
        else if (a == "--activation" && i + 1 < argc) act = argv[++i];
        else if (a.rfind("--", 0) == 0 || std::atoi(argv[i]) <= 0) return 2;
        else layers.push_back(std::atoi(argv[i]));
    }
    if (layers.empty() || (act != "relu" && act != "leaky_relu" && act != "sigmoid" && act != "tanh")) return 2;
    torch::nn::Sequential seq = make_model(std::atoi(argv[4]), std::atoi(argv[5]), layers, layer_norm, act);
    torch::NoGradGuard ng;
    int64_t total = 0;
    for (auto& p : seq->parameters()) total += p.numel();
    std::vector<float> buf((size_t)total);
    if (save) {
        std::ifstream in(argv[3], std::ios::binary);
        in.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)(buf.size() * sizeof(float)));
        if (!in) {
            std::cerr << "parameter file too short\n";
            return 3;
        }
        int64_t off = 0;
        for (auto& p : seq->parameters()) {
            p.copy_(torch::from_blob(buf.data() + off, p.sizes(), torch::kFloat32));
            off += p.numel();
        }
        std::ofstream out(argv[2], std::ios::binary);  // Model::Save (Models.cpp:116-120)
        torch::save(seq, out);
        return out ? 0 : 3;
    }
    const auto before = seq_sizes(seq);
    std::ifstream in(argv[2], std::ios::binary);  // Model::Load (Models.cpp:130-166)
    in >> std::noskipws;
    if (!in.good()) {
        std::cerr << "cannot open " << argv[2] << "\n";
        return 3;
    }
    torch::load(seq, in);
    if (seq_sizes(seq) != before) {
        std::cerr << "Saved model has different size than current model, cannot load model from " << argv[2] << "\n";
        return 5;
    }
    int64_t off = 0;
    for (auto& p : seq->parameters()) {
        auto c = p.to(torch::kCPU).to(torch::kFloat32).contiguous();
        std::copy(c.data_ptr<float>(), c.data_ptr<float>() + c.numel(), buf.begin() + off);
        off += p.numel();
    }
    std::ofstream out(argv[3], std::ios::binary);
    out.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)(buf.size() * sizeof(float)));
    return out ? 0 : 3;
}

// the flat state of one optimizer class: per parameter the step and one tensor (Adagrad's sum, RMSprop's square_avg),
// kept in the second half of state.f32
template <class Opt, class State, class Get>
void put_state(Opt& opt, std::vector<torch::Tensor>& ps, std::vector<float>& buf, int64_t total, int64_t step, Get span) {
    int64_t off = 0;
    for (auto& p : ps) {
        auto st = std::make_unique<State>();
        st->step(step);
        span(*st)(torch::from_blob(buf.data() + total + off, p.sizes(), torch::kFloat32).clone());
        opt.state()[p.unsafeGetTensorImpl()] = std::move(st);
        off += p.numel();
    }
}
template <class Opt, class State, class Get>
bool get_state(Opt& opt, std::vector<torch::Tensor>& ps, std::vector<float>& buf, int64_t total, int64_t& step, Get span) {
    int64_t off = 0;
    for (auto& p : ps) {
        auto it = opt.state().find(p.unsafeGetTensorImpl());
        if (it != opt.state().end()) {
            auto& st = static_cast<State&>(*it->second);
            step = st.step();
            const torch::Tensor v = span(st).to(torch::kCPU).to(torch::kFloat32).contiguous();
            if (v.numel() != p.numel()) return false;
            std::copy(v.data_ptr<float>(), v.data_ptr<float>() + v.numel(), buf.begin() + total + off);
        }
        off += p.numel();
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        // --optimizer NAME, anywhere after the mode
        std::string optimizer = "adamw";
        for (int i = 2; i + 1 < argc; i++)
            if (std::string(argv[i]) == "--optimizer") {
                optimizer = argv[i + 1];
                for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
                argc -= 2;
                break;
            }
        if (optimizer == "adam") optimizer = "adamw";
        if (optimizer != "adamw" && optimizer != "adagrad" && optimizer != "rmsprop" && optimizer != "magsgd") {
            std::cerr << "--optimizer must be adamw, adam, adagrad, rmsprop or magsgd\n";
            return 2;
        }
        if (argc < 4) return 2;
        const std::string mode = argv[1];
        if (mode == "model-save" || mode == "model-load") return model_mode(mode == "model-save", argc, argv);
        if (mode == "save") {
            if (argc < 10) return 2;
            const int64_t step = std::atoll(argv[4]);
            const double lr = std::atof(argv[5]), b1 = std::atof(argv[6]), b2 = std::atof(argv[7]), eps = std::atof(argv[8]),
                         wd = std::atof(argv[9]);
            std::vector<torch::Tensor> ps = make_params(argv + 10, argc - 10);
            int64_t total = 0;
            for (auto& p : ps) total += p.numel();
            std::vector<float> buf((size_t)(2 * total));
            std::ifstream in(argv[3], std::ios::binary);
            in.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)(buf.size() * sizeof(float)));
            if (!in) {
                std::cerr << "state file too short\n";
                return 3;
            }
            if (optimizer != "adamw") {  // MakeOptimizer(type, parameters(), lr): the class's defaults but lr
                torch::serialize::OutputArchive archive;
                if (optimizer == "adagrad") {
                    torch::optim::Adagrad opt(ps, torch::optim::AdagradOptions(lr));
                    put_state<torch::optim::Adagrad, torch::optim::AdagradParamState>(
                        opt, ps, buf, total, step, [](auto& st) { return [&st](torch::Tensor t) { st.sum(t); }; });
                    opt.save(archive);
                } else if (optimizer == "rmsprop") {
                    torch::optim::RMSprop opt(ps, torch::optim::RMSpropOptions(lr));
                    put_state<torch::optim::RMSprop, torch::optim::RMSpropParamState>(
                        opt, ps, buf, total, step, [](auto& st) { return [&st](torch::Tensor t) { st.square_avg(t); }; });
                    opt.save(archive);
                } else {
                    torch::optim::SGD opt(ps, torch::optim::SGDOptions(lr));  // MagSGD : SGD, momentum 0: no state
                    opt.save(archive);
                }
                archive.save_to(argv[2]);
                return 0;
            }
            // Model::Model: MakeOptimizer(AdamW, parameters(), lr) (Models.h:40-56)
            torch::optim::AdamW opt(ps, torch::optim::AdamWOptions(lr).betas({b1, b2}).eps(eps).weight_decay(wd));
            int64_t off = 0;
            for (auto& p : ps) {
                auto st = std::make_unique<torch::optim::AdamWParamState>();
                st->step(step);
                st->exp_avg(torch::from_blob(buf.data() + off, p.sizes(), torch::kFloat32).clone());
                st->exp_avg_sq(torch::from_blob(buf.data() + total + off, p.sizes(), torch::kFloat32).clone());
                opt.state()[p.unsafeGetTensorImpl()] = std::move(st);
                off += p.numel();
            }
            torch::serialize::OutputArchive archive;  // Model::Save (Models.cpp:122-125)
            opt.save(archive);
            archive.save_to(argv[2]);
            return 0;
        }
        if (mode == "load") {
            std::vector<torch::Tensor> ps = make_params(argv + 4, argc - 4);
            if (optimizer != "adamw") {
                int64_t step = 0, total = 0;
                for (auto& p : ps) total += p.numel();
                std::vector<float> buf((size_t)(2 * total), 0.f);
                torch::serialize::InputArchive archive;
                archive.load_from(argv[2]);
                bool ok = true;
                if (optimizer == "adagrad") {
                    torch::optim::Adagrad opt(ps, torch::optim::AdagradOptions(1e-3));
                    opt.state().clear();  // the constructor's zero sums: only what the file holds counts
                    opt.load(archive);
                    ok = get_state<torch::optim::Adagrad, torch::optim::AdagradParamState>(
                        opt, ps, buf, total, step, [](auto& st) { return st.sum(); });
                } else if (optimizer == "rmsprop") {
                    torch::optim::RMSprop opt(ps, torch::optim::RMSpropOptions(1e-3));
                    opt.load(archive);
                    ok = get_state<torch::optim::RMSprop, torch::optim::RMSpropParamState>(
                        opt, ps, buf, total, step, [](auto& st) { return st.square_avg(); });
                } else {
                    torch::optim::SGD opt(ps, torch::optim::SGDOptions(1e-3));
                    opt.load(archive);
                }
                if (!ok) {
                    std::cerr << "optimizer state does not match the parameter shapes\n";
                    return 3;
                }
                std::ofstream out(argv[3], std::ios::binary);
                out.write(reinterpret_cast<const char*>(&step), sizeof step);
                out.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)(buf.size() * sizeof(float)));
                return out ? 0 : 3;
            }
            torch::optim::AdamW opt(ps, torch::optim::AdamWOptions(1e-3));
            torch::serialize::InputArchive archive;  // Model::Load (Models.cpp:177-180)
            archive.load_from(argv[2]);
            opt.load(archive);
            int64_t step = 0, total = 0;
            for (auto& p : ps) total += p.numel();
            std::vector<float> buf((size_t)(2 * total), 0.f);
            int64_t off = 0;
            for (auto& p : ps) {
                auto it = opt.state().find(p.unsafeGetTensorImpl());
                if (it != opt.state().end()) {
                    auto& st = static_cast<torch::optim::AdamWParamState&>(*it->second);
                    step = st.step();
                    auto m = st.exp_avg().to(torch::kCPU).to(torch::kFloat32).contiguous();
                    auto v = st.exp_avg_sq().to(torch::kCPU).to(torch::kFloat32).contiguous();
                    if (m.numel() != p.numel() || v.numel() != p.numel()) {
                        std::cerr << "optimizer state does not match the parameter shapes\n";
                        return 3;
                    }
                    std::copy(m.data_ptr<float>(), m.data_ptr<float>() + m.numel(), buf.begin() + off);
                    std::copy(v.data_ptr<float>(), v.data_ptr<float>() + v.numel(), buf.begin() + total + off);
                }
                off += p.numel();
            }
            std::ofstream out(argv[3], std::ios::binary);
            out.write(reinterpret_cast<const char*>(&step), sizeof step);
            out.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)(buf.size() * sizeof(float)));
            return out ? 0 : 3;
        }
        return 2;
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 4;
    }
}

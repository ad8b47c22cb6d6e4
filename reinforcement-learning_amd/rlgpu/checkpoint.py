"""Checkpoints in the reference's on-disk format.

Reference map:
    Learner::Save / Load                 GigaLearnCPP/src/public/GigaLearnCPP/Learner.cpp:224-279
      <checkpointFolder>/<totalTimesteps>/ numbered directories, the highest one is loaded,
      checkpointsToKeep (default 8, -1 = keep all) oldest-first pruning      :236-252
    Learner::SaveStats / LoadStats       Learner.cpp:166-221  -> RUNNING_STATS.json
      {"total_timesteps", "total_iterations", "return_stat": WelfordStat::ToJSON}
    Model::Save / Load                   src/private/GigaLearnCPP/Util/Models.cpp:116-195
      <NAME>.lt = torch::save(nn::Sequential): a TorchScript archive whose submodules "0", "1", ...
      hold the Linear / LayerNorm parameters ("weight", "bias"); Load refuses a checkpoint whose
      per-parameter sizes differ (GetSeqSizes, Models.cpp:79-87, 147-166)
    Utils::FindNumberedDirs              src/public/GigaLearnCPP/Util/Utils.cpp:3-27

The model files written here are TorchScript-scripted torch.nn.Sequential modules with the same
layer order as GGL::Model (Linear [, LayerNorm], LeakyReLU per hidden layer, then the output
Linear), which libtorch's torch::load(seq, stream) reads into the reference's Sequential
(verified by tools/lt_load_check.cpp, tests/test_checkpoint.py), so a GPU-trained policy loads in
the reference's InferUnit / RLBotClient; reference-written POLICY.lt / CRITIC.lt load here.

Optimizer state: the reference writes <NAME>_OPTIM.lt with torch::optim::AdamW::save into a
torch::serialize archive (Models.cpp:116-126) and reads it back with AdamW::load (state keyed by
parameter address, mapped back by parameter order; a missing file resets the optimizer with a
warning, Models.cpp:168-186).  Here the same archives are written and read by libtorch itself
(rlgpu/rlgpu_optim_lt, host/optim_archive.cpp), so a reference checkpoint resumes with its AdamW state
and a GPU checkpoint resumes in the reference with ours.  The exact state (step, exp_avg, exp_avg_sq
in the flat torch parameter order) is also kept in RLGPU_OPTIM.safetensors, which load() prefers.

The other optimizers of ModelConfig::optimType keep their state in the same spans: Adagrad's `sum` and RMSprop's
`square_avg` in exp_avg_sq (exp_avg stays zero), MagSGD none.  Their <NAME>_OPTIM.lt is written and read by the matching
libtorch class (torch::optim::Adagrad, RMSprop, SGD: MagSGD is an SGD, and its stateless file is still written so the
reference's Model::Load finds one).  RLGPU_OPTIM.safetensors records each model's type as <NAME>.optim_type (one
int64, RLGPU_OPT_*); a file without the key holds Adam / AdamW state.  A stored type whose state the handle's optimizer
cannot use (anything but Adam <-> AdamW) warns by name and resets that model's state, as the reference resets an
optimizer whose file it cannot use.
"""
import json
import os
import shutil
import warnings

STATS_FILE = "RUNNING_STATS.json"          # Learner.cpp:221
MODEL_NAMES = ("policy", "critic", "shared_head")  # PPOLearner model names (PPOLearner.cpp:42-74)
OPTIM_FILE = "RLGPU_OPTIM.safetensors"
OPTIM_TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rlgpu_optim_lt")
OPTIMIZERS = {"adamw": 0, "adam": 1, "adagrad": 2, "rmsprop": 3, "magsgd": 4}  # RLGPU_OPT_* (rlgpu.ppo.OPTIMIZERS)


def _optimizer_name(name):
    if name not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {sorted(OPTIMIZERS)}, not {name!r}")
    return name


def _model_optimizers(ppo):
    """The optimizer name of each model of a PPO (its optim_options; AdamW where it carries none)."""
    names = (getattr(ppo, "optim_options", None) or {}).get("optimizer", ("adamw",) * 3)
    return {mi: _optimizer_name(names[mi]) for mi in ppo.models}


def _same_state(a, b):
    """Whether optimizer b can use optimizer a's state: the same type, or Adam and AdamW (the same moments)."""
    return a == b or {a, b} == {"adam", "adamw"}


def model_path(folder, name, suffix=""):
    """Model::GetSuffixedSavePath (Models.h:114-128): upper-cased name + suffix + ".lt"."""
    return os.path.join(folder, (name + suffix).upper() + ".lt")


def numbered_dirs(base):
    """Utils::FindNumberedDirs: integer-named subdirectories of base."""
    if not os.path.isdir(base):
        return set()
    return {int(n) for n in os.listdir(base) if n.isdigit() and os.path.isdir(os.path.join(base, n))}


def _shape_args(shapes):
    return ["x".join(str(int(d)) for d in s) for s in shapes]


def _optimizer_args(optimizer):
    # the default stays the command line it always was
    return [] if _optimizer_name(optimizer) == "adamw" else ["--optimizer", optimizer]


def write_optim_archive(path, shapes, step, lr, betas, eps, weight_decay, exp_avg, exp_avg_sq, optimizer="adamw"):
    """<NAME>_OPTIM.lt via libtorch's AdamW::save (Models.cpp:122-125).  shapes: the model's parameter
    shapes in parameters() order; exp_avg / exp_avg_sq: their moments, flat in that order.  optimizer: the libtorch
    class that writes the file -- "adamw" / "adam" (AdamW, as always), "adagrad" (Adagrad: step and sum = exp_avg_sq),
    "rmsprop" (RMSprop: step and square_avg = exp_avg_sq) or "magsgd" (SGD, no state); betas, eps and weight_decay
    matter to AdamW alone."""
    import subprocess
    import tempfile

    import numpy as np
    if not os.path.exists(OPTIM_TOOL):
        raise FileNotFoundError(f"{OPTIM_TOOL} is not built (__graft_entry__.build / make optim)")
    state = np.concatenate([np.asarray(exp_avg, np.float32).ravel(), np.asarray(exp_avg_sq, np.float32).ravel()])
    with tempfile.NamedTemporaryFile(suffix=".f32", delete=False) as f:
        state.tofile(f)
        tmp = f.name
    try:
        r = subprocess.run([OPTIM_TOOL, "save", path, tmp, str(int(step)), repr(float(lr)), repr(float(betas[0])),
                            repr(float(betas[1])), repr(float(eps)), repr(float(weight_decay)), *_shape_args(shapes),
                            *_optimizer_args(optimizer)],
                           capture_output=True, text=True)
    finally:
        os.unlink(tmp)
    if r.returncode != 0:
        raise RuntimeError(f"writing {path} failed: {r.stderr.strip()}")


def read_optim_archive(path, shapes, optimizer="adamw"):
    """(step, exp_avg, exp_avg_sq) of a <NAME>_OPTIM.lt read by libtorch's AdamW::load
    (Models.cpp:177-180) into parameters of `shapes`; parameters without state read as zeros.  optimizer: the
    libtorch class that reads it, as in write_optim_archive; Adagrad's sum / RMSprop's square_avg come back as
    exp_avg_sq with exp_avg zero, an SGD file as step 0 and zeros."""
    import subprocess
    import tempfile

    import numpy as np
    if not os.path.exists(OPTIM_TOOL):
        raise FileNotFoundError(f"{OPTIM_TOOL} is not built (__graft_entry__.build / make optim)")
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        tmp = f.name
    try:
        r = subprocess.run([OPTIM_TOOL, "load", path, tmp, *_shape_args(shapes), *_optimizer_args(optimizer)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reading {path} failed: {r.stderr.strip()}")
        raw = open(tmp, "rb").read()
    finally:
        os.unlink(tmp)
    n = sum(int(np.prod(s)) for s in shapes)
    step = int(np.frombuffer(raw[:8], np.int64)[0])
    v = np.frombuffer(raw[8:], np.float32)
    return step, v[:n].copy(), v[n:2 * n].copy()


def write_model(seq, path):
    """torch::save(seq) equivalent: a scripted nn.Sequential (CPU tensors)."""
    import torch
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)  # TorchScript is the format libtorch reads
        torch.jit.script(seq.cpu()).save(path)


class _ScriptObject:
    """Stand-in for a pickled TorchScript module object: only its attribute dict is kept."""


_STORAGE_DTYPES = {"FloatStorage": "float32", "DoubleStorage": "float64", "HalfStorage": "float16",
                   "BFloat16Storage": "bfloat16", "LongStorage": "int64", "IntStorage": "int32",
                   "ShortStorage": "int16", "CharStorage": "int8", "ByteStorage": "uint8", "BoolStorage": "bool"}


def _rebuild_tensor(storage, offset, size, stride, *_):
    return storage.as_strided(tuple(size), tuple(stride), offset).clone()


def read_model_state(path):
    """Parameters of a <NAME>.lt in torch parameters() order (reference- or rlgpu-written), read
    without executing anything from the archive: the TorchScript zip's data.pkl is unpickled by a
    loader that admits only tensor rebuilds (torch._utils._rebuild_tensor_v2 with typed storages
    from the archive's data/ records), OrderedDict and inert stand-ins for the __torch__ module
    classes -- the archive's code/ is never read.  Tensors are collected depth-first, each object's
    own tensors before its submodules' (Module::parameters() order; Linear / LayerNorm hold only
    weight and bias)."""
    import collections
    import io
    import pickle
    import zipfile

    import torch

    with zipfile.ZipFile(path) as z:
        names = z.namelist()
        pkl = [n for n in names if n.endswith("/data.pkl") and n.count("/") == 1]
        if len(pkl) != 1:
            raise ValueError(f"{path}: not a TorchScript archive (no top-level data.pkl)")
        prefix = pkl[0][:-len("data.pkl")]

        class _Reader(pickle.Unpickler):
            def find_class(self, module, name):
                if module.startswith("__torch__"):
                    return _ScriptObject
                if (module, name) == ("torch._utils", "_rebuild_tensor_v2"):
                    return _rebuild_tensor
                if (module, name) == ("collections", "OrderedDict"):
                    return collections.OrderedDict
                if module == "torch" and name in _STORAGE_DTYPES:
                    return getattr(torch, _STORAGE_DTYPES[name])
                raise pickle.UnpicklingError(f"{path}: refusing to load global {module}.{name}")

            def persistent_load(self, pid):
                if not (isinstance(pid, tuple) and len(pid) == 5 and pid[0] == "storage"):
                    raise pickle.UnpicklingError(f"{path}: unexpected persistent id {pid!r}")
                _, dtype, key, _loc, numel = pid
                raw = bytearray(z.read(prefix + "data/" + str(key)))
                t = torch.frombuffer(raw, dtype=dtype) if raw else torch.empty(0, dtype=dtype)
                if t.numel() < numel:
                    raise pickle.UnpicklingError(f"{path}: storage {key} is truncated")
                return t

        root = _Reader(io.BytesIO(z.read(pkl[0]))).load()

    out = []

    def walk(obj):
        attrs = obj.__dict__ if isinstance(obj, _ScriptObject) else {}
        out.extend(v.detach().float() for v in attrs.values() if isinstance(v, torch.Tensor))
        for v in attrs.values():
            if isinstance(v, _ScriptObject):
                walk(v)

    walk(root)
    return out


def save(learner, folder, keep=8):
    """Learner::Save: <folder>/<total_timesteps>/{RUNNING_STATS.json, POLICY.lt, CRITIC.lt,
    [SHARED_HEAD.lt,] POLICY_OPTIM.lt, CRITIC_OPTIM.lt, [SHARED_HEAD_OPTIM.lt,] RLGPU_OPTIM.safetensors}, then
    prune to `keep` checkpoints (-1 keeps all).
    Returns the path."""
    import torch
    from safetensors.torch import save_file
    path = os.path.join(folder, str(int(learner.total_steps)))
    os.makedirs(path, exist_ok=True)
    stats = {"total_timesteps": int(learner.total_steps), "total_iterations": int(learner.iteration),
             "return_stat": learner.return_stat.to_json()}
    if getattr(learner, "obs_stat", None) is not None:  # Learner.cpp:184-185
        stats["obs_stat"] = learner.obs_stat.to_json()
    skill = getattr(learner, "skill", None)
    if skill is not None:  # PolicyVersionManager::AddRunningStatsToJSON
        stats["skill_ratings"] = skill.cur_ratings.to_json()
    with open(os.path.join(path, STATS_FILE), "w") as f:
        json.dump(stats, f, indent=4)
    ppo = learner.ppo
    shapes = {}
    for mi in ppo.models:
        mod = ppo.torch_module(mi)
        shapes[mi] = [tuple(p.shape) for p in mod.parameters()]
        write_model(mod, model_path(path, MODEL_NAMES[mi]))
    step, m, v = ppo.optimizer_state()
    # one AdamW step count per model: they differ only after transfer learning, whose steps leave the critic's alone;
    # while they are equal the file is what it always was ("step" alone, the policy's)
    steps = {mi: ppo.model_optimizer_step(mi) for mi in ppo.models}
    t = {"step": torch.tensor([step], dtype=torch.int64)}
    kinds = _model_optimizers(ppo)
    for mi in ppo.models:
        name = MODEL_NAMES[mi]
        o, c = ppo.model_range(mi)
        t[name + ".optim_type"] = torch.tensor([OPTIMIZERS[kinds[mi]]], dtype=torch.int64)
        if len(set(steps.values())) > 1:
            t[name + ".step"] = torch.tensor([steps[mi]], dtype=torch.int64)
        t[name + ".exp_avg"] = m[o:o + c].detach().cpu().contiguous()
        t[name + ".exp_avg_sq"] = v[o:o + c].detach().cpu().contiguous()
    save_file(t, os.path.join(path, OPTIM_FILE))
    # the reference's <NAME>_OPTIM.lt (Model::Save with saveOptim)
    opts = getattr(ppo, "optim_options", None)
    if opts is None or not os.path.exists(OPTIM_TOOL):
        warnings.warn("*_OPTIM.lt archives not written (no optimizer options or rlgpu_optim_lt not built)")
    else:
        for mi in ppo.models:
            name = MODEL_NAMES[mi]
            write_optim_archive(model_path(path, name, "_OPTIM"), shapes[mi], steps[mi], opts["lr"][mi], opts["betas"], opts["eps"],
                                opts["weight_decay"], t[name + ".exp_avg"].numpy(), t[name + ".exp_avg_sq"].numpy(),
                                optimizer=kinds[mi])
    if keep != -1:
        dirs = numbered_dirs(folder)
        while len(dirs) > keep:
            low = min(dirs)
            shutil.rmtree(os.path.join(folder, str(low)))
            dirs.discard(low)
    return path


def load(learner, folder, allow_missing_models=True):
    """Learner::Load: the highest numbered checkpoint under `folder` (none: start fresh, returns
    None).  Model sizes must match the current architecture (Models.cpp:147-166)."""
    import torch
    dirs = numbered_dirs(folder)
    if not dirs:
        return None
    path = os.path.join(folder, str(max(dirs)))
    with open(os.path.join(path, STATS_FILE)) as f:
        j = json.load(f)
    learner.total_steps = int(j["total_timesteps"])
    learner.iteration = int(j["total_iterations"])
    if "return_stat" in j:
        learner.return_stat.read_json(j["return_stat"])
    if getattr(learner, "obs_stat", None) is not None and "obs_stat" in j:  # Learner.cpp:214-215
        learner.obs_stat.read_json(j["obs_stat"])
    skill = getattr(learner, "skill", None)
    if skill is not None and "skill_ratings" in j:  # LoadRunningStatsFromJSON
        from .skill import SkillRating
        skill.cur_ratings = SkillRating.from_json(j["skill_ratings"])
    ppo = learner.ppo
    for mi in ppo.models:
        name = MODEL_NAMES[mi]
        p = model_path(path, name)
        if not os.path.exists(p):
            if allow_missing_models:
                warnings.warn(f'model "{name}" does not exist in {path} and will be reset')
                continue
            raise FileNotFoundError(f'model "{name}" does not exist in {path}')
        tensors = read_model_state(p)
        want = ppo.model_sizes(mi)
        got = [t.numel() for t in tensors]
        if got != want:
            raise ValueError(f"Saved model has different size than current model, cannot load model from {p}:\n"
                             f" > Current model: {want},\n > Saved model:   {got}")
        o, c = ppo.model_range(mi)
        ppo.params[o:o + c].copy_(torch.cat([t.reshape(-1) for t in tensors]).to(ppo.params.device))
    ppo.refresh_half()
    op = os.path.join(path, OPTIM_FILE)
    if os.path.exists(op):
        from safetensors.torch import load_file
        t = load_file(op)
        step, m, v = ppo.optimizer_state()
        kinds = _model_optimizers(ppo)
        names = {v_: k for k, v_ in OPTIMIZERS.items()}
        reset = []
        for mi in ppo.models:
            name = MODEL_NAMES[mi]
            o, c = ppo.model_range(mi)
            if name + ".exp_avg" not in t or t[name + ".exp_avg"].numel() != c:
                raise ValueError(f"optimizer state in {op} does not match the model sizes")
            # a file without the key is Adam / AdamW
            stored = names.get(int(t[name + ".optim_type"][0]), "unknown") if name + ".optim_type" in t else "adamw"
            if not _same_state(stored, kinds[mi]):
                warnings.warn(f'the optimizer state of model "{name}" in {op} is {stored}\'s and the model\'s optimizer is '
                              f"{kinds[mi]}, optimizer will be reset")
                m[o:o + c].zero_()
                v[o:o + c].zero_()
                reset.append(mi)
                continue
            m[o:o + c].copy_(t[name + ".exp_avg"].to(m.device))
            v[o:o + c].copy_(t[name + ".exp_avg_sq"].to(v.device))
        ppo.set_optimizer_step(int(t["step"][0]))
        for mi in ppo.models:  # per-model counts, written when they differ
            if MODEL_NAMES[mi] + ".step" in t:
                ppo.set_model_optimizer_step(mi, int(t[MODEL_NAMES[mi] + ".step"][0]))
        for mi in reset:
            ppo.set_model_optimizer_step(mi, 0)
    elif any(os.path.exists(model_path(path, MODEL_NAMES[mi], "_OPTIM")) for mi in ppo.models):
        # a reference checkpoint: its AdamW archives (Model::Load, Models.cpp:168-186); a model
        # without one resets its moments, as the reference resets that model's optimizer
        step, m, v = ppo.optimizer_state()
        steps, own = [], {}
        for mi in ppo.models:
            name = MODEL_NAMES[mi]
            o, c = ppo.model_range(mi)
            p = model_path(path, name, "_OPTIM")
            usable = os.path.exists(p) and os.path.getsize(p) > 0
            if usable and not os.path.exists(OPTIM_TOOL):
                # a readable archive this build cannot parse: resetting would silently drop the saved moments
                raise RuntimeError(f"{p} holds optimizer state but {OPTIM_TOOL} is not built (make -C "
                                   "reinforcement-learning_amd optim)")
            if not usable:
                # the reference resets a model's optimizer whose state it cannot use (Models.cpp:168-186)
                warnings.warn(f"no optimizer found at {p}, optimizer will be reset")
                m[o:o + c].zero_()
                v[o:o + c].zero_()
                continue
            shapes = [tuple(q.shape) for q in ppo.torch_module(mi).parameters()]
            s_, ea, eas = read_optim_archive(p, shapes, optimizer=_model_optimizers(ppo)[mi])
            m[o:o + c].copy_(torch.from_numpy(ea).to(m.device))
            v[o:o + c].copy_(torch.from_numpy(eas).to(v.device))
            steps.append(s_)
            own[mi] = s_
        ppo.set_optimizer_step(max(steps) if steps else 0)
        for mi, s_ in own.items():  # each archive's own count (they differ after transfer learning)
            if s_ != max(steps):
                ppo.set_model_optimizer_step(mi, s_)
    else:
        warnings.warn(f"no optimizer state found in {path}, optimizer will be reset")
        step, m, v = ppo.optimizer_state()
        m.zero_()
        v.zero_()
        ppo.set_optimizer_step(0)
    return path

"""PPO actor/critic over the C ABI of include/rlgpu_ppo.h -- the Python mirror of
GGL::PPOLearner (GigaLearnCPP/src/private/GigaLearnCPP/PPO/PPOLearner.h:41-59) and
GGL::Model (Util/Models.h:21-163).

Method map (reference -> here):
    Model(name, ModelConfig)                         -> part of PPO(...) (policy = 0, critic = 1,
                                                        shared_head = 2 when shared_layers is given)
    PPOLearner::InferActions(obs, masks, ...)        -> infer_actions(obs, masks, step)
    PPOLearner::InferCritic / InferCriticBatched     -> infer_critic(obs)
    PPOLearner::Learn per-minibatch body (:341-475)  -> minibatch(...)
    clip_grad_norm_ + ModelSet::StepOptims (:521-529)-> optimizer_step()
    Model::CopyParams / parameters()                 -> params (flat fp32 device tensor), model_slice()
"""
import ctypes
import math

from . import _lib
from ._lib import alias

MAX_LAYERS = 8
NUM_METRICS = 16
METRICS = ("entropy", "kl", "policy_loss", "critic_loss", "ratio", "clip_fraction", "count",
           "grad_norm_policy", "grad_norm_critic", "grad_norm_shared", "guiding_loss", "tl_loss", "tl_accuracy",
           "tl_old_entropy")
M_GUIDING_LOSS = 10  # RLGPU_M_GUIDING_LOSS
M_TL_LOSS, M_TL_ACCURACY, M_TL_OLD_ENTROPY = 11, 12, 13  # RLGPU_M_TL_*
MODEL_NAMES = ("policy", "critic", "shared_head")  # GGL::Model::modelName (PPOLearner.cpp:66-72)


class _Cfg(ctypes.Structure):
    _fields_ = [("obs_size", ctypes.c_int32), ("num_actions", ctypes.c_int32),
                ("policy_layers", ctypes.c_int32 * MAX_LAYERS), ("n_policy_layers", ctypes.c_int32),
                ("critic_layers", ctypes.c_int32 * MAX_LAYERS), ("n_critic_layers", ctypes.c_int32),
                ("layer_norm", ctypes.c_int32), ("leaky_slope", ctypes.c_float), ("activation", ctypes.c_int32),
                ("policy_lr", ctypes.c_float), ("critic_lr", ctypes.c_float),
                ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("weight_decay", ctypes.c_float), ("clip_range", ctypes.c_float),
                ("entropy_scale", ctypes.c_float), ("max_grad_norm", ctypes.c_float),
                ("max_rows", ctypes.c_int32), ("seed", ctypes.c_uint64), ("train_gemm", ctypes.c_int32),
                ("infer_fp16", ctypes.c_int32), ("shared_layers", ctypes.c_int32 * MAX_LAYERS),
                ("n_shared_layers", ctypes.c_int32), ("sample_row_offset", ctypes.c_int64),
                ("policy_temperature", ctypes.c_float), ("mask_entropy", ctypes.c_int32)]

GEMM_F32X6, GEMM_F32, GEMM_F16X3 = 0, 1, 2  # rlgpu_ppo_config.train_gemm (include/rlgpu_ppo.h)
# rlgpu_ppo_config.activation / rlgpu_learner_config.activation (RLGPU_ACT_*, ModelActivationType)
ACTIVATIONS = {"leaky_relu": 0, "relu": 1, "sigmoid": 2, "tanh": 3}


# rlgpu_ppo_set_optimizer / rlgpu_learner_config.optimizer (RLGPU_OPT_*, ModelOptimType)
OPTIMIZERS = {"adamw": 0, "adam": 1, "adagrad": 2, "rmsprop": 3, "magsgd": 4}
OPTIMIZER_NAMES = {v: k for k, v in OPTIMIZERS.items()}


def optimizer_id(name):
    """RLGPU_OPT_* of an optimizer name."""
    if name not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {sorted(OPTIMIZERS)}, not {name!r}")
    return OPTIMIZERS[name]


def activation_id(name):
    """RLGPU_ACT_* of an activation name."""
    if name not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}, not {name!r}")
    return ACTIVATIONS[name]


_bound = False


def _bind():
    global _bound
    L = _lib.lib()
    if _bound:
        return L
    vp, i32, i64, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float
    L.rlgpu_ppo_create.argtypes = [ctypes.POINTER(_Cfg), ctypes.POINTER(vp)]
    L.rlgpu_ppo_destroy.argtypes = [vp]
    L.rlgpu_ppo_config_size.restype = i32
    L.rlgpu_ppo_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i64)]
    L.rlgpu_ppo_model_range.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.rlgpu_ppo_init_params.argtypes = [vp, u64, vp]
    L.rlgpu_ppo_refresh_half.argtypes = [vp, vp]
    L.rlgpu_ppo_forward.argtypes = [vp, i32, i32, vp, i32, vp, vp]
    L.rlgpu_ppo_infer_actions.argtypes = [vp, vp, vp, i32, i32, u64, vp, vp, vp]
    L.rlgpu_ppo_infer_critic.argtypes = [vp, vp, i64, vp, vp]
    L.rlgpu_mean_std.argtypes = [vp, i64, vp, vp]
    L.rlgpu_ppo_minibatch.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i64, vp, vp, vp]
    L.rlgpu_ppo_minibatch_guided.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i64, vp, vp, f32, vp, vp]
    L.rlgpu_ppo_set_guide.argtypes = [vp, vp, vp]
    L.rlgpu_ppo_infer_guide_logits.argtypes = [vp, vp, i64, vp, vp]
    L.rlgpu_ppo_optimizer_step.argtypes = [vp, vp, vp]
    L.rlgpu_ppo_zero_grad.argtypes = [vp, vp]
    L.rlgpu_ppo_optimizer_state.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.rlgpu_ppo_set_optimizer_step.argtypes = [vp, i64]
    L.rlgpu_ppo_model_optimizer_step.argtypes = [vp, i32, ctypes.POINTER(i64)]
    L.rlgpu_ppo_set_model_optimizer_step.argtypes = [vp, i32, i64]
    L.rlgpu_ppo_set_optimizer.argtypes = [vp, i32, i32]
    L.rlgpu_ppo_get_optimizer.argtypes = [vp, i32, ctypes.POINTER(i32)]
    L.rlgpu_ppo_teacher_probs.argtypes = [vp, vp, vp, i64, vp, i32, vp, vp, vp, vp]
    L.rlgpu_teacher_probs_from_logits.argtypes = [vp, vp, i64, i32, vp, i32, f32, i32, vp, vp, vp, vp]
    L.rlgpu_ppo_transfer_chunk.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i64, i32, f32, f32, vp, vp]
    L.rlgpu_ppo_transfer_step.argtypes = [vp, f32, vp]
    L.rlgpu_diff_norm.argtypes = [vp, vp, i64, vp, vp, vp]
    L.rlgpu_ppo_set_version.argtypes = [vp, vp, vp]
    L.rlgpu_ppo_infer_actions_mixed.argtypes = [vp, vp, vp, i32, i32, u64, vp, vp, vp, vp]
    L.rlgpu_ppo_infer_actions_rows.argtypes = [vp, vp, vp, i32, i64, i32, u64, vp, vp, vp, vp]
    L.rlgpu_ppo_infer_actions_wave.argtypes = [vp, vp, vp, i32, i64, i32, u64, vp, vp, vp, vp]
    L.rlgpu_ppo_infer_values_wave.argtypes = [vp, i32, vp, i32, vp, vp]
    L.rlgpu_ppo_wave_infer.argtypes = [vp, i32]
    L.rlgpu_permutation.argtypes = [i64, u64, u64, vp, vp]
    L.rlgpu_kernel_timing.argtypes = [i32]
    L.rlgpu_kernel_timing_read.argtypes = [vp, vp, vp, i32]
    _bound = True
    return L


def param_count(obs_size, num_actions, layers, out=None, layer_norm=True):
    """Parameter count of a GGL::Model (Linear [+LayerNorm] per hidden layer + output Linear;
    out=0: no output layer, the shared head)."""
    n, prev = 0, obs_size
    for h in layers:
        n += prev * h + h + (2 * h if layer_norm else 0)
        prev = h
    o = num_actions if out is None else out
    return n + prev * o + o


class PPO:
    """Policy + critic (+ an optional shared head in front of both: PPOLearnerConfig::sharedHead),
    AdamW, fp32 training / bf16 inference, all in HBM."""

    def __init__(self, obs_size=167, num_actions=90, policy_layers=(512, 512), critic_layers=(512, 512),
                 layer_norm=True, policy_lr=2.5e-4, critic_lr=2.5e-4, clip_range=0.2, entropy_scale=0.035,
                 max_grad_norm=0.5, max_rows=50_000, seed=42, init=True, device="cuda:0",
                 betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, leaky_slope=0.01, train_gemm=GEMM_F16X3,
                 infer_fp16=False, shared_layers=(), policy_temperature=1.0, mask_entropy=False, activation="leaky_relu",
                 optimizer="adamw"):
        """activation (ModelConfig::activationType of every model): "leaky_relu" (with leaky_slope), "relu", "sigmoid"
        or "tanh".  optimizer (ModelConfig::optimType of every model): "adamw", "adam" (AdamW's arithmetic with
        weight_decay 0), "adagrad", "rmsprop" or "magsgd" (libtorch's defaults, rlgpu_ppo_set_optimizer; set_optimizer
        changes one model's before its first step).  policy_temperature (PPOLearnerConfig::policyTemperature): sampling and the minibatch loss divide the
        logits by it (0 = the C default, 1).  mask_entropy (maskEntropy): each row's entropy over log(its legal
        actions) instead of log(num_actions)."""
        import torch
        opt_type = optimizer_id(optimizer)
        if optimizer == "adam":
            weight_decay = 0.0
        if not torch.cuda.is_available():
            raise _lib.RLGPUError("PPO needs an MI355X: the product path has no CPU fallback")
        L = _bind()
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        c = _Cfg()
        c.obs_size, c.num_actions = obs_size, num_actions
        c.n_policy_layers, c.n_critic_layers = len(policy_layers), len(critic_layers)
        for i, v in enumerate(policy_layers):
            c.policy_layers[i] = v
        for i, v in enumerate(critic_layers):
            c.critic_layers[i] = v
        c.n_shared_layers = len(shared_layers)
        for i, v in enumerate(shared_layers):
            c.shared_layers[i] = v
        c.layer_norm, c.leaky_slope, c.activation = int(layer_norm), leaky_slope, activation_id(activation)
        self.leaky_slope, self.activation = leaky_slope, activation
        c.policy_lr, c.critic_lr = policy_lr, critic_lr
        c.beta1, c.beta2, c.eps, c.weight_decay = betas[0], betas[1], eps, weight_decay
        c.clip_range, c.entropy_scale, c.max_grad_norm = clip_range, entropy_scale, max_grad_norm
        c.max_rows, c.seed = max_rows, seed
        c.train_gemm = train_gemm
        c.infer_fp16 = self.infer_fp16 = int(infer_fp16)
        c.policy_temperature, c.mask_entropy = policy_temperature, int(mask_entropy)
        h = ctypes.c_void_p()
        _lib.check(L.rlgpu_ppo_create(ctypes.byref(c), ctypes.byref(h)), "rlgpu_ppo_create")
        self._h = h
        self.cfg = c
        # optimizer options per model (checkpoint.py's *_OPTIM.lt): the shared head steps at min(LR)
        self.optim_options = {"lr": (policy_lr, critic_lr, min(policy_lr, critic_lr)), "betas": tuple(betas), "eps": eps,
                              "weight_decay": weight_decay, "optimizer": (optimizer,) * 3}
        if opt_type != OPTIMIZERS["adamw"]:
            _lib.check(L.rlgpu_ppo_set_optimizer(h, -1, opt_type), "rlgpu_ppo_set_optimizer")
        self.obs_size, self.num_actions = obs_size, num_actions
        self.policy_layers, self.critic_layers, self.layer_norm = tuple(policy_layers), tuple(critic_layers), layer_norm
        self.shared_layers = tuple(shared_layers)
        self.max_rows = max_rows
        p, g, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(L.rlgpu_ppo_buffers(h, ctypes.byref(p), ctypes.byref(g), ctypes.byref(n)), "rlgpu_ppo_buffers")
        self.num_params = n.value
        self.params = alias(p.value, (n.value,), torch.float32, self.device)
        self.grads = alias(g.value, (n.value,), torch.float32, self.device)
        self.metrics = torch.zeros(NUM_METRICS, device=self.device)
        self.adv_stats = torch.zeros(2, device=self.device)
        if init:
            self.init_params(seed)

    @classmethod
    def wrap(cls, handle, device, policy_layers, critic_layers, max_rows, obs_size=167, num_actions=90,
             layer_norm=True, leaky_slope=0.01, metrics_source=None, owner=None, shared_layers=(), optim_options=None,
             activation="leaky_relu", infer_fp16=False):
        """A PPO view of a handle owned elsewhere (the C++ Learner's PPOLearner): not destroyed
        by this object.  metrics_source(reset) -> (sums, count) replaces the own metric buffer."""
        import torch
        L = _bind()
        self = cls.__new__(cls)
        self._h, self._owned, self._owner = ctypes.c_void_p(handle), False, owner
        self.device = torch.device(device)
        self.obs_size, self.num_actions = obs_size, num_actions
        self.policy_layers, self.critic_layers, self.layer_norm = tuple(policy_layers), tuple(critic_layers), layer_norm
        self.shared_layers = tuple(shared_layers)
        self.leaky_slope, self.max_rows = leaky_slope, max_rows
        self.infer_fp16 = int(infer_fp16)
        activation_id(activation)
        self.activation = activation
        self.optim_options = optim_options
        p, g, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(L.rlgpu_ppo_buffers(self._h, ctypes.byref(p), ctypes.byref(g), ctypes.byref(n)), "rlgpu_ppo_buffers")
        self.num_params = n.value
        self.params = alias(p.value, (n.value,), torch.float32, self.device)
        self.grads = alias(g.value, (n.value,), torch.float32, self.device)
        self.metrics = torch.zeros(NUM_METRICS, device=self.device)
        self.adv_stats = torch.zeros(2, device=self.device)
        self._metrics_source = metrics_source
        return self

    _owned = True
    _metrics_source = None
    _guided = False  # a guide was used since the metrics were last reset: read_metrics reports "Guiding Loss"
    infer_fp16 = 0
    optim_options = None

    def set_optimizer(self, model, optimizer):
        """rlgpu_ppo_set_optimizer: the optimizer (a name of OPTIMIZERS) of one model (0 policy, 1 critic, 2 shared
        head) or of every model (-1), before that model's first step.  "adam" and "adamw" both mean the handle's Adam
        arithmetic with its weight_decay."""
        t = optimizer_id(optimizer)
        _lib.check(_bind().rlgpu_ppo_set_optimizer(self._h, int(model), t), "rlgpu_ppo_set_optimizer")
        if self.optim_options is not None:
            names = list(self.optim_options.get("optimizer", ("adamw",) * 3))
            for mi in range(3):
                if model < 0 or model == mi:
                    names[mi] = optimizer
            self.optim_options["optimizer"] = tuple(names)

    def get_optimizer(self, model):
        """The optimizer name of one model (rlgpu_ppo_get_optimizer)."""
        t = ctypes.c_int32()
        _lib.check(_bind().rlgpu_ppo_get_optimizer(self._h, int(model), ctypes.byref(t)), "rlgpu_ppo_get_optimizer")
        return OPTIMIZER_NAMES[t.value]

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                _lib.check(_lib.lib().rlgpu_ppo_destroy(self._h), "rlgpu_ppo_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- parameters
    def model_range(self, model):
        off, cnt = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.lib().rlgpu_ppo_model_range(self._h, model, ctypes.byref(off), ctypes.byref(cnt)), "model_range")
        return off.value, cnt.value

    def model_slice(self, model, grads=False):
        off, cnt = self.model_range(model)
        return (self.grads if grads else self.params)[off:off + cnt]

    @property
    def models(self):
        """Model indices present: policy, critic (and the shared head)."""
        return (0, 1, 2) if self.shared_layers else (0, 1)

    def flat(self, grads=False):
        """Concatenation of the models' parameters (or gradients) in torch parameters() order,
        without the alignment gap between models (policy, critic, shared head)."""
        import torch
        return torch.cat([self.model_slice(m, grads) for m in self.models])

    def policy_version(self):
        """The flat parameters an old policy version holds: the policy's, then the shared head's
        (PolicyVersionManager versions GetPolicyModels(), PPOLearner.cpp:665-674)."""
        import torch
        return torch.cat([self.model_slice(m) for m in self.models if m != 1])

    def model_in(self, model):
        return self.shared_layers[-1] if (self.shared_layers and model != 2) else self.obs_size

    def model_out(self, model):
        return (self.num_actions, 1, self.shared_layers[-1] if self.shared_layers else 0)[model]

    def init_params(self, seed):
        _lib.check(_lib.lib().rlgpu_ppo_init_params(self._h, seed, _lib.stream_ptr()), "init_params")

    def refresh_half(self):
        _lib.check(_lib.lib().rlgpu_ppo_refresh_half(self._h, _lib.stream_ptr()), "refresh_half")

    def torch_module(self, model):
        """An equivalent torch.nn.Sequential (torch parameters() order = the flat layout), on CPU,
        holding a copy of the current parameters: checkpoint export and test reference."""
        import torch
        layers = (self.policy_layers, self.critic_layers, self.shared_layers)[model]
        out = None if model == 2 else self.model_out(model)
        seq = make_sequential(self.model_in(model), out, layers, self.layer_norm, self.leaky_slope, self.activation)
        flat = self.model_slice(model).detach().cpu()
        o = 0
        with torch.no_grad():
            for prm in seq.parameters():
                prm.copy_(flat[o:o + prm.numel()].view_as(prm))
                o += prm.numel()
        return seq

    def torch_chain(self, model):
        """shared head -> model as one torch.nn.Sequential (the module chain the reference's
        InferPolicyProbsFromModels / InferCritic run, PPOLearner.cpp:90-91,188-191)."""
        import torch
        mods = list(self.torch_module(2)) if (self.shared_layers and model != 2) else []
        return torch.nn.Sequential(*(mods + list(self.torch_module(model))))

    def load_torch_module(self, model, seq):
        import torch
        flat = torch.cat([p.detach().reshape(-1).float() for p in seq.parameters()])
        dst = self.model_slice(model)
        assert flat.numel() == dst.numel(), "architecture mismatch"
        dst.copy_(flat.to(self.device))
        self.refresh_half()

    # ---------------------------------------------------------------- inference
    def forward(self, model, x, half=False, out=None):
        import torch
        n = x.shape[0]
        width = self.model_out(model)
        out = torch.empty((n, width), device=self.device) if out is None else out
        _lib.check(_lib.lib().rlgpu_ppo_forward(self._h, model, int(half), _lib.ptr(x.contiguous()), n, _lib.ptr(out),
                                                _lib.stream_ptr()), "rlgpu_ppo_forward")
        return out

    def infer_actions(self, obs, masks, step=0, deterministic=False, actions=None, logp=None):
        import torch
        n = obs.shape[0]
        actions = torch.empty(n, dtype=torch.int32, device=self.device) if actions is None else actions
        logp = torch.empty(n, device=self.device) if logp is None else logp
        _lib.check(_lib.lib().rlgpu_ppo_infer_actions(self._h, _lib.ptr(obs), _lib.ptr(masks), n, int(deterministic),
                                                      step, _lib.ptr(actions), _lib.ptr(logp), _lib.stream_ptr()),
                   "rlgpu_ppo_infer_actions")
        return actions, logp

    def set_version(self, policy_params):
        """bf16 inference copy of an old policy version (flat fp32 parameters on the device: the
        policy's, then the shared head's -- policy_version())."""
        cnt = sum(self.model_range(m)[1] for m in self.models if m != 1)
        if policy_params.numel() != cnt:
            raise _lib.RLGPUError("policy version has the wrong parameter count")
        _lib.check(_lib.lib().rlgpu_ppo_set_version(self._h, _lib.ptr(policy_params.contiguous()), _lib.stream_ptr()),
                   "rlgpu_ppo_set_version")

    def set_guide(self, policy_params):
        """The guiding policy (PPOLearnerConfig::useGuidingPolicy): a frozen 16-bit copy of a policy given as
        set_version takes one (flat fp32 parameters on the device: the policy's, then the shared head's)."""
        cnt = sum(self.model_range(m)[1] for m in self.models if m != 1)
        if policy_params.numel() != cnt:
            raise _lib.RLGPUError("guiding policy has the wrong parameter count")
        _lib.check(_lib.lib().rlgpu_ppo_set_guide(self._h, _lib.ptr(policy_params.contiguous()), _lib.stream_ptr()),
                   "rlgpu_ppo_set_guide")

    @property
    def logit_dtype(self):
        """torch dtype of the 16-bit inference format (guide logits)."""
        import torch
        return torch.float16 if self.infer_fp16 == 1 else torch.bfloat16

    def guide_logits(self, obs, out=None):
        """The guide's 16-bit inference forward over any number of rows: [n, num_actions] in the handle's 16-bit
        format (the guide_logits of minibatch)."""
        import torch
        n = obs.shape[0]
        out = torch.empty((n, self.num_actions), dtype=self.logit_dtype, device=self.device) if out is None else out
        _lib.check(_lib.lib().rlgpu_ppo_infer_guide_logits(self._h, _lib.ptr(obs.contiguous()), n, _lib.ptr(out),
                                                           _lib.stream_ptr()), "rlgpu_ppo_infer_guide_logits")
        return out

    def infer_actions_mixed(self, obs, masks, old_rows, step=0, deterministic=False, actions=None, logp=None):
        """Rows with old_rows != 0 act with the version of set_version (their logp is not written)."""
        import torch
        n = obs.shape[0]
        actions = torch.empty(n, dtype=torch.int32, device=self.device) if actions is None else actions
        logp = torch.empty(n, device=self.device) if logp is None else logp
        _lib.check(_lib.lib().rlgpu_ppo_infer_actions_mixed(self._h, _lib.ptr(obs), _lib.ptr(masks), n, int(deterministic),
                                                            step, _lib.ptr(old_rows), _lib.ptr(actions), _lib.ptr(logp),
                                                            _lib.stream_ptr()), "rlgpu_ppo_infer_actions_mixed")
        return actions, logp

    def _actions_rows(self, entry, obs, masks, row0, step, deterministic, old_rows, actions, logp):
        import torch
        n = obs.shape[0]
        actions = torch.empty(n, dtype=torch.int32, device=self.device) if actions is None else actions
        logp = torch.empty(n, device=self.device) if logp is None else logp
        _lib.check(getattr(_lib.lib(), entry)(self._h, _lib.ptr(obs), _lib.ptr(masks), n, row0, int(deterministic), step,
                                              _lib.ptr(old_rows) if old_rows is not None else None, _lib.ptr(actions),
                                              _lib.ptr(logp), _lib.stream_ptr()), entry)
        return actions, logp

    def infer_actions_rows(self, obs, masks, row0=0, step=0, deterministic=False, old_rows=None, actions=None, logp=None):
        """rlgpu_ppo_infer_actions_rows: the rows are rows [row0, row0 + n) of the sampler's numbering (fused kernel only)."""
        return self._actions_rows("rlgpu_ppo_infer_actions_rows", obs, masks, row0, step, deterministic, old_rows, actions, logp)

    def infer_actions_wave(self, obs, masks, row0=0, step=0, deterministic=False, old_rows=None, actions=None, logp=None):
        """The same call on the one-wave form of the fused kernel (16 rows per 64-thread workgroup, the collection
        loop's inference): the same actions and log probs, bit for bit.  RLGPUError when the policy is not eligible
        (wave_infer_ok)."""
        return self._actions_rows("rlgpu_ppo_infer_actions_wave", obs, masks, row0, step, deterministic, old_rows, actions, logp)

    def infer_values_wave(self, model, obs, out=None):
        """The 16-bit forward of model 0 / 1 on the one-wave kernel: f32 outputs [n, outputs] (= forward(model, x, half=True))."""
        import torch
        n = obs.shape[0]
        out = torch.empty((n, self.model_out(model)), device=self.device) if out is None else out
        _lib.check(_lib.lib().rlgpu_ppo_infer_values_wave(self._h, model, _lib.ptr(obs), n, _lib.ptr(out), _lib.stream_ptr()),
                   "rlgpu_ppo_infer_values_wave")
        return out

    def wave_infer_ok(self, model=0):
        return bool(_lib.lib().rlgpu_ppo_wave_infer(self._h, model))

    def infer_critic(self, obs, out=None):
        import torch
        n = obs.shape[0]
        out = torch.empty(n, device=self.device) if out is None else out
        _lib.check(_lib.lib().rlgpu_ppo_infer_critic(self._h, _lib.ptr(obs), n, _lib.ptr(out), _lib.stream_ptr()),
                   "rlgpu_ppo_infer_critic")
        return out

    # ---------------------------------------------------------------- learning
    def adv_normalizer(self, adv):
        _lib.check(_lib.lib().rlgpu_mean_std(_lib.ptr(adv), adv.numel(), _lib.ptr(self.adv_stats), _lib.stream_ptr()),
                   "rlgpu_mean_std")
        return self.adv_stats

    def minibatch(self, obs, masks, actions, old_logp, adv, target, index, start, n, batch_size, guide_logits=None,
                  guiding_strength=0.0):
        """guide_logits (16-bit, the handle's inference format, one row of num_actions per row of the batch, addressed
        like masks): adds guiding_strength * mean |guide probs - probs| to the loss (rlgpu_ppo_minibatch_guided)."""
        if guide_logits is None:
            _lib.check(_lib.lib().rlgpu_ppo_minibatch(
                self._h, _lib.ptr(obs), _lib.ptr(masks), _lib.ptr(actions), _lib.ptr(old_logp), _lib.ptr(adv),
                _lib.ptr(target), _lib.ptr(index), start, n, batch_size, _lib.ptr(self.adv_stats), _lib.ptr(self.metrics),
                _lib.stream_ptr()), "rlgpu_ppo_minibatch")
        else:
            self.minibatch_guided(obs, masks, actions, old_logp, adv, target, index, start, n, batch_size, guide_logits,
                                  guiding_strength)
            return
        self._count += 1

    def minibatch_guided(self, obs, masks, actions, old_logp, adv, target, index, start, n, batch_size, guide_logits,
                         guiding_strength):
        """rlgpu_ppo_minibatch_guided; guide_logits None is the unguided minibatch through the same entry point."""
        if guide_logits is not None:
            if guide_logits.element_size() != 2 or guide_logits.shape[-1] != self.num_actions or \
                    guide_logits.shape[0] != masks.shape[0] or not guide_logits.is_contiguous():
                raise _lib.RLGPUError("guide_logits must be contiguous 16-bit [rows of masks, num_actions]")
            self._guided = True
        _lib.check(_lib.lib().rlgpu_ppo_minibatch_guided(
            self._h, _lib.ptr(obs), _lib.ptr(masks), _lib.ptr(actions), _lib.ptr(old_logp), _lib.ptr(adv),
            _lib.ptr(target), _lib.ptr(index), start, n, batch_size, _lib.ptr(self.adv_stats),
            _lib.ptr(guide_logits) if guide_logits is not None else None, guiding_strength, _lib.ptr(self.metrics),
            _lib.stream_ptr()), "rlgpu_ppo_minibatch_guided")
        self._count += 1

    _count = 0

    def optimizer_step(self):
        _lib.check(_lib.lib().rlgpu_ppo_optimizer_step(self._h, _lib.ptr(self.metrics), _lib.stream_ptr()),
                   "rlgpu_ppo_optimizer_step")

    def zero_grad(self):
        _lib.check(_lib.lib().rlgpu_ppo_zero_grad(self._h, _lib.stream_ptr()), "zero_grad")

    def read_metrics(self, reset=True):
        """Report entries of PPOLearner::Learn (:537-566): means over the accumulated minibatches."""
        if self._metrics_source is not None:
            m, cnt = self._metrics_source(reset)
            cnt = max(cnt, 1)
            rep = {"Policy Entropy": m[0] / cnt, "Mean KL Divergence": m[1] / cnt, "Policy Loss": m[2] / cnt,
                   "Critic Loss": m[3] / cnt, "Ratio": m[4] / cnt, "SB3 Clip Fraction": m[5] / cnt,
                   "Policy Grad Norm": m[7], "Critic Grad Norm": m[8], "Shared Head Grad Norm": m[9]}
            if self._guided:
                rep["Guiding Loss"] = m[M_GUIDING_LOSS] / cnt
            return rep
        m = self.metrics.cpu().tolist()
        cnt = max(self._count, 1)
        rep = {"Policy Entropy": m[0] / cnt, "Mean KL Divergence": m[1] / cnt, "Policy Loss": m[2] / cnt,
               "Critic Loss": m[3] / cnt, "Ratio": m[4] / cnt, "SB3 Clip Fraction": m[5] / cnt,
               "Policy Grad Norm": m[7], "Critic Grad Norm": m[8], "Shared Head Grad Norm": m[9]}
        if self._guided:
            rep["Guiding Loss"] = m[M_GUIDING_LOSS] / cnt
        if reset:
            self.metrics.zero_()
            self._count = 0
            self._guided = False
        return rep

    def optimizer_state(self):
        import torch
        step, m, v = ctypes.c_int64(), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(_lib.lib().rlgpu_ppo_optimizer_state(self._h, ctypes.byref(step), ctypes.byref(m), ctypes.byref(v)),
                   "optimizer_state")
        return (step.value, alias(m.value, (self.num_params,), torch.float32, self.device),
                alias(v.value, (self.num_params,), torch.float32, self.device))

    def set_optimizer_step(self, step):
        _lib.check(_lib.lib().rlgpu_ppo_set_optimizer_step(self._h, int(step)), "set_optimizer_step")

    def model_optimizer_step(self, model):
        """The AdamW step count of one model (0 policy, 1 critic, 2 shared head): equal for all models unless
        transfer_step ran, which leaves the critic's alone."""
        step = ctypes.c_int64()
        _lib.check(_lib.lib().rlgpu_ppo_model_optimizer_step(self._h, model, ctypes.byref(step)), "model_optimizer_step")
        return step.value

    def set_model_optimizer_step(self, model, step):
        _lib.check(_lib.lib().rlgpu_ppo_set_model_optimizer_step(self._h, model, int(step)), "set_model_optimizer_step")

    # ---------------------------------------------------------------- transfer learning
    def teacher_probs(self, obs, masks, action_map=None, num_actions_out=None, metrics=None):
        """This handle as the teacher of PPOLearner::TransferLearn: its inference forward over obs [n, obs_size], the
        clamped masked softmax at its policy_temperature over masks [n, num_actions], and -- action_map int32
        [n, num_actions_out] given -- the gather out[i][k] = old[i][map[i][k]].  Returns (probs f32 [n, A_out], argmax
        int32 [n]); the teacher's mean entropy is added to metrics[M_TL_OLD_ENTROPY] (metrics: a NUM_METRICS device
        tensor, usually the student's; default this handle's own).  Map entries must lie in [0, num_actions): they are
        not checked on the device."""
        import torch
        n = obs.shape[0]
        A = self.num_actions if action_map is None else (num_actions_out or action_map.shape[-1])
        if action_map is not None and (action_map.dtype != torch.int32 or tuple(action_map.shape) != (n, A)
                                       or not action_map.is_contiguous()):
            raise _lib.RLGPUError("action_map must be contiguous int32 [rows, num_actions_out]")
        probs = torch.empty((n, A), device=self.device)
        arg = torch.empty(n, dtype=torch.int32, device=self.device)
        metrics = self.metrics if metrics is None else metrics
        _lib.check(_lib.lib().rlgpu_ppo_teacher_probs(
            self._h, _lib.ptr(obs.contiguous()), _lib.ptr(masks.contiguous()), n,
            _lib.ptr(action_map) if action_map is not None else None, A, _lib.ptr(probs), _lib.ptr(arg), _lib.ptr(metrics),
            _lib.stream_ptr()), "rlgpu_ppo_teacher_probs")
        return probs, arg

    def transfer_chunk(self, obs, masks, target_probs, target_argmax, index, start, n, total_rows, use_kl=False,
                       loss_scale=1.0, loss_exponent=1.0):
        """rlgpu_ppo_transfer_chunk: rows index[start : start + n] (index None: identity) of a batch of total_rows rows;
        the distillation loss toward target_probs and its backward through the policy and the shared head, accumulating
        gradients; this chunk's share of the whole-batch metrics into self.metrics."""
        for t in (obs, masks, target_probs, target_argmax):
            if not t.is_contiguous():
                raise _lib.RLGPUError("transfer_chunk takes contiguous tensors")
        if target_probs.shape[-1] != self.num_actions or target_probs.shape[0] != masks.shape[0]:
            raise _lib.RLGPUError("target_probs must be [rows of masks, num_actions]")
        _lib.check(_lib.lib().rlgpu_ppo_transfer_chunk(
            self._h, _lib.ptr(obs), _lib.ptr(masks), _lib.ptr(target_probs), _lib.ptr(target_argmax),
            _lib.ptr(index) if index is not None else None, start, n, total_rows, int(use_kl), loss_scale, loss_exponent,
            _lib.ptr(self.metrics), _lib.stream_ptr()), "rlgpu_ppo_transfer_chunk")

    def transfer_step(self, lr):
        """rlgpu_ppo_transfer_step: AdamW (or the models' optimizer) at learning rate lr on the policy and the shared head, no gradient clipping; the
        critic, its moments and its step count stay."""
        _lib.check(_lib.lib().rlgpu_ppo_transfer_step(self._h, lr, _lib.stream_ptr()), "rlgpu_ppo_transfer_step")

    def transfer_learn(self, teacher, obs, masks, cfg, old_obs=None, old_masks=None, action_map=None):
        """PPOLearner::TransferLearn (PPOLearner.cpp:583-637) on one batch held on the device: the teacher pass, cfg.epochs
        times the whole batch in chunks of max_rows followed by transfer_step(cfg.lr).  cfg: a TransferLearnConfig
        (rlgpu.learner) or anything with its lr / epochs / use_kl_div / loss_scale / loss_exponent.  Returns the report
        entries of the reference."""
        import torch
        N = obs.shape[0]
        tm = torch.zeros(NUM_METRICS, device=self.device)
        probs, arg = teacher.teacher_probs(obs if old_obs is None else old_obs, masks if old_masks is None else old_masks,
                                           action_map, self.num_actions, metrics=tm)
        before = self.model_slice(0).clone()
        first = None
        for _ in range(cfg.epochs):
            self.metrics.zero_()
            for b in range(0, N, self.max_rows):
                self.transfer_chunk(obs, masks, probs, arg, None, b, min(self.max_rows, N - b), N, cfg.use_kl_div,
                                    cfg.loss_scale, cfg.loss_exponent)
            if first is None:
                first = self.metrics.clone()
            self.transfer_step(cfg.lr)
        self.metrics.zero_()
        rep = {"Old Policy Entropy": float(tm[M_TL_OLD_ENTROPY])}
        if first is not None:
            rep.update({"Transfer Learn Accuracy": float(first[M_TL_ACCURACY]), "Transfer Learn Loss": float(first[M_TL_LOSS]),
                        "Policy Entropy": float(first[0])})
        rep["Policy Update Magnitude"] = diff_norm(before, self.model_slice(0))
        return rep

    def model_sizes(self, model):
        """Per-parameter element counts in torch order (GetSeqSizes, Models.cpp:79-87)."""
        return [p.numel() for p in self.torch_module(model).parameters()]


def make_sequential(obs_size, out, layers, layer_norm=True, leaky_slope=0.01, activation="leaky_relu"):
    """GGL::Model's module list (Models.cpp:7-33): per hidden layer Linear [, LayerNorm], the
    activation (AddActivationFunc: ReLU, LeakyReLU(leaky_slope), Sigmoid or Tanh); then the output
    Linear (none when out is None: the shared head, addOutputLayer false).  CPU, torch default init."""
    import torch
    act = (lambda: torch.nn.LeakyReLU(leaky_slope), torch.nn.ReLU, torch.nn.Sigmoid, torch.nn.Tanh)[activation_id(activation)]
    mods, prev = [], obs_size
    for hdim in layers:
        mods.append(torch.nn.Linear(prev, hdim))
        if layer_norm:
            mods.append(torch.nn.LayerNorm(hdim))
        mods.append(act())
        prev = hdim
    if out is not None:
        mods.append(torch.nn.Linear(prev, out))
    return torch.nn.Sequential(*mods)


KERNEL_TIMING_SLOTS = ("forward / input-gradient GEMMs", "weight-gradient GEMMs", "LayerNorm forward",
                       "LayerNorm backward")


def kernel_timing(enable):
    """Start (clearing earlier records) or stop the learn-phase kernel timing (rlgpu_kernel_timing)."""
    _bind()
    _lib.check(_lib.lib().rlgpu_kernel_timing(1 if enable else 0), "rlgpu_kernel_timing")


def kernel_timing_read():
    """{slot name: (ms summed, work summed -- flops or bytes --, launches)} since kernel_timing(True)."""
    import numpy as np
    _bind()
    n = len(KERNEL_TIMING_SLOTS)
    ms, work, cnt = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    _lib.check(_lib.lib().rlgpu_kernel_timing_read(ms.ctypes.data, work.ctypes.data, cnt.ctypes.data, n),
               "rlgpu_kernel_timing_read")
    return {k: (float(ms[i]), float(work[i]), int(cnt[i])) for i, k in enumerate(KERNEL_TIMING_SLOTS)}


def teacher_probs_from_logits(logits, masks, temperature=1.0, mask_entropy=False, action_map=None, metrics=None):
    """rlgpu_teacher_probs_from_logits: PPO.teacher_probs after the forward, from f32 logits [n, A_old] on the device.
    Returns (probs [n, A_out], argmax int32 [n]); metrics as in PPO.teacher_probs (None: not written)."""
    import torch
    _bind()
    n, a_old = logits.shape
    A = a_old if action_map is None else action_map.shape[-1]
    probs = torch.empty((n, A), device=logits.device)
    arg = torch.empty(n, dtype=torch.int32, device=logits.device)
    _lib.check(_lib.lib().rlgpu_teacher_probs_from_logits(
        _lib.ptr(logits.contiguous()), _lib.ptr(masks.contiguous()), n, a_old,
        _lib.ptr(action_map.contiguous()) if action_map is not None else None, A, temperature, int(mask_entropy),
        _lib.ptr(probs), _lib.ptr(arg), _lib.ptr(metrics) if metrics is not None else None, _lib.stream_ptr()),
        "rlgpu_teacher_probs_from_logits")
    return probs, arg


def diff_norm(a, b):
    """||a - b|| of two device tensors of equal size (rlgpu_diff_norm), as a float."""
    import torch
    _bind()
    out = torch.empty(1, device=a.device)
    _lib.check(_lib.lib().rlgpu_diff_norm(_lib.ptr(a.contiguous()), _lib.ptr(b.contiguous()), a.numel(), _lib.ptr(out),
                                          None, _lib.stream_ptr()), "rlgpu_diff_norm")
    return float(out)


def permutation(n, seed, counter, out=None, device="cuda:0"):
    """ExperienceBuffer shuffle (ExperienceBuffer.cpp:130): random permutation of [0, n) on device."""
    import torch
    out = torch.empty(n, dtype=torch.int32, device=device) if out is None else out
    _bind()
    _lib.check(_lib.lib().rlgpu_permutation(n, seed, counter, _lib.ptr(out), _lib.stream_ptr()), "rlgpu_permutation")
    return out


def log_num_actions(a):
    return math.log(a)

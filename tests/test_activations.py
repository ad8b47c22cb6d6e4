"""SIGMOID / TANH activations and addLayerNorm = false: the Python surface, the C config checks, the checkpoint tools
and the training kernels against float64.

The training cases are tests/test_ppo_variants.py's (same numpy parameter streams, same seeds, same batches) with
every LeakyReLU module swapped for Sigmoid / Tanh and the cases' slope set to 1.0, which makes side_conditions skip
its kink check (it reads LeakyReLU inputs; these activations have no kink).  The rules are tests/ppo_reference.py's
check_grads / check_metrics / check_forward, unchanged: error at most factor(mode, n) x torch fp32's own error against
float64 plus the floor, the 1e-4 normwise ceiling, the elementwise band.

Largest (err - floor) / (torch fp32 err) measured on an MI355X over test_training_kernels_against_float64 and
test_fallback_from_full_row_kernels, gradients / forward outputs (metrics: largest err / allowed error):
    x6   6.18 / 0.88 (0.27)      f32   2.43 / 2.78 (0.17)      h3   2.83 / 1.59 (0.14)
The largest gradient error is 2.9e-6 of its tensor's norm, against the 1e-4 ceiling.  x6's 6.18 is one case, the
one-row minibatch with sigmoid (rows1 / sigmoid / x6: every critic tensor, 4.2 .. 6.2; 1.78 on every other case of
that mode), see CASE_FACTOR.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ppo_reference import MODE_IDS, MODES, Case, build_case, check_golden, run_engine_case, side_conditions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "reinforcement-learning_amd", "rlgpu", "rlgpu_optim_lt")
ACTS = ("sigmoid", "tanh")
# the GPU sweep: LayerNorm on / off, M = 1 .. 32 scalar and float4, with and without the rank-1 head, both wide
# kernels, one row and a ragged second block
GPU_CASES = ("a2", "d64", "e100", "h90", "i16", "noln", "noln_wide", "rows1", "rows33")
CPU_CASES = ("a2", "b17", "c16", "d64", "e100", "g128", "h90", "i16", "noln", "noln_wide", "rows1", "rows33")
GOLDEN_CASES = ("a2", "h90", "noln")  # pinned in tests/golden/ppo_reference.npz for both activations
# The entries of test_ppo_variants' SWEEP that the lists above name, restated (that table's comments name the kernels)
CASES = {c.name: c for c in [
    Case("a2", 167, 2, (33, 65), (130, 64), seed=0),
    Case("b17", 168, 17, (64, 128), (65, 33), seed=1),
    Case("c16", 167, 16, (130, 255), (33, 128), seed=1),
    Case("d64", 168, 64, (256, 257), (128, 65), seed=0),
    Case("e100", 167, 100, (510, 512), (257, 256), seed=8),
    Case("g128", 168, 128, (516, 1024), (256, 512), seed=75),
    Case("h90", 167, 90, (1028, 2048), (510, 257), seed=254),
    Case("i16", 167, 16, (1023,), (2047, 1024), seed=350),
    Case("noln", 167, 90, (65, 256), (130, 33), seed=7, ln=False),
    Case("noln_wide", 167, 90, (516, 33), (1023,), seed=2, ln=False),
    Case("rows1", 167, 90, (96, 33), (40, 64), seed=0, n=1),
    Case("rows33", 167, 90, (96, 33), (40, 64), seed=0, n=33),
]}
# The fallback from the full-row H3 kernels: both models (512, 512), 65 rows (one row past the 64-row tile), obs 167
FALLBACK = Case("fallback", 167, 90, (512, 512), (512, 512), seed=0, slope=1.0, n=65)


# The one case with a factor of its own, twice the measured ratio (the float64 yardstick and the 1e-4 ceiling stay).
# rows1 / sigmoid / x6: with one row nothing averages, every element of the critic's gradient is a per-row factor
# times the one dv = 2 (v - t) bsr, so each tensor's error is v's error amplified by |v| / |v - t| = 6.5 here
# (v = 0.213, t = 0.246).  v's error is 3.6 ulp of v and comes from the accuracy of 1 / (1 + expf(-h)) (expf's
# error, then two more roundings; the 64 activations under the rank-1 head are all near 0.5, an ulp of 6e-8 each)
# against torch's CPU sigmoid, which lands 1.7 ulp of v from float64: with the sigmoid computed in double and rounded
# once, everything else unchanged, the same case measured 0.56 on an MI355X.
CASE_FACTOR = {("rows1", "sigmoid", 0): 12.4}


def case_of(name):
    return FALLBACK if name == "fallback" else CASES[name]._replace(slope=1.0)


def act_case(name, act, ln=None):
    """Case `name` with the activation swapped (ln: override the case's LayerNorm setting): modules, batch, the
    float64 reference and the torch fp32 yardstick, computed once."""
    c = case_of(name)
    return build_case(c if ln is None else c._replace(ln=ln), act=act)


def assert_inputs_hold(d, tag):
    """side_conditions by the float64 reference alone, finite gradients, and torch fp32's own error against float64
    in the fp32 class per parameter tensor (a yardstick of 0 or of 1e-3 would make the factor rule vacuous)."""
    import torch
    c = d["case"]
    why = side_conditions(c, d["r64"], torch.from_numpy(d["batch"]["masks"][d["rows"]]))
    assert why is None, f"{tag}: {why}"
    g64, g32 = d["r64"]["grads"], d["r32"]["grads"].double()
    assert bool(g64.isfinite().all()) and bool(g32.isfinite().all()), tag
    assert np.isfinite(d["r64"]["metrics"]).all(), tag
    o = 0
    for m in d["mods"]:
        for name, prm in m.named_parameters():
            k = prm.numel()
            w, t = g64[o:o + k], g32[o:o + k]
            o += k
            rel = float((t - w).norm()) / float(w.norm())
            assert 0 < rel < 1e-5, (tag, name, rel)
    assert o == g64.numel()


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("act,cls", [("leaky_relu", "LeakyReLU"), ("relu", "ReLU"), ("sigmoid", "Sigmoid"),
                                     ("tanh", "Tanh")])
def test_make_sequential_modules(act, cls, ln):
    """Module types and order of GGL::Model's list for the four activation types with and without LayerNorm, with
    and without the output Linear."""
    from rlgpu.ppo import make_sequential
    seq = make_sequential(167, 90, (64, 48), ln, 0.01, act)
    per = ["Linear"] + (["LayerNorm"] if ln else []) + [cls]
    assert [type(m).__name__ for m in seq] == per * 2 + ["Linear"]
    assert [(m.in_features, m.out_features) for m in seq if type(m).__name__ == "Linear"] == [(167, 64), (64, 48), (48, 90)]
    if act == "leaky_relu":
        assert all(m.negative_slope == 0.01 for m in seq if type(m).__name__ == cls)
    head = make_sequential(167, None, (64,), ln, activation=act)
    assert [type(m).__name__ for m in head] == per


def test_make_sequential_positional_call():
    """The five-argument positional call keeps its meaning: LeakyReLU with the given slope."""
    from rlgpu.ppo import make_sequential
    seq = make_sequential(167, 1, (33,), False, 0.2)
    assert [type(m).__name__ for m in seq] == ["Linear", "LeakyReLU", "Linear"] and seq[1].negative_slope == 0.2
    with pytest.raises(ValueError, match="activation"):
        make_sequential(167, 1, (33,), True, 0.01, "swish")


def _small_cfg():
    from rlgpu.ppo import _Cfg
    cfg = _Cfg()
    cfg.obs_size, cfg.num_actions, cfg.max_rows = 167, 90, 64
    cfg.n_policy_layers = cfg.n_critic_layers = 1
    cfg.policy_layers[0] = cfg.critic_layers[0] = 64
    return cfg


@pytest.mark.parametrize("value", [-1, 4])
def test_create_rejects_unknown_activation(value):
    """rlgpu_ppo_create names an activation outside 0..3 with RLGPU_ERR_INVALID_ARG, before any allocation."""
    from rlgpu.ppo import _bind
    L = _bind()
    L.rlgpu_last_error.restype = ctypes.c_char_p
    cfg = _small_cfg()
    cfg.activation = value
    h = ctypes.c_void_p()
    assert L.rlgpu_ppo_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and not h.value
    assert b"activation" in L.rlgpu_last_error()


@pytest.mark.parametrize("value", [0, 1, 2, 3])
def test_create_accepts_every_activation(value):
    """0..3 pass the field (without a GPU create fails later, on its first allocation, not on the field)."""
    from rlgpu.ppo import ACTIVATIONS, _bind
    assert sorted(ACTIVATIONS.values()) == [0, 1, 2, 3]
    L = _bind()
    L.rlgpu_last_error.restype = ctypes.c_char_p
    cfg = _small_cfg()
    cfg.activation = value
    h = ctypes.c_void_p()
    if L.rlgpu_ppo_create(ctypes.byref(cfg), ctypes.byref(h)) == 0:
        assert L.rlgpu_ppo_destroy(h) == 0
    else:
        assert b"activation" not in L.rlgpu_last_error()


def test_learner_default_config_activation():
    """rlgpu_learner_default_config writes LeakyReLU and LayerNorm on; LearnerConfig's defaults say the same; the ABI
    version says the config structs grew."""
    from rlgpu import learner
    L = learner._bind()
    c = learner._CConfig()
    c.activation, c.no_layer_norm = 7, 7
    L.rlgpu_learner_default_config.argtypes = [ctypes.POINTER(learner._CConfig)]
    assert L.rlgpu_learner_default_config(ctypes.byref(c)) == 0
    assert c.activation == 0 and c.no_layer_norm == 0
    d = learner.LearnerConfig()
    assert d.activation == "leaky_relu" and d.layer_norm is True
    assert L.rlgpu_abi_version() >= 101


@pytest.mark.parametrize("ln", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("name", CPU_CASES + ("fallback",))
def test_side_conditions_hold(name, act, ln):
    """The inputs of the GPU tests vouched for on the CPU: the case table's seeds with both activations, LayerNorm on
    and off (the GPU tests run each case at its own setting)."""
    assert_inputs_hold(act_case(name, act, ln), f"{name}/{act}/{'ln' if ln else 'noln'}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_reference_matches_golden(name, act):
    """The float64 reference of three cases with both activations against tests/golden/ppo_reference.npz
    (ppo_reference.check_golden)."""
    check_golden(f"act/{name}/{act}", act_case(name, act))


def _tool(*args):
    return subprocess.run([TOOL, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)


def test_checkpoint_tools_without_layer_norm(tmp_path):
    """A (tanh, no-LayerNorm) policy: checkpoint.write_model's archive read by rlgpu_optim_lt model-load in its
    no-LayerNorm form gives the flat parameters; model-save's archive read by checkpoint.read_model_state gives them
    back; the LayerNorm layout refuses the archive (its module indices do not match)."""
    import torch
    from rlgpu import checkpoint as ckpt
    from rlgpu.ppo import make_sequential
    assert os.path.exists(TOOL), "rlgpu_optim_lt is not built"
    torch.manual_seed(5)
    seq = make_sequential(167, 90, (64, 48), False, activation="tanh")
    flat = torch.cat([p.detach().reshape(-1) for p in seq.parameters()]).numpy()
    assert len(list(seq.parameters())) == 6
    p = tmp_path / "POLICY.lt"
    ckpt.write_model(seq, str(p))
    shape, opt = ["167", "90", "64", "48"], ["--no-layer-norm", "--activation", "tanh"]
    r = _tool("model-load", p, tmp_path / "got.f32", *shape, *opt)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(np.fromfile(tmp_path / "got.f32", np.float32), flat)
    flat.tofile(tmp_path / "p.f32")
    q = tmp_path / "SAVED.lt"
    r = _tool("model-save", q, tmp_path / "p.f32", *shape, *opt)
    assert r.returncode == 0, r.stderr
    state = ckpt.read_model_state(str(q))
    assert [tuple(t.shape) for t in state] == [(64, 167), (64,), (48, 64), (48,), (90, 48), (90,)]
    np.testing.assert_array_equal(torch.cat([t.reshape(-1) for t in state]).numpy(), flat)
    for archive in (p, q):  # the old argument form is the LayerNorm layout
        r = _tool("model-load", archive, tmp_path / "bad.f32", *shape)
        assert r.returncode != 0, "a no-LayerNorm archive loaded into the LayerNorm layout"
    r = _tool("model-load", p, tmp_path / "bad.f32", *shape, "--no-layer-norm", "--activation", "swish")
    assert r.returncode == 2


# ------------------------------------------------------------------ GPU
def run_act_case(gpu, d, act, mode, tag, after_minibatch=None, grad_factor=None):
    """grad_factor: the gradient rule's factor for this case instead of ppo_reference.factor's (CASE_FACTOR)."""
    c = d["case"]
    assert_inputs_hold(d, tag)

    def around(p, when):
        if when == "before":  # the engine's own restatement holds the swapped modules
            for m in (0, 1):
                kinds = {type(x).__name__ for x in p.torch_module(m)}
                assert {"sigmoid": "Sigmoid", "tanh": "Tanh"}[act] in kinds and "LeakyReLU" not in kinds
                assert ("LayerNorm" in kinds) == c.ln
        if after_minibatch:
            after_minibatch(p, when)

    run_engine_case(gpu, d, mode, tag, engine_kw=dict(activation=act), grad_factor=grad_factor,
                    around_minibatch=around)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("name", GPU_CASES)
def test_training_kernels_against_float64(gpu, name, act, mode):
    """One minibatch from zero_grad per case, activation and GEMM mode: gradients, the six metrics and the fp32
    forward of both models against float64, by ppo_reference's rules."""
    run_act_case(gpu, act_case(name, act), act, mode, f"{name}/{act}/{MODE_IDS[mode]}",
                 grad_factor=CASE_FACTOR.get((name, act, mode)))


@pytest.mark.gpu
def test_fallback_from_full_row_kernels(gpu):
    """Sigmoid on H3 with (512, 512) models: the full-row kernels (gemm_h3_rowln, gemm_h3_row_lnbwd) do LeakyReLU
    only, so every hidden layer runs gemm_x6 + ln_act_fwd_f32 / ln_act_bwd -- the timing spans count one stand-alone
    LayerNorm forward and one backward launch per hidden layer (4 and 4), what RLGPU_H3_ROWFUSE=0 /
    RLGPU_H3_ROWFUSE_BWD=0 give LeakyReLU in test_ppo_rowfuse*.py -- and the results pass the float64 rules."""
    import torch
    from rlgpu.ppo import kernel_timing, kernel_timing_read
    counts = {}

    def spans(p, when):
        if when == "before":
            kernel_timing(True)
        else:
            torch.cuda.synchronize()
            t = kernel_timing_read()
            counts.update(fwd=t["LayerNorm forward"][2], bwd=t["LayerNorm backward"][2])
            kernel_timing(False)

    run_act_case(gpu, act_case("fallback", "sigmoid"), "sigmoid", 2, "fallback/sigmoid/h3", spans)
    assert counts == {"fwd": 4, "bwd": 4}, counts

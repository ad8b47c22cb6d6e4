"""Every 16-bit inference entry point of rlgpu.ppo.PPO against the float64 restatement of its roundings
(tests/infer_reference.py: the reference, its two summation-order yardsticks, rules 0 - 2 and the argmax rule), on the
helper's case table with randomised LayerNorm parameters:

    forward(m, x, half=True)      policy, critic and shared head, on infer::mlp_infer and (RLGPU_FUSED_INFER=0) on the
                                  layer path rows_to_bf16 -> gemm_bf16 -> ln_act_fwd_bf16; the wide cases are refused by
                                  the fused kernel (rlgpu_ppo_fused_infer == 0) and answered by the layer path
    infer_critic                  fused, and on the layer path in chunks (n > max_rows = 128)
    infer_values_wave(m, x)       infer::mlp_infer_wave (the LeakyReLU cases on the fused kernel's tiles)
    guide_logits                  the guide's 16-bit copy (parameter set 1), fused and chunked
    infer_actions_mixed / _rows / _wave with old rows, deterministic: the old version's copy (parameter set 2) through the
                                  sampler's argmax

Each test prints its figures (run with -s); the measured ones are recorded in infer_reference's MEASURED.
"""
import numpy as np
import pytest

import infer_reference as ir

pytestmark = pytest.mark.gpu

WAVE_CASES = [c for c in ir.CASES if c.fused and c.act == "leaky_relu"]
WAVE_IDS = [c.name for c in WAVE_CASES]


def dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)


def run(p, gpu, c, counts, fn):
    """[(n, fn(the first n input rows) as a float32 numpy array)] for n in counts."""
    X = dev(gpu, ir.inputs(c))
    return [(n, fn(X[:n]).float().cpu().numpy()) for n in counts]


def layer_path_engine(gpu, monkeypatch, c):
    """An engine of max_rows = 128 on the layer path: 129 and 300 rows run in chunks."""
    monkeypatch.setenv("RLGPU_FUSED_INFER", "0")
    p = ir.make_engine(gpu, c, max_rows=ir.MAX_ROWS_CHUNKED)
    assert all(ir.fused(p, m) == 0 for m in ir.models_of(c))
    return p


@pytest.mark.parametrize("c", ir.CASES, ids=ir.CASE_IDS)
def test_forward_fused(gpu, c):
    """forward(m, x, half=True) as shipped: infer::mlp_infer where the widths fit its tiles, else (the wide cases, and
    the shared head alone, which ends on no output Linear) the layer path."""
    p = ir.make_engine(gpu, c)
    for m in ir.models_of(c):
        assert ir.fused(p, m) == int(c.fused and m != 2), (c.name, m)
        outs = run(p, gpu, c, ir.ROWS_FUSED, lambda x: p.forward(m, x, half=True))
        ir.check(f"forward {c.name} {ir.MODEL_NAMES[m]}", c.fp16, ir.reference(c, m), outs)
    p.close()


@pytest.mark.parametrize("c", ir.CASES, ids=ir.CASE_IDS)
def test_forward_layer_path(gpu, monkeypatch, c):
    monkeypatch.setenv("RLGPU_FUSED_INFER", "0")
    p = ir.make_engine(gpu, c)
    for m in ir.models_of(c):
        assert ir.fused(p, m) == 0
        outs = run(p, gpu, c, ir.ROWS_FUSED, lambda x: p.forward(m, x, half=True))
        ir.check(f"forward, layer path {c.name} {ir.MODEL_NAMES[m]}", c.fp16, ir.reference(c, m), outs)
    p.close()


@pytest.mark.parametrize("c", ir.CASES, ids=ir.CASE_IDS)
def test_infer_critic(gpu, monkeypatch, c):
    R = ir.reference(c, 1)
    p = ir.make_engine(gpu, c)
    assert ir.fused(p, 1) == int(c.fused)
    ir.check(f"infer_critic {c.name}", c.fp16, R, run(p, gpu, c, ir.ROWS_FUSED + (ir.ROWS,), p.infer_critic))
    p.close()
    p = layer_path_engine(gpu, monkeypatch, c)
    ir.check(f"infer_critic, layer path in chunks {c.name}", c.fp16, R, run(p, gpu, c, ir.ROWS_CHUNKED, p.infer_critic))
    p.close()


@pytest.mark.parametrize("c", WAVE_CASES, ids=WAVE_IDS)
def test_infer_values_wave(gpu, c):
    p = ir.make_engine(gpu, c)
    for m in (0, 1):
        assert p.wave_infer_ok(m)
        outs = run(p, gpu, c, ir.ROWS_WAVE, lambda x: p.infer_values_wave(m, x))
        ir.check(f"infer_values_wave {c.name} {ir.MODEL_NAMES[m]}", c.fp16, ir.reference(c, m), outs)
    p.close()


@pytest.mark.parametrize("c", ir.CASES, ids=ir.CASE_IDS)
def test_guide_logits(gpu, monkeypatch, c):
    """The guide's copy holds parameter set 1 (policy and shared head) while the engine's own hold set 0; its output is
    16-bit storage, so rule 0 is the dtype."""
    import torch
    R = ir.reference(c, 0, 1)
    want = torch.float16 if c.fp16 else torch.bfloat16

    def guide(p):
        def fn(x):
            g = p.guide_logits(x)
            assert g.dtype == want and tuple(g.shape) == (x.shape[0], c.A)
            return g
        return fn

    p = ir.make_engine(gpu, c)
    p.set_guide(ir.version_vector(c, 1).to(gpu))
    ir.check(f"guide_logits {c.name}", c.fp16, R, run(p, gpu, c, ir.ROWS_FUSED, guide(p)))
    p.close()
    p = layer_path_engine(gpu, monkeypatch, c)
    p.set_guide(ir.version_vector(c, 1).to(gpu))
    ir.check(f"guide_logits, layer path in chunks {c.name}", c.fp16, R, run(p, gpu, c, ir.ROWS_CHUNKED, guide(p)))
    p.close()


@pytest.mark.parametrize("c", ir.CASES, ids=ir.CASE_IDS)
def test_old_version_actions(gpu, monkeypatch, c):
    """The old version's copy holds parameter set 2: the deterministic action of every decided row is the argmax of the
    reference's masked logits, the version's on the old rows and the current parameters' on the others."""
    import torch
    masks, old = ir.masks_of(c)
    X, M, OLD = dev(gpu, ir.inputs(c)), dev(gpu, masks), dev(gpu, old)

    def actions(call, n, **kw):
        a = torch.full((n,), -1, dtype=torch.int32, device=gpu)
        call(X[:n], M[:n], deterministic=True, actions=a, **kw)
        return a.cpu().numpy()

    decided = 0
    p = ir.make_engine(gpu, c)
    p.set_version(ir.version_vector(c, 2).to(gpu))
    for n in ir.ROWS_FUSED + (ir.ROWS,):
        decided += ir.check_actions(f"infer_actions_mixed {c.name} n = {n}", c, n,
                                    actions(lambda x, m, **kw: p.infer_actions_mixed(x, m, OLD[:n], step=3, **kw), n))
        if c.fused:
            decided += ir.check_actions(f"infer_actions_rows {c.name} n = {n}", c, n,
                                        actions(p.infer_actions_rows, n, row0=5, step=3, old_rows=OLD[:n]))
    if c in WAVE_CASES:
        for n in ir.ROWS_WAVE:
            decided += ir.check_actions(f"infer_actions_wave {c.name} n = {n}", c, n,
                                        actions(p.infer_actions_wave, n, row0=5, step=3, old_rows=OLD[:n]))
    p.close()
    p = layer_path_engine(gpu, monkeypatch, c)
    p.set_version(ir.version_vector(c, 2).to(gpu))
    for n in ir.ROWS_CHUNKED:
        decided += ir.check_actions(f"infer_actions_mixed, layer path in chunks {c.name} n = {n}", c, n,
                                    actions(lambda x, m, **kw: p.infer_actions_mixed(x, m, OLD[:n], step=3, **kw), n))
    p.close()
    print(f"old version actions {c.name}: {decided} decided rows over every entry point, none wrong")

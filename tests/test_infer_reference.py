"""The float64 restatement of the 16-bit inference forward (tests/infer_reference.py) on the CPU: its rounding
helper, its agreement with torch's own bf16 module chain, what its two yardsticks cost, and that rule 1 rejects every
listed wrong variant while the older 2e-2 max-norm bound (close_16bit) lets most of them through.

Figures of this file, computed on the CPU (policy model, all 300 rows of a case; "share" is the share of outputs not
bit-equal to the float64-accumulated reference):

  * the yardsticks' shares k16 / t32: c2 0.42 % / 0.77 %, odd 0 / 0.015 %, fp16-tanh 2.3 % / 5.3 %, noln-sigmoid
    0.011 % / 0.052 %, shared-bf16 0.007 % / 0.004 %, shared-fp16 1.3 % / 2.2 %, edge-out128 0.026 % / 0.28 %,
    edge-k160 0 / 0, wide-hidden 0.048 % / 0.030 %, wide-in 0.17 % / 0.17 %; the largest |yardstick - ref| is one
    16-bit ulp of the output's scale (3.9e-3 at max |ref| 1.8 in bf16, 9.8e-4 in fp16).
  * torch's bf16 module chain against the reference: c2 0.26 %, wide-hidden 0.16 % (3.3 x its yardsticks, the largest
    ratio), wide-in 0.11 %, every other bf16 case below 0.05 %.
  * the mutants' shares on c2 / odd (rule 1's bound with the floor at its 0.5 % cap: 3.6 % / 0.6 %): unbiased variance
    62 % / 77 %, eps 1e-6 23 % / 16 %, bias unrounded 46 % / 53 %, LayerNorm output unrounded 14 % / 19 %, activation
    output unrounded 11 % / 13 %, gamma / beta shifted one column 99.7 % / 99.7 %, gamma / beta of the layer before
    99.5 % (c2, the one case with two equal widths), obs truncated 72 % / 71 %, last input column dropped 93 % / 91 %.
  * close_16bit (2e-2 max |ref| + 1e-3) lets through, on every case: unbiased variance (at most 1.4e-2 of max |ref|),
    eps 1e-6, bias unrounded, LayerNorm output unrounded, activation output unrounded and obs truncated (each at most
    9.5e-3); it rejects only the two gamma / beta mutants (0.4 .. 0.66) and the dropped column (4.3e-2 .. 0.23).
"""
import numpy as np
import pytest

import infer_reference as ir

BF16_CASES = [c for c in ir.CASES if not c.fp16]
LN_MUTANTS = ("unbiased_variance", "eps_1e-6", "ln_unrounded", "gamma_shift", "gamma_prev_layer")


def test_r16_ties_and_casts():
    """Round to nearest even on hand-written ties, NaN and overflow; bf16 against torch's cast and fp16 against numpy's
    over random values, subnormals and huge values."""
    import torch
    e = 2.0 ** -8  # half a bf16 ulp at 1
    ties = np.array([1 + e, 1 + 3 * e, -(1 + e), -(1 + 3 * e), 1 + 5 * e, 1 + e + 2.0 ** -20, 1 + e - 2.0 ** -20], np.float32)
    want = np.array([1.0, 1 + 4 * e, -1.0, -(1 + 4 * e), 1 + 4 * e, 1 + 2 * e, 1.0], np.float32)
    assert np.array_equal(ir.r16(ties, False), want)
    h = 2.0 ** -11  # half an fp16 ulp at 1
    assert np.array_equal(ir.r16(np.array([1 + h, 1 + 3 * h, -(1 + h), 70000.0], np.float32), True),
                          np.array([1.0, 1 + 4 * h, -1.0, np.inf], np.float32))
    for fp16 in (False, True):
        special = ir.r16(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32), fp16)
        assert np.isnan(special[0]) and special[1] == np.inf and special[2] == -np.inf
        assert np.array_equal(ir.bits(special[3:]), ir.bits(np.array([0.0, -0.0], np.float32)))
        assert ir.r16(np.float64(1.0 + 2.0 ** -30), fp16) == 1.0  # float64 in: rounded to fp32 first
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(20000), rng.standard_normal(2000) * 1e-41, rng.standard_normal(2000) * 1e37,
                        rng.standard_normal(2000) * 1e-6, ties]).astype(np.float32)
    assert np.array_equal(ir.bits(ir.r16(x, False)), ir.bits(torch.from_numpy(x).to(torch.bfloat16).float().numpy()))
    with np.errstate(over="ignore"):
        assert np.array_equal(ir.bits(ir.r16(x, True)), ir.bits(x.astype(np.float16).astype(np.float32)))
    for fp16 in (False, True):  # the mutant's truncation: never away from zero, at most one ulp off, a fixed point on 16-bit values
        t, r = ir.trunc16(x[:24000], fp16), ir.r16(x[:24000], fp16)
        fin = np.isfinite(r)
        assert (np.abs(t[fin]) <= np.abs(x[:24000][fin])).all() and np.array_equal(ir.trunc16(r[fin], fp16), r[fin])
        assert (t != r).mean() > 0.3
    assert ir.ulp16(1.5, False) == 2.0 ** -7 and ir.ulp16(1.5, True) == 2.0 ** -10 and ir.ulp16(0.75, False) == 2.0 ** -8


def test_the_table_holds_every_kind():
    """The case table's kinds, and what the GPU tests rely on: the wide cases alone are off the fused kernel's tiles."""
    by = {c.name: c for c in ir.CASES}
    assert by["c2"].pol == (512, 512) and by["c2"].obs == 167 and by["c2"].A == 90 and not by["c2"].fp16
    assert by["odd"].edge and by["fp16-tanh"].fp16 and by["fp16-tanh"].act == "tanh"
    assert not by["noln-sigmoid"].ln and by["noln-sigmoid"].act == "sigmoid"
    assert by["shared-bf16"].shared == (96, 64) and by["shared-fp16"].fp16 and by["edge-out128"].A == 128
    for c in ir.CASES:
        widths = [c.obs, *c.shared, *c.pol, *c.crit]
        assert c.fused == (max(widths) <= 512 and c.A <= 128), c.name
    x = ir.inputs(by["odd"])
    assert not x[0].any() and set(np.abs(x[1]).tolist()) == {1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8}
    assert np.abs(x[2]).max() > 1000 and 0 < np.abs(x[3]).max() < 1e-5


@pytest.mark.parametrize("c", ir.CASES, ids=ir.CASE_IDS)
def test_yardstick_shares(c):
    """What a change of summation order alone costs, per case and model (printed: run with -s), and that the three
    statements are one function: the yardsticks stay within one 16-bit ulp of the output scale per 4 (rule 2's bound
    is finite and small) and below a 10 % share."""
    for m in ir.models_of(c):
        R = ir.reference(c, m)
        f = ir.figures(c.fp16, R, [(ir.ROWS, R.ya)])
        print(f"{c.name} {ir.MODEL_NAMES[m]}: k16 {100 * f.share_ya:.3f} % t32 {100 * f.share_yb:.3f} %, max err k16 "
              f"{f.err_ya:.2e} t32 {f.err_yb:.2e}, max |ref| {f.ref_max:.3f}, rule 1 bound {100 * f.bound1:.3f} %, rule 2 "
              f"bound {f.bound2:.2e}")
        assert max(f.share_ya, f.share_yb) < 0.10
        assert max(f.err_ya, f.err_yb) <= 2 * ir.ulp16(f.ref_max, c.fp16)


@pytest.mark.parametrize("c", BF16_CASES, ids=[c.name for c in BF16_CASES])
def test_reference_is_the_torch_bf16_chain(c):
    """forward16("f64") against torch's CPU bf16 module chain (one rounding per module output, the reference project's
    Model::Forward on the bf16 copy): within rules 1 and 2 measured from the yardsticks -- the rounding points are
    torch's, not an invention."""
    import torch
    for m in ir.models_of(c):
        with torch.no_grad():
            x = torch.from_numpy(ir.inputs(c).copy()).to(torch.bfloat16)
            want = ir.torch_chain(c, m).to(torch.bfloat16)(x).float().numpy()
        ir.check(f"torch bf16 chain, {c.name} {ir.MODEL_NAMES[m]}", False, ir.reference(c, m), [(ir.ROWS, want)])


@pytest.mark.parametrize("c", ir.CASES, ids=ir.CASE_IDS)
def test_action_rows_are_decided(c):
    """The argmax rule's side condition: at least half of the rows of every case have a top-two gap above twice rule
    2's bound, under the current and the old version's parameters (action_rows asserts it)."""
    want, decided = ir.action_rows(c)
    masks, old = ir.masks_of(c)
    assert old.any() and not old.all() and (masks.sum(1) >= 2).all()
    assert (masks[np.arange(ir.ROWS), want] == 1).all()
    print(f"{c.name}: {decided.sum()} of {ir.ROWS} rows decided")


@pytest.fixture(scope="module")
def mutant_table():
    """{mutant: {case name: (share, rule 1's bound with the floor at its cap, max err / max |ref|, close_16bit passes)}}
    on the policy of every case."""
    table = {}
    for mu in ir.MUTANTS:
        table[mu] = {}
        for c in ir.CASES:
            if mu in LN_MUTANTS and not c.ln:
                continue
            R = ir.reference(c, 0)
            f = ir.figures(c.fp16, R, [(ir.ROWS, ir.mutant_output(c, 0, mu))], floor=ir.FLOOR_CAP)
            table[mu][c.name] = (f.share, f.bound1, f.err / f.ref_max, f.err <= 2e-2 * f.ref_max + 1e-3)
    return table


@pytest.mark.parametrize("mutant", ir.MUTANTS)
def test_every_mutant_is_rejected(mutant_table, mutant):
    """Rule 1 rejects every listed wrong variant: on at least one case its share of unequal outputs is at least twice
    the case's rule 1 bound, the floor taken at its 0.5 % cap."""
    row = mutant_table[mutant]
    for name, (s, b, e, ok) in row.items():
        print(f"{mutant} {name}: share {100 * s:.2f} % bound {100 * b:.2f} % err {e:.2e} of max |ref| close_16bit {ok}")
    caught = [name for name, (s, b, _, _) in row.items() if s >= 2 * b]
    assert caught, (mutant, row)
    if mutant != "gamma_prev_layer":  # the shipped shape and the odd widths both catch every other one
        assert "c2" in caught and "odd" in caught, (mutant, caught)


def test_max_norm_bound_lets_mutants_through(mutant_table):
    """For the record (module docstring): close_16bit's 2e-2 bound passes six of the nine mutants on every case and
    rejects the gamma / beta mutants and the dropped column alone."""
    passed = {mu: [ok for (_, _, _, ok) in row.values()] for mu, row in mutant_table.items()}
    for mu in ("unbiased_variance", "eps_1e-6", "bias_unrounded", "ln_unrounded", "act_unrounded", "obs_truncated"):
        assert all(passed[mu]), mu
    for mu in ("gamma_shift", "last_column_dropped"):
        assert not any(passed[mu]), mu
    assert not mutant_table["gamma_prev_layer"]["c2"][3]


@pytest.mark.parametrize("name", ["c2", "odd", "shared-fp16"])
def test_column_shift_is_invisible_at_the_initial_layer_norm(name):
    """Why the cases randomise gamma / beta: at weight 1, bias 0 (every inference test's state before this reference)
    shifting them by a column changes no output bit; at the cases' parameters it changes almost every one."""
    c = ir.case(name)
    kw = dict(fp16=c.fp16, layer_norm=c.ln, activation=c.act, slope=c.slope)
    L = ir.chain(c, 0, identity_ln=True)
    assert all((l.g == 1).all() and (l.beta == 0).all() for l in L if l.g is not None)
    plain, shifted = (ir.forward16(ir.inputs(c), L, mutant=mu, **kw) for mu in (None, "gamma_shift"))
    assert np.array_equal(ir.bits(plain), ir.bits(shifted))
    assert ir.share(ir.mutant_output(c, 0, "gamma_shift"), ir.reference(c, 0).ref) > 0.99

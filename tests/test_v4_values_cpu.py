"""CPU: what the RWKV-4 value sweep of tests/test_gpu_v4_values.py stands on (tests/v4_values_table.py holds stressors, recipes and bounds).

  * every stressor BITES: the condition it exists for occurs in V4Ref's own intermediates over the rows the GPU test runs, with numpy's
    overflow and invalid warnings raised as errors in the float64 reference (a stressor that does not bite fails, it is never skipped);
  * the planted quantisation blocks are what they claim, in V4's seven quantised matrices;
  * conditioning: for every case, recipe and compared unit, the distance of V4Ref(float32) from V4Ref(float64) in units of the Fp32 bound.
    A unit the table does not name stays at or below 0.5 (the GPU holds it to the plain bound); a named one is recomputed;
  * the Fp16 simulation: rounded operands against unrounded; a unit the table does not name stays at or below 1.0, a named one is recomputed;
  * the saturation contract: clipped and unclipped checkers separate only where operands saturate;
  * every (stressor, recipe, precision, quantisation) the GPU file parametrises has a bound.

The salt of the planted noise (v4_values_table.QUANT_SALT).  Criterion: the float32 and the float64 checker agree within the Fp32 bound on
every unit of the decode recipe in all four quantised cases.  Salts tried, worst decode figure over the four cases: 0: 0.563 (taken, the
first that holds), 1: 0.540, 2: 0.540, 3: 0.540, 4: 0.540, 5: 0.540 — the figure is `all` + Int8's aa row in every draw, the keys of tens
and not the noise; the V5 / V6 / V7 sweep's blow-ups of 25 x the bound have no counterpart here."""
import numpy as np
import pytest

from oracle import rwkv_ref as R
from tests import v4_ref
from tests import v4_values_table as T
from tests import values_table as VT

IDS = [T.case_id(*c) for c in T.CASES]
UCASES = [c for c in T.CASES if not c[1]]


@pytest.mark.parametrize("stressor,quant", UCASES, ids=[T.case_id(*c) for c in UCASES])
def test_the_stressor_bites_on_the_rows_the_gpu_test_runs(stressor, quant):
    with np.errstate(over="raise", invalid="raise"):
        ref = T.reference(stressor)
    got = T.bites(stressor, ref.probe, T.tensors(stressor))
    print(f"\n[v4 values] bite {stressor}: " + "; ".join(f"{k}: {v[1]:.6g}" for k, v in got.items()))
    assert got or stressor == "ln_spread", "no predicate"           # ln_spread changes every row: it has none
    assert all(ok for ok, _ in got.values()), got
    assert all(np.isfinite(l).all() for l in ref.logits) and all(np.isfinite(s).all() for s in ref.state.values())
    assert np.isfinite(ref.greedy_state).all() and np.isfinite(np.stack(ref.greedy_logits)).all()
    assert ref.base[0][0] == T.CONST_ROW and 0 not in [t for p in ref.base for t in p]


def test_planted_blocks_are_what_they_claim_in_v4s_matrices():
    """The checks of tests/test_values_cpu.py test_planted_blocks_are_what_they_claim, on the V4 tensors: every kind of the format is planted in
    att.receptance.weight, f16's top (Int8: 32768) there and nowhere else, and every planted matrix dequantises to finite values."""
    for quant in (R.QUANT_INT8, R.QUANT_NF4):
        t = T.tensors(T.QUANT_BLOCKS, quant)
        top = T.F16_MAX if quant == R.QUANT_NF4 else 32768.0
        n = R.INT8_BLOCK if quant == R.QUANT_INT8 else R.NF4_BLOCK
        for l in range(T.LAYERS):
            for name in v4_ref.QUANT_NAMES:
                w = t[f"blocks.{l}.{name}"]
                kinds = {k for _, _, k in T.planted_blocks(name, w.shape, quant)}
                want = set(VT.QUANT_KINDS) - (set() if quant == R.QUANT_NF4 else {"nf4_midpoints"}) - (set() if name == VT.F16_MAX_IN else {"f16_max"})
                assert kinds == want, (name, kinds)
                assert (float(np.abs(w.astype(np.float32)).max()) == top) == (name == VT.F16_MAX_IN), name
                assert np.isfinite(R.fake_quant(w, quant).astype(np.float32)).all(), name
                zero = [(r, c) for r, c, k in T.planted_blocks(name, w.shape, quant) if k == "zero"]
                assert zero and all(not w[r, c:c + n].any() for r, c in zero)
    assert set(v4_ref.QUANT_NAMES) == {"att.receptance.weight", "att.key.weight", "att.value.weight", "att.output.weight",
                                       "ffn.key.weight", "ffn.value.weight", "ffn.receptance.weight"}


def _recomputed(name, got, table, plain_limit, rel):
    """A unit the table names: its figure is the table's within `rel`; any other stays at or below `plain_limit`."""
    for k, v in got.items():
        if k in table:
            assert abs(v - table[k]) <= rel * table[k], (name, k, v, table[k])
        else:
            assert v <= plain_limit, (name, k, v, "needs a derived bound in tests/v4_values_table.py")
    assert set(table) <= set(got), (name, set(table) - set(got))


@pytest.mark.parametrize("stressor,quant", T.CASES, ids=IDS)
def test_the_float32_checker_resolves_every_unit_or_the_table_names_it(stressor, quant):
    """Conditioning (a condition, not a measurement).  A named unit is recomputed within 25 %: the figure is fp32 rounding noise, summed
    pairwise by numpy so that it does not depend on a BLAS kernel, but numpy's float32 exp may still differ in its last bit between CPUs."""
    got = T.conditioning(stressor, quant)
    print(f"\n[v4 values] float32 vs float64 / Fp32 bound, {T.case_id(stressor, quant)}: worst {max(got.values()):.3f}; above 0.45: " +
          " ".join(f"{k[0]}.{k[1]}={v:.3f}" for k, v in got.items() if v > 0.45))
    _recomputed((stressor, quant), got, T.FP32_DERIVED.get((stressor, quant), {}), 0.5, 0.25)
    if quant:                                                     # the criterion of QUANT_SALT
        assert max(v for k, v in got.items() if k[0] == "decode") <= 1.0


@pytest.mark.parametrize("stressor,quant", T.CASES, ids=IDS)
def test_the_derived_fp16_bounds_are_what_the_simulation_gives(stressor, quant):
    """V4Ref(round_operands=("wo", "ffn1", "fv", "head"), clip_operands=True) against itself unrounded on the recipes' own rows, float64 both:
    2 % covers another libm's exp."""
    got = T.simulate_fp16(stressor, quant)
    print(f"\n[v4 values] simulated Fp16 error / 1e-3 tolerance, {T.case_id(stressor, quant)}: worst {max(got.values()):.3f}; above 1: " +
          " ".join(f"{k[0]}.{k[1]}={v:.3f}" for k, v in got.items() if v > 1.0))
    _recomputed((stressor, quant), got, T.FP16_DERIVED.get((stressor, quant), {}), 1.0, 0.02)


def test_every_run_of_the_gpu_file_has_a_bound():
    n = 0
    for stressor, quant in T.CASES:
        for fp32 in (True, False):
            for recipe in T.recipes_of(quant):
                for unit in T.UNITS:
                    c = T.cap(stressor, quant, fp32, recipe, unit)
                    assert np.isfinite(c) and c >= 1.0
                    n += 1
    for table in (T.FP32_DERIVED, T.FP16_DERIVED):                   # and the tables name nothing the GPU file does not run
        for case, units in table.items():
            assert case in T.CASES and all(r in T.recipes_of(case[1]) and u in T.UNITS for r, u in units), case
    assert n == 2 * len(T.UNITS) * (9 * len(T.RECIPES) + 4 * len(T.QUANT_RECIPES))


@pytest.mark.parametrize("stressor,quant", UCASES, ids=[T.case_id(*c) for c in UCASES])
def test_clipped_and_unclipped_checkers_separate_only_where_operands_saturate(stressor, quant):
    toks = [T.base_tokens(b)[:24] for b in range(T.NSLOT)]
    plain, clip = T.make_model(stressor, clip=False), T.make_model(stressor, clip=True)
    a = [plain.forward(p, plain.init_state(), full=True) for p in toks]
    b = [clip.forward(p, clip.init_state(), full=True) for p in toks]
    if stressor == "ffn_saturating":
        gap = max(T.unit_ratio(x, y, T.FP16_TOL) for A, B in zip(a, b) for x, y in zip(A, B))
        print(f"\n[v4 values] clipped vs unclipped logits: {gap:.1f} x the Fp16 tolerance")
        assert gap > 10.0, gap
    else:
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_default_arithmetic_did_not_move():
    """`clip_operands`, `round_operands`, `pairwise_sums` and `probe` are off by default and then touch nothing: a probed run returns the bits of
    an unprobed one, and blending a LoRA file's whole vectors at alpha = 1 gives the model that holds those vectors."""
    t = v4_ref.synth_v4("v4-tiny")
    toks = v4_ref.prompt(512, 3, 8)
    a, b = v4_ref.V4Ref(t), v4_ref.V4Ref(t)
    b.probe = T.Probe()
    s1, s2 = a.init_state(), b.init_state()
    assert np.array_equal(a.forward(toks, s1, full=True), b.forward(toks, s2, full=True)) and np.array_equal(s1, s2)
    assert b.probe.relu2_n > 0 and b.probe.k_max == a.k_absmax
    stressed = T.tensors("decay_ends")
    lora = {k: v for k, v in stressed.items() if k.endswith("att.time_decay")}
    c, d = v4_ref.V4Ref(v4_ref.blend_lora(T.base(), lora, 1.0)), v4_ref.V4Ref(stressed)
    assert all(np.array_equal(c.w[k], d.w[k]) for k in d.w)
    half = v4_ref.blend_lora(T.base(), lora, 0.5)["blocks.0.att.time_decay"]
    want = np.float32(0.5) * stressed["blocks.0.att.time_decay"].astype(np.float32) + np.float32(0.5) * T.base()["blocks.0.att.time_decay"].astype(np.float32)
    assert half.dtype == np.float32 and np.array_equal(half, want)

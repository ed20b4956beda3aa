"""CPU: what the RWKV-4 dimension sweep of tests/test_gpu_v4_dims.py stands on (tests/v4_sweep_table.py holds the rows and the recipes).

  (a) the reference resolves the device: V4Ref(float32) stays within HALF the Fp32 bound of V4Ref(float64) on every unit the GPU file
      compares (last rows, state per layer and row kind, the Full request, the greedy rows), quantised forms of the 768 row included;
  (b) LiteralV4, BlinkDL's published functions in their own state layout, agrees with V4Ref at the 64 and 192 rows;
  (c) no greedy run of the GPU file hangs on a margin fp32 cannot resolve: the float32 checker picks the float64 checker's ids;
  (d) the checker catches a wrong kernel: eight one-line mistakes, each applied to a float32 restatement of the token function (`Mutant`,
      which without a mistake returns V4Ref(float32)'s bits), must exceed the Fp32 bound on a unit the GPU file compares, at two or more of
      the four rows.

Of the eight, seven are caught at all four rows.  `no_running_max` (p = ww in the output half) is INVISIBLE here by construction and is
asserted to be: with p = ww the output is (exp(pp - ww) aa + v) / (exp(pp - ww) bb + 1), the same quotient scaled by exp(p - ww) above and
below, so it differs from the right form by rounding only until exp(pp - ww) overflows fp32, which needs pp - (u + k) > 88.7.  The
synthetic rows keep |k| below 5 and |u| near 1 (printed), no recipe of step sizes can change that, and sharpening the recipes cannot
help: the mistake lives in the value range, not in a dimension.  It is caught where the values are: under att.key.weight x 36 (the edit
of tests/test_gpu_v4.py's range test, |k| of 50 .. 88) the same mutant leaves the bound by orders of magnitude or goes non-finite, which
the last assertion of that test shows on the 64 row."""
import numpy as np
import pytest

from tests import v4_ref
from tests import v4_sweep_table as S
from tests.v4_literal import LiteralV4

IDS = [S.row_id(i) for i in S.RUN]
QUANTS = [(i, q) for i in S.RUN for q in ((0, 1, 2) if S.quantisable(S.TABLE[i]) else (0,))]
QIDS = [f"{S.row_id(i)}-{('f16', 'int8', 'nf4')[q]}" for i, q in QUANTS]


# ---- (a) --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,quant", QUANTS, ids=QIDS)
def test_float32_checker_stays_within_half_the_fp32_bound_of_the_float64_one(i, quant):
    ref, f32 = S.reference(i, quant), S.reference(i, quant, np.float32)
    units = S.compared_units(ref, f32, S.FP32_TOL)
    for b, ((_, _, lg64, s64), (_, _, lg32, s32)) in enumerate(zip(ref.greedy(), f32.greedy())):
        units[f"greedy.slot{b}.logits"] = max(S.unit_ratio(g, w, S.FP32_TOL) for g, w in zip(lg32, lg64))
        units[f"greedy.slot{b}.state"] = S.state_ratio(s32, s64, S.FP32_TOL)
    lg = max(v for k, v in units.items() if "state" not in k)
    st = max(v for k, v in units.items() if "state" in k)
    print(f"\n[v4 dims] {S.row_id(i)} quant {quant}: float32 vs float64 over {len(units)} units, worst error / Fp32 bound: logits {lg:.4f} "
          f"({lg * S.FP32_TOL:.2e} relative), state per row kind {st:.4f} ({st * S.FP32_TOL:.2e} relative)")
    over = {k: v for k, v in units.items() if not v <= 0.5}
    assert not over, over


# ---- (b) --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
def test_v4_ref_equals_the_literal_blinkdl_functions_at_the_small_rows(i):
    t = S.tensors(i)
    ref, lit = v4_ref.V4Ref(t), LiteralV4(t)
    s, ls = ref.init_state(), lit.new_state()
    for tok in S.base_tokens(i, 0)[:24]:
        got, want = ref.forward([tok], s)[-1], lit.forward(tok, ls)
        assert np.abs(got - want).max() <= 1e-9 * max(1.0, float(np.abs(want).max()))
        for ((l, kind), g), (_, w) in zip(S.state_units(s), S.state_units(lit.to_slab_order(ls))):
            assert np.abs(g - w).max() <= 1e-9 * max(1.0, float(np.abs(w).max())), (l, kind)


# ---- (c) --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,quant", QUANTS, ids=QIDS)
def test_greedy_runs_of_the_gpu_sweep_do_not_hang_on_a_near_tie(i, quant):
    """The 24 greedy steps of the three slots of the 3-row step: an fp32 evaluation of the checker picks the float64 one's ids, and the
    smallest gap between the best and the second logit of any step is printed in units of the Fp32 tolerance of its row."""
    want, got = S.reference(i, quant).greedy(), S.reference(i, quant, np.float32).greedy()
    gap = min(float(np.diff(np.sort(row)[-2:])[0]) / (S.FP32_TOL * max(1.0, float(np.abs(row).max()))) for _, _, lgs, _ in want for row in lgs)
    print(f"\n[v4 dims] {S.row_id(i)} quant {quant}: smallest greedy margin {gap:.1f} x the Fp32 tolerance")
    for b in range(3):
        assert got[b][0] == want[b][0] and got[b][1] == want[b][1], b


# ---- (d) --------------------------------------------------------------------------------------------------------------------------
MISTAKES = ("no_running_max", "state_uses_u_plus_k", "mix_k_for_v", "v5_decay", "no_sigmoid_r", "ffn_shift_from_att", "second_row_state",
            "aa_bb_swapped")
INVISIBLE_BY_CONSTRUCTION = ("no_running_max",)                    # argued in the module docstring, asserted below


class Mutant(v4_ref.V4Ref):
    """A float32 restatement of V4Ref's token function with one switchable mistake.  `second_row_state` depends on how a step is formed:
    every step of the sweep feeds a prefix of a base sequence to a fresh slot, so the wrong kernel mixes the row of token index 1 with the
    state row the step began with (zeros) where row 0 belongs; `init_state` marks the beginning of a sequence."""

    def __init__(self, tensors, mistake=None):
        super().__init__(tensors, dtype=np.float32)
        assert mistake is None or mistake in MISTAKES
        self.m, self.t = mistake, 0

    def init_state(self):
        self.t = 0
        return super().init_state()

    def _token(self, token, s, want_logits=True):
        w, m = self.w, self.m
        x = self._ln(w["emb.weight"][token], w["blocks.0.ln0.weight"], w["blocks.0.ln0.bias"])
        for l in range(self.info.num_layer):
            p, a, f = f"blocks.{l}.", f"blocks.{l}.att.", f"blocks.{l}.ffn."
            xx = self._ln(x, w[p + "ln1.weight"], w[p + "ln1.bias"])
            sx_att = s[5 * l].copy()
            s[5 * l] = xx
            sx = np.zeros_like(sx_att) if m == "second_row_state" and self.t == 1 else sx_att
            mix = lambda mu: xx * mu + sx * (1 - mu)
            r = w[a + "receptance.weight"] @ mix(w[a + "time_mix_r"])
            r = r if m == "no_sigmoid_r" else self._sigmoid(r)
            k = w[a + "key.weight"] @ mix(w[a + "time_mix_k"])
            v = w[a + "value.weight"] @ mix(w[a + ("time_mix_k" if m == "mix_k_for_v" else "time_mix_v")])
            aa, bb, pp = s[5 * l + 1], s[5 * l + 2], s[5 * l + 3]
            u = w[a + "time_first"]
            wd = np.exp(-np.exp(w[a + "time_decay"])) if m == "v5_decay" else -np.exp(w[a + "time_decay"])
            ww = u + k
            q = ww if m == "no_running_max" else np.maximum(pp, ww)
            e1, e2 = np.exp(pp - q), np.exp(ww - q)
            wkv = (e1 * aa + e2 * v) / (e1 * bb + e2)
            ww = pp + wd
            ks = u + k if m == "state_uses_u_plus_k" else k
            q = np.maximum(ww, ks)
            e1, e2 = np.exp(ww - q), np.exp(ks - q)
            na, nb = e1 * aa + e2 * v, e1 * bb + e2
            if m == "aa_bb_swapped":
                na, nb = nb, na
            s[5 * l + 1], s[5 * l + 2], s[5 * l + 3] = na, nb, q
            x = x + w[a + "output.weight"] @ (r * wkv)
            xx = self._ln(x, w[p + "ln2.weight"], w[p + "ln2.bias"])
            sx = sx_att if m == "ffn_shift_from_att" else s[5 * l + 4].copy()
            s[5 * l + 4] = xx
            mix = lambda mu: xx * mu + sx * (1 - mu)
            kk = np.maximum(w[f + "key.weight"] @ mix(w[f + "time_mix_k"]), 0) ** 2
            x = x + self._sigmoid(w[f + "receptance.weight"] @ mix(w[f + "time_mix_r"])) * (w[f + "value.weight"] @ kk)
        self.t += 1
        return w["head.weight"] @ self._ln(x, w["ln_out.weight"], w["ln_out.bias"]) if want_logits else None


def test_the_restatement_without_a_mistake_is_the_float32_checker_bit_for_bit():
    a, b = S.reference(1, 0, np.float32), S.Reference(1, Mutant(S.tensors(1)))
    assert all(np.array_equal(x, y) for x, y in zip(a.logits, b.logits))
    assert a.state.keys() == b.state.keys() and all(np.array_equal(a.state[k], b.state[k]) for k in a.state)


_CAUGHT = {}


def caught(i, mistake):
    """(worst error / Fp32 bound over the units the GPU file compares, the unit) of the mutant at row i; a non-finite result counts as inf."""
    if (i, mistake) not in _CAUGHT:
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            units = S.compared_units(S.reference(i), S.Reference(i, Mutant(S.tensors(i), mistake)), S.FP32_TOL)
        units = {k: (v if np.isfinite(v) else np.inf) for k, v in units.items()}
        worst = max(units, key=units.get)
        _CAUGHT[(i, mistake)] = (units[worst], worst)
    return _CAUGHT[(i, mistake)]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_the_checker_catches_a_wrong_kernel(mistake):
    got = [caught(i, mistake) for i in S.RUN]
    print(f"\n[v4 dims] mistake {mistake}: worst error / Fp32 bound per row " +
          " ".join(f"{S.row_id(i)}={r:.3g}@{u}" for i, (r, u) in zip(S.RUN, got)))
    seen = sum(r > 1.0 for r, _ in got)
    if mistake in INVISIBLE_BY_CONSTRUCTION:
        assert seen == 0, (mistake, "became visible: take it off INVISIBLE_BY_CONSTRUCTION", got)
        return
    assert seen >= 2, (mistake, "passes the sweep's bounds", got)


def test_the_dropped_running_maximum_is_invisible_only_because_of_the_value_range():
    """See the module docstring.  On the sweep's rows the exponent the mistake exposes stays far below fp32's overflow; with the keys of
    tests/test_gpu_v4.py's range test it does not, and the very same mutant is caught."""
    i = 0
    t = S.tensors(i)
    seen = []

    def probe(name, layer, a):
        if name == "k":
            seen.append(float(np.abs(a).max()))

    ref = v4_ref.V4Ref(t)
    ref.probe = probe
    S.Reference(i, ref)
    u = max(float(np.abs(t[f"blocks.{l}.att.time_first"].astype(np.float32)).max()) for l in range(S.LAYERS))
    print(f"\n[v4 dims] {S.row_id(i)}: max |k| {max(seen):.2f}, max |u| {u:.2f} over the sweep's rows")
    assert 2.0 * max(seen) + u < 88.0                               # pp <= max k, ww >= -max|k| - |u|: exp(pp - ww) cannot overflow fp32
    big = dict(t)
    for l in range(S.LAYERS):
        n = f"blocks.{l}.att.key.weight"
        big[n] = (t[n].astype(np.float32) * np.float32(36.0)).astype(np.float16)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        units = S.compared_units(S.Reference(i, v4_ref.V4Ref(big)), S.Reference(i, Mutant(big, "no_running_max")), S.FP32_TOL)
        right = S.compared_units(S.Reference(i, v4_ref.V4Ref(big)), S.Reference(i, Mutant(big)), S.FP32_TOL)
    worst = max((v if np.isfinite(v) else np.inf) for v in units.values())
    print(f"[v4 dims] with att.key.weight x 36: the mutant's worst error / Fp32 bound {worst:.3g}, the right form's logits "
          f"{max(v for k, v in right.items() if 'state' not in k):.3g}")
    assert worst > 1.0
    assert max(v for k, v in right.items() if "state" not in k) <= 1.0

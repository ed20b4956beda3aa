"""GPU (-m gpu): the segmented max-plus scan form of the V4 WKV (rwkv_engine_set_wkv_form, RWKV_WKV_SCAN_MAX) through the ABI, against the float64
V4Ref runs of tests/v4_values_table.py, never against the recurrent GPU form.  Models: the value sweep's 2-layer, 128-wide V4 checkpoints (two
64-channel blocks).

Recipes: `full` 130 rows, Full, one slot (every position inside a segment, three chunks, a ragged last chunk of 2); `mixed` four slots, two Last
calls of (70, 1, 16, 33) and (1, 64, 17, 5) rows (carry across calls, one-row sequences beside long ones, an exact 64); `tile` 250 rows, Last;
`long` 600 rows in one Last call (ten chunks for the carry to compound over; under `keys_large` the sums overflow without the running maximum).
Units as in the value sweep: the logits per row, the state per layer and row kind, each against its own |ref|_inf, in units of 2e-5 (Fp32) /
1e-3 (Fp16).  `tile` and `long` compare the rows the sweep's caps were derived on and are held to v4_values_table.cap unchanged (2 x the float32
checker's own distance from float64; the scan's exponents are of the walk's kind).  `full` and `mixed` run only the stressors whose derived
figures stay below 0.5 up to 250 rows and are held to the plain bound 1.0.  Every worst error / tolerance is printed and appended to the file
RWKV_WKV_SCAN_JSONL names, if set."""
import json
import os

import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import v4_values_table as T
from tests import values_table as T6

pytestmark = pytest.mark.gpu
TOL = {rt.Precision.Fp32: T.FP32_TOL, rt.Precision.Fp16: T.FP16_TOL}
MAX = rt.WkvForm.ScanMax
FULL_ROWS = 130
MIXED = ((70, 1, 16, 33), (1, 64, 17, 5))
MAX_KERNELS = {"wkv4_scan_local_kernel", "wkv4_scan_carry_kernel", "wkv4_scan_out_kernel"}
SHORT_STRESSORS, LONG_STRESSORS = ["decay_ends", "bonus_large"], ["decay_ends", "keys_large", "bonus_large", T.ALL]
CASES = [(r, s) for r in ("full", "mixed") for s in SHORT_STRESSORS] + [(r, s) for r in ("tile", "long") for s in LONG_STRESSORS]
_STEPPED = {}


def slot_tokens(ref, b):
    return ref.base[0][100 * b:100 * b + MIXED[0][b] + MIXED[1][b]]


def stepped_reference(stressor):
    """Token by token on the float64 checker, shared by both precisions: ("full", the state after 130 rows) and per slot of `mixed` the logits
    after each of the two calls and the final state."""
    if stressor not in _STEPPED:
        ref = T.reference(stressor)
        st = ref.state[(0, T.CHUNK32_ROWS)].copy()                    # the checker's state after 70 rows, stepped on to 130
        for tok in ref.base[0][T.CHUNK32_ROWS:FULL_ROWS]:
            ref.model.forward([tok], st)
        mixed = []
        for b in range(T.NSLOT):
            s, rows = ref.model.init_state(), []
            for tok in slot_tokens(ref, b):
                rows.append(ref.model.forward([tok], s)[-1])
            mixed.append((rows[MIXED[0][b] - 1], rows[-1], s))
        _STEPPED[stressor] = (st, mixed)
    return _STEPPED[stressor]


def run_recipe(recipe, stressor, prec):
    ref, t = T.reference(stressor), T.Tally(TOL[prec])
    mb = rt.ModelBuilder(R.st_serialize(T.tensors(stressor)))
    if recipe == "mixed":
        eng = mb.build(max_batch=T.NSLOT, token_chunk_size=128, precision=prec, wkv_form=MAX)
        want, pos = stepped_reference(stressor)[1], [0] * T.NSLOT
        for call, lens in enumerate(MIXED):
            _, outs = eng.infer(rt.RnnInput([rt.RnnInputBatch(slot_tokens(ref, b)[pos[b]:pos[b] + lens[b]], rt.RnnOption.Last) for b in range(T.NSLOT)]))
            pos = [p + n for p, n in zip(pos, lens)]
            for b in range(T.NSLOT):
                t.row(outs[b][-1], want[b][call])
        for b in range(T.NSLOT):
            t.slab(eng.state.back(b), want[b][2])
    else:
        n = {"full": FULL_ROWS, "tile": T.TILE_ROWS, "long": T.LONG_ROWS}[recipe]
        eng = mb.build(max_batch=1, token_chunk_size=n, precision=prec, wkv_form=MAX)
        _, outs = eng.infer(rt.RnnInput([rt.RnnInputBatch(ref.base[0][:n], rt.RnnOption.Full if recipe == "full" else rt.RnnOption.Last)]))
        if recipe == "full":
            assert len(outs[0]) == n
            for r in range(n):
                t.row(outs[0][r], ref.logits[0][r])
            t.slab(eng.state.back(0), stepped_reference(stressor)[0])
        else:
            assert len(outs[0]) == 1
            t.row(outs[0][-1], ref.logits[0][n - 1])
            t.slab(eng.state.back(0), ref.state[(0, n)])
    assert eng.wkv_form == MAX
    eng.close()
    return t


@pytest.mark.parametrize("prec", list(TOL), ids=["fp32", "fp16"])
@pytest.mark.parametrize("recipe,stressor", CASES, ids=[f"{r}-{s}" for r, s in CASES])
def test_max_form_matches_v4_ref(recipe, stressor, prec):
    t = run_recipe(recipe, stressor, prec)
    fp32 = prec == rt.Precision.Fp32
    caps = {u: T.cap(stressor, 0, fp32, recipe, u) if recipe in ("tile", "long") else 1.0 for u in T.UNITS}
    line = {"recipe": recipe, "version": 4, "stressor": stressor, "precision": prec.name, **{u: round(t.worst[u], 4) for u in T.UNITS}}
    print(f"\n[wkv4_scan] {line}")
    if os.environ.get("RWKV_WKV_SCAN_JSONL"):
        with open(os.environ["RWKV_WKV_SCAN_JSONL"], "a") as f:
            f.write(json.dumps(line) + "\n")
    assert t.finite                                                   # a NaN or an overflowed sum is reported as such
    over = {u: (round(t.worst[u], 3), caps[u]) for u in T.UNITS if not t.worst[u] <= caps[u]}
    assert not over, f"error / tolerance above the unit's bound {{unit: (figure, bound)}}: {over}"


def test_multi_row_steps_launch_the_three_max_kernels(tmp_path):
    ref, log = T.reference("decay_ends"), str(tmp_path / "launch.jsonl")
    os.environ["RWKV_LAUNCH_LOG"] = log
    try:
        eng = rt.ModelBuilder(R.st_serialize(T.tensors("decay_ends"))).build(max_batch=2, token_chunk_size=80, wkv_form=MAX)
    finally:
        os.environ.pop("RWKV_LAUNCH_LOG", None)
    eng.infer(rt.RnnInput([rt.RnnInputBatch(ref.base[0][:70], rt.RnnOption.Last), rt.RnnInputBatch(ref.base[1][:1], rt.RnnOption.Last)]))
    eng.infer(rt.RnnInput([rt.RnnInputBatch(ref.base[0][70:71], rt.RnnOption.Last), rt.RnnInputBatch(ref.base[1][1:2], rt.RnnOption.Last)]))
    eng.close()
    wkv = [d for d in map(json.loads, open(log)) if d["kind"] == "row" and d["kernel"].startswith("wkv")]
    assert {d["kernel"] for d in wkv if d["T"] == 71} == MAX_KERNELS                       # the multi-row step, the one-row sequence included
    assert {d["kernel"] for d in wkv if d["T"] == 2} == {"wkv4_kernel"}                    # one-row steps keep the decode kernel
    assert [d["grid"] for d in wkv if d["T"] == 71 and d["kernel"] == "wkv4_scan_carry_kernel"][0] == 2 * (T.width(0) // 64)


def test_a_v6_engine_refuses_the_max_form_and_is_left_unchanged():
    ref = T6.reference(6, "bonus_large")
    outs = []
    for ask in (False, True):
        eng = rt.ModelBuilder(R.st_serialize(ref.tens)).build(max_batch=1, token_chunk_size=40, precision=rt.Precision.Fp32)
        if ask:
            with pytest.raises(rt.RwkvError) as e:
                eng.set_wkv_form(MAX)
            assert e.value.code == -3 and eng.wkv_form == rt.WkvForm.Recurrent
        outs.append([r.copy() for r in eng.infer(rt.RnnInput([rt.RnnInputBatch(ref.base[0][:40], rt.RnnOption.Full)]))[1][0]])
        eng.close()
    assert len(outs[0]) == 40 and all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))


def test_a_v4_engine_refuses_the_matrix_forms_and_takes_the_max_form():
    eng = rt.ModelBuilder(R.st_serialize(T.tensors("bonus_large"))).build(max_batch=1, token_chunk_size=16)
    for form in (rt.WkvForm.Scan, rt.WkvForm.ScanDelta):
        with pytest.raises(rt.RwkvError) as e:
            eng.set_wkv_form(form)
        assert e.value.code == -3 and eng.wkv_form == rt.WkvForm.Recurrent
    eng.set_wkv_form(MAX)
    assert eng.wkv_form == MAX
    eng.close()

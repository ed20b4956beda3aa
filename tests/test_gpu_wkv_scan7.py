"""GPU (-m gpu): the chunked matrix form of the V7 WKV (rwkv_engine_set_wkv_form, RWKV_WKV_SCAN_DELTA) through the ABI, against the oracle's
lock-step evaluation (tests/values_table.py), never against the recurrent GPU form.  Models: the value sweep's 2-layer, 128-wide V7 checkpoints
(layer 0 writes v_first, layer 1 reads it) under `bonus_large`, `decay_ends` (w at both ends of [0.545, 1]) and `all`.

Recipes: `full` 130 rows, Full, one slot (every position of a 16-token sub-block, three chunks, a ragged last chunk of 2); `mixed` four slots,
two Last calls of (70, 1, 16, 33) and (1, 64, 17, 5) rows (carry across calls, one-row sequences beside long ones, an exact 64); `tile` 250
rows, Last; `long` 600 rows in one Last call (ten chunks, a tail of 24: the carry's two products per chunk have chunks to compound over).
Bounds: logits 2e-5 (Fp32) / 1e-3 (Fp16) x max(1, |ref row|_inf); state the same factor per values_table.state_blocks block.
Worst error / tolerance per case is printed and appended to the file RWKV_WKV_SCAN_JSONL names, if set."""
import json
import os

import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import values_table as T

pytestmark = pytest.mark.gpu
TOL = {rt.Precision.Fp32: 2e-5, rt.Precision.Fp16: 1e-3}
DELTA = rt.WkvForm.ScanDelta
FULL_ROWS = 130
MIXED = ((70, 1, 16, 33), (1, 64, 17, 5))
DELTA_KERNELS = {"wkv7_scan_local_kernel", "wkv7_scan_carry_kernel", "wkv7_scan_out_kernel"}
_MIXED_REF = {}


def slot_tokens(ref, b):
    return ref.base[0][100 * b:100 * b + MIXED[0][b] + MIXED[1][b]]


def mixed_reference(stressor):
    """Per slot: the logits after each of the two calls and the final state, one oracle step per token; shared by both precisions."""
    if stressor not in _MIXED_REF:
        ref, out = T.reference(7, stressor), []
        for b in range(T.NSLOT):
            st, rows = ref.rb.init_states(1), []
            for tok in slot_tokens(ref, b):
                rows.append(ref.rb.step([tok], st)[0])
            out.append((rows[MIXED[0][b] - 1], rows[-1], st[0]))
        _MIXED_REF[stressor] = out
    return _MIXED_REF[stressor]


def ratios(f, rows, slabs):
    """Worst error / tolerance over (got, want) logits rows and over the blocks of (got, want) state slabs; everything finite."""
    lg = max(float(np.abs(g - w).max()) / (f * max(1.0, float(np.abs(w).max()))) for g, w in rows)
    st = max(float(np.abs(g - w).max()) / (f * max(1.0, float(np.abs(w).max())))
             for got, want in slabs for (_, g), (_, w) in zip(T.state_blocks(got), T.state_blocks(want)))
    assert all(np.isfinite(g).all() for g, _ in rows) and all(np.isfinite(g).all() for g, _ in slabs)
    return lg, st


def run_recipe(recipe, stressor, prec):
    ref = T.reference(7, stressor)
    mb = rt.ModelBuilder(R.st_serialize(ref.tens))
    if recipe == "mixed":
        eng = mb.build(max_batch=T.NSLOT, token_chunk_size=128, precision=prec, wkv_form=DELTA)
        want, rows, pos = mixed_reference(stressor), [], [0] * T.NSLOT
        for call, lens in enumerate(MIXED):
            _, outs = eng.infer(rt.RnnInput([rt.RnnInputBatch(slot_tokens(ref, b)[pos[b]:pos[b] + lens[b]], rt.RnnOption.Last) for b in range(T.NSLOT)]))
            pos = [p + n for p, n in zip(pos, lens)]
            rows += [(outs[b][-1].copy(), want[b][call]) for b in range(T.NSLOT)]       # the arena is reused by the next call
        slabs = [(eng.state.back(b), want[b][2]) for b in range(T.NSLOT)]
    else:
        n = {"full": FULL_ROWS, "tile": T.TILE_ROWS, "long": T.LONG_ROWS}[recipe]
        eng = mb.build(max_batch=1, token_chunk_size=n, precision=prec, wkv_form=DELTA)
        _, outs = eng.infer(rt.RnnInput([rt.RnnInputBatch(ref.base[0][:n], rt.RnnOption.Full if recipe == "full" else rt.RnnOption.Last)]))
        if recipe == "full":
            assert len(outs[0]) == n
            rows = [(outs[0][r], ref.logits[0][r]) for r in range(n)]
            st = ref.state[(0, T.CHUNK32_ROWS)][None].copy()              # the oracle's state after 70 rows, stepped on to 130
            for tok in ref.base[0][T.CHUNK32_ROWS:n]:
                ref.rb.step([tok], st)
            slabs = [(eng.state.back(0), st[0])]
        else:
            rows, slabs = [(outs[0][-1], ref.logits[0][n - 1])], [(eng.state.back(0), ref.state[(0, n)])]
    assert eng.wkv_form == DELTA
    res = ratios(TOL[prec], rows, slabs)                              # before close(): the rows are views of the engine's pinned arena
    eng.close()
    return res


@pytest.mark.parametrize("prec", list(TOL), ids=["fp32", "fp16"])
@pytest.mark.parametrize("stressor", ["bonus_large", "decay_ends", T.ALL])
@pytest.mark.parametrize("recipe", ["full", "mixed", "tile", "long"])
def test_delta_form_matches_the_oracle(recipe, stressor, prec):
    lg, st = run_recipe(recipe, stressor, prec)
    line = {"recipe": recipe, "version": 7, "stressor": stressor, "precision": prec.name, "logits": round(lg, 4), "state": round(st, 4)}
    print(f"\n[wkv_scan7] {line}")
    if os.environ.get("RWKV_WKV_SCAN_JSONL"):
        with open(os.environ["RWKV_WKV_SCAN_JSONL"], "a") as f:
            f.write(json.dumps(line) + "\n")
    assert lg <= 1.0 and st <= 1.0, f"worst error / tolerance (logits, state per block): {(lg, st)}"


def test_multi_row_steps_launch_the_three_delta_kernels(tmp_path):
    ref, log = T.reference(7, "decay_ends"), str(tmp_path / "launch.jsonl")
    os.environ["RWKV_LAUNCH_LOG"] = log
    try:
        eng = rt.ModelBuilder(R.st_serialize(ref.tens)).build(max_batch=2, token_chunk_size=80, wkv_form=DELTA)
    finally:
        os.environ.pop("RWKV_LAUNCH_LOG", None)
    eng.infer(rt.RnnInput([rt.RnnInputBatch(ref.base[0][:70], rt.RnnOption.Last), rt.RnnInputBatch(ref.base[1][:1], rt.RnnOption.Last)]))
    eng.infer(rt.RnnInput([rt.RnnInputBatch(ref.base[0][70:71], rt.RnnOption.Last), rt.RnnInputBatch(ref.base[1][1:2], rt.RnnOption.Last)]))
    eng.close()
    wkv = [d for d in map(json.loads, open(log)) if d["kind"] == "row" and d["kernel"].startswith("wkv")]
    assert {d["kernel"] for d in wkv if d["T"] == 71} == DELTA_KERNELS                     # the multi-row step, the one-row sequence included
    assert {d["kernel"] for d in wkv if d["T"] == 2} == {"wkv_kernel"}                     # one-row steps keep the decode kernel
    assert [d["grid"] for d in wkv if d["T"] == 71 and d["kernel"] == "wkv7_scan_carry_kernel"][0] == 2 * 2


def test_a_v6_engine_refuses_the_delta_form_and_is_left_unchanged():
    ref = T.reference(6, "bonus_large")
    outs = []
    for ask in (False, True):
        eng = rt.ModelBuilder(R.st_serialize(ref.tens)).build(max_batch=1, token_chunk_size=40, precision=rt.Precision.Fp32)
        if ask:
            with pytest.raises(rt.RwkvError) as e:
                eng.set_wkv_form(DELTA)
            assert e.value.code == -3 and eng.wkv_form == rt.WkvForm.Recurrent
        outs.append([r.copy() for r in eng.infer(rt.RnnInput([rt.RnnInputBatch(ref.base[0][:40], rt.RnnOption.Full)]))[1][0]])
        eng.close()
    assert len(outs[0]) == 40 and all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))

"""GPU (-m gpu): RWKV-4 in the dimension sweep (tests/v4_sweep_table.py; the recipes are tests/dims_table.py's): widths 64, 192, 320 and 768
at single steps of exactly 1, 3, 16, 17, 32, 33, 64, 65, 192, 193 and 250 rows, one engine per step size (max_batch and token_chunk_size are
the step's own), in Precision.Fp32 and Fp16, the 768 row also with Int8 and NF4 on every layer.  What no other test runs: V4's three-problem
time-mix launch (Wk, Wv plain, Wr through the sigmoid epilogue, all fp32 out) in the 17-32, 33-192 and tile families, wkv4_chunk_kernel over
more than 25 rows of a sequence, wkv4_kernel at one wave and at a partial last block, K % 128 = 64, F = 32 x odd, V = 16 and 272.

The reference of a row is ONE float64 run of tests/v4_ref.py's V4Ref per (row, quantisation) over twelve base sequences; slot b of every
step feeds a prefix of base sequence b.  tests/test_v4_sweep_cpu.py pins that checker first (float32 against float64, the literal form,
the greedy margins, eight planted mistakes).  Bounds are the project's: 1e-3 (Fp16) and 2e-5 (Fp32) times max(1, |ref|_inf), logits per
row, state per layer and row kind (att shift, aa, bb, pp, ffn shift) against that row's own |ref|_inf.

The engines are built with RWKV_LAUNCH_LOG, one file per (row, precision, quantisation); the last test reads them and proves that the sweep
took the paths it exists for.  Every figure is printed (`-s`) and appended to the file RWKV_V4_SWEEP_JSONL names, if set."""
import json
import os

import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import v4_sweep_table as S

pytestmark = pytest.mark.gpu
PRECS = [rt.Precision.Fp32, rt.Precision.Fp16]
PREC_ID = {rt.Precision.Fp32: "fp32", rt.Precision.Fp16: "fp16"}
QUANT_ID = {0: "f16", 1: "int8", 2: "nf4"}
ATT3 = "att.key.weight+att.value.weight+att.receptance.weight"
_SWEEP, _ST = {}, {}


def factor(prec):
    return S.FP32_TOL if prec == rt.Precision.Fp32 else S.FP16_TOL


def serialized(i):
    if i not in _ST:
        _ST[i] = R.st_serialize(S.tensors(i))
    return _ST[i]


@pytest.fixture(scope="module")
def log_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("launch_logs")


def log_path(log_dir, i, prec, quant):
    return str(log_dir / f"{i}_{PREC_ID[prec]}_{QUANT_ID[quant]}.jsonl")


def build(st, log, B, chunk, prec, quant=0):
    """An engine whose launches of layers 0 / 1 and the head are appended to `log` (the variable is read at engine creation)."""
    os.environ["RWKV_LAUNCH_LOG"] = log
    try:
        return rt.ModelBuilder(st).quant(S.LAYERS if quant else 0, rt.Quant(quant)).build(max_batch=B, token_chunk_size=chunk, precision=prec)
    finally:
        os.environ.pop("RWKV_LAUNCH_LOG", None)


def greedy_check(eng, want, prec):
    """decode_greedy for GREEDY_STEPS steps on the three slots of the 3-row step against the checker's greedy ids (`want`: Reference.greedy()).
    A slot's first differing id must be a near-tie of the reference (its own gap at most twice the measured error of that row: the rule of
    tests/test_gpu_dims.py greedy_check), measured by replaying the reference's ids through `infer` from a snapshot.  Returns (slots that
    diverged on a near-tie, worst error / tolerance of the replayed rows, the same of the state after an undiverged run)."""
    B, n = len(want), S.GREEDY_STEPS
    snaps = [eng.state.read(b) for b in range(B)]
    got, _ = eng.decode_greedy([w[0] for w in want], n)
    split = {}
    for b in range(B):
        bad = [s for s in range(n) if int(got[s, b]) != want[b][1][s]]
        if bad:
            split[b] = bad[0]
    worst = state = 0.0
    for b in range(B):
        if b not in split:                                        # the ids agreed: the state after 24 steps is the checker's
            state = max(state, S.state_ratio(eng.state.back(b), want[b][3], factor(prec)))
    if split:
        for b in range(B):
            eng.state.write(snaps[b], b)
        cur = [w[0] for w in want]
        for s in range(max(split.values()) + 1):
            _, outs = eng.infer(rt.RnnInput([rt.RnnInputBatch([cur[b]], rt.RnnOption.Last) for b in range(B)]))
            for b in range(B):
                row = want[b][2][s]
                err = float(np.abs(outs[b][-1] - row).max())
                worst = max(worst, S.unit_ratio(outs[b][-1], row, factor(prec)))
                if split.get(b) == s:
                    gi, wi = int(got[s, b]), want[b][1][s]
                    assert float(row[wi] - row[gi]) <= 2.0 * err, ("greedy ids differ beyond a near-tie", b, s, gi, wi, err)
            cur = [want[b][1][s] for b in range(B)]
    return len(split), worst, state


def run_sweep(i, prec, quant, log_dir):
    """Every step size, the Full request and the greedy run of one (row, precision, quantisation); returns {case: worst error / tolerance} and
    the structural failures (a step of the wrong size).  Memoised: the path proof reads the logs these runs leave."""
    key = (i, prec, quant)
    if key in _SWEEP:
        return _SWEEP[key]
    ref, st, f = S.reference(i, quant), serialized(i), factor(prec)
    log = log_path(log_dir, i, prec, quant)
    ratios, wrong = {}, []
    for N in S.STEP_SIZES:
        lens = S.step_lengths(N)
        B = len(lens)
        eng = build(st, log, B, N, prec, quant)
        inp = rt.RnnInput([rt.RnnInputBatch(list(ref.base[b][:lens[b]]), rt.RnnOption.Last) for b in range(B)])
        before = inp.num_token()
        plan = rt.plan_chunk(lens, eng.token_chunk_size)
        inp, outs = eng.infer(inp)
        if not (eng.token_chunk_size == N and plan == lens and before - inp.num_token() == sum(plan) == N):
            wrong.append((N, eng.token_chunk_size, plan, before, inp.num_token()))
        lg = sl = 0.0
        for b in range(B):
            assert len(outs[b]) == 1, (N, b, len(outs[b]))
            assert np.isfinite(outs[b][-1]).all() and np.isfinite(eng.state.back(b)).all(), (N, b)
            lg = max(lg, S.unit_ratio(outs[b][-1], ref.logits[b][lens[b] - 1], f))
            sl = max(sl, S.state_ratio(eng.state.back(b), ref.state[(b, lens[b])], f))
        ratios[f"step{N}"], ratios[f"step{N}_state"] = lg, sl
        if N == 3:                                                # the greedy run goes on from this step's three slots
            ntie, gw, gs = greedy_check(eng, ref.greedy(), prec)
            ratios["greedy_replay"], ratios["greedy_state"], ratios["greedy_near_ties"] = gw, gs, float(ntie)
        eng.close()
    eng = build(st, log, 1, S.FULL_ROWS, prec, quant)              # one Full request: every row of the step is an output row
    inp = rt.RnnInput([rt.RnnInputBatch(list(ref.base[0][:S.FULL_ROWS]), rt.RnnOption.Full)])
    inp, outs = eng.infer(inp)
    if inp.num_token() != 0 or len(outs[0]) != S.FULL_ROWS:
        wrong.append(("full", inp.num_token(), len(outs[0])))
    else:
        ratios["full65"] = max(S.unit_ratio(outs[0][t], ref.logits[0][t], f) for t in range(S.FULL_ROWS))
    eng.close()
    print(f"\n[v4 dims] {S.row_id(i)} {PREC_ID[prec]} {QUANT_ID[quant]}: worst error / tolerance (logits, state per row kind) " +
          " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    if os.environ.get("RWKV_V4_SWEEP_JSONL"):
        with open(os.environ["RWKV_V4_SWEEP_JSONL"], "a") as fh:
            fh.write(json.dumps({"sweep": "dims", "row": S.row_id(i), "precision": PREC_ID[prec], "quant": QUANT_ID[quant],
                                 **{k: round(v, 4) for k, v in ratios.items()}}) + "\n")
    _SWEEP[key] = (ratios, wrong)
    return _SWEEP[key]


def check_sweep(i, prec, quant, log_dir):
    ratios, wrong = run_sweep(i, prec, quant, log_dir)
    assert not wrong, f"steps of the wrong size (N, chunk, plan, tokens before, after): {wrong}"
    over = {k: v for k, v in ratios.items() if k != "greedy_near_ties" and not v <= 1.0}
    assert not over, f"{S.row_id(i)} {PREC_ID[prec]} {QUANT_ID[quant]}: error / tolerance above 1: {over} (all: {ratios})"
    assert ratios["greedy_near_ties"] <= 1, ratios                  # near-ties are rare: three slots, 24 steps


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_ID[p] for p in PRECS])
@pytest.mark.parametrize("i", S.RUN, ids=[S.row_id(i) for i in S.RUN])
def test_every_step_size_full_request_and_greedy_match_v4_ref(i, prec, log_dir):
    check_sweep(i, prec, 0, log_dir)


QROWS = [i for i in S.RUN if S.quantisable(S.TABLE[i])]


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_ID[p] for p in PRECS])
@pytest.mark.parametrize("quant", [1, 2], ids=["int8", "nf4"])
@pytest.mark.parametrize("i", QROWS, ids=[S.row_id(i) for i in QROWS])
def test_the_quantisable_row_matches_v4_ref_with_the_same_quantisation(i, quant, prec, log_dir):
    check_sweep(i, prec, quant, log_dir)


NOQ = [i for i in S.RUN if i not in QROWS]


@pytest.mark.parametrize("i", NOQ, ids=[S.row_id(i) for i in NOQ])
def test_rows_that_cannot_be_quantised_are_refused_before_any_kernel_runs(i, log_dir):
    log = str(log_dir / f"refused_quant_{i}.jsonl")
    for quant in (1, 2):
        with pytest.raises(rt.RwkvError) as e:
            build(serialized(i), log, 2, 16, rt.Precision.Fp16, quant)
        assert e.value.code == -3 and "multiples of 256" in str(e.value)
    assert not os.path.exists(log) or os.path.getsize(log) == 0     # refused at build time: the engine launched nothing


@pytest.mark.parametrize("j", range(len(S.REFUSED)), ids=["C96", "V50277"])
def test_shapes_outside_the_loaders_lattice_are_refused_by_name(j, log_dir):
    """C = 96 (no multiple of 64) and the Pile vocabulary of 50277 (no multiple of 16): RWKV_ERR_UNSUPPORTED, the rule in the message, nothing launched."""
    log = str(log_dir / f"refused_shape_{j}.jsonl")
    with pytest.raises(rt.RwkvError) as e:
        build(R.st_serialize(S.refused_tensors(j)), log, 2, 16, rt.Precision.Fp16)
    assert e.value.code == -3 and S.REFUSAL in str(e.value), str(e.value)
    assert not os.path.exists(log) or os.path.getsize(log) == 0


def test_the_sweep_took_the_paths_it_exists_for(log_dir):
    """From the engines' own launch logs (the runs above, or run here when this test is selected alone): both WKV-4 kernels on every row; the
    three-matrix time-mix launch in the tile family at T >= 193 in both precisions, and the same launch at 33 .. 192 and at 17 .. 32 rows; the
    chunked tile kernel at K % 128 != 0 on the 192 and 320 rows; a TAIL decode launch with a K split; both quantised formats in the tile
    family on the 768 row.  Prints the distinct (kind, variant, ksplit) per row."""
    def lines(i, prec, quant=0):
        run_sweep(i, prec, quant, log_dir)
        return [json.loads(l) for l in open(log_path(log_dir, i, prec, quant))]

    def names(d):                                                   # a launch's matrices without their `blocks.N.` prefix
        return "+".join(m.split(".", 2)[-1] if m.startswith("blocks.") else m for m in d["mats"].split("+"))

    def K_of(i, name):
        return S.TABLE[i].F if name == "ffn.value.weight" else S.TABLE[i].C

    seen = {}
    for i in S.RUN:
        for prec in PRECS:
            for d in lines(i, prec):
                if d["kind"] != "row":
                    seen.setdefault((S.row_id(i), PREC_ID[prec]), set()).add((d["kind"], d["variant"], d["ksplit"]))
    for k in sorted(seen):
        print(f"\n[v4 dims] paths {k[0]} {k[1]}: {sorted(seen[k])}")
    for i in S.RUN:
        for prec in PRECS:
            rows = [d for d in lines(i, prec) if d["kind"] == "row"]
            gemms = [d for d in lines(i, prec) if d["kind"] != "row"]
            kernels = {d["kernel"] for d in rows}
            assert {"wkv4_kernel", "wkv4_chunk_kernel"} <= kernels, (S.row_id(i), kernels)
            assert max(d["T"] for d in rows if d["kernel"] == "wkv4_chunk_kernel") == 250
            att = [d for d in gemms if names(d) == ATT3]
            assert att and all(d["rows"] == 3 * S.TABLE[i].C for d in att), S.row_id(i)
            assert not [d for d in gemms if "att.key.weight" in d["mats"] and names(d) != ATT3]     # the composition is the only one
            assert any(d["kind"] == "tile" and d["T"] >= 193 for d in att), (S.row_id(i), PREC_ID[prec], "no three-matrix tile launch")
            assert any(d["kind"] == "decode" and 33 <= d["T"] <= 192 for d in att), (S.row_id(i), PREC_ID[prec], "33 .. 192 rows")
            assert any(d["kind"] != "tile" and 17 <= d["T"] <= 32 for d in att), (S.row_id(i), PREC_ID[prec], "17 .. 32 rows")
    for i in [i for i in S.RUN if S.TABLE[i].C % 128]:
        for prec in PRECS:
            hit = [d for d in lines(i, prec) if d["kind"] == "tile" and d["variant"] < 10 and any(K_of(i, m) % 128 for m in names(d).split("+"))]
            assert hit, f"no chunked tile launch at K % 128 != 0 on {S.row_id(i)} in {PREC_ID[prec]}"
    # decode with a K split whose per-block range is no whole number of 256-k slices (TAIL): Kb = K / ksplit
    tail = [(S.row_id(i), d["T"], d["mats"], d["ksplit"]) for i in S.RUN for prec in PRECS for d in lines(i, prec)
            if d["kind"] == "decode" and d["ksplit"] > 1 and (K_of(i, names(d).split("+")[0]) // d["ksplit"]) % 256]
    assert tail, "no TAIL decode launch with a K split"
    for i in QROWS:
        per_weight = {}
        for quant in (1, 2):
            q = [d for prec in PRECS for d in lines(i, prec, quant) if d["kind"] == "tile" and names(d) == "att.output.weight"]
            assert q, (S.row_id(i), QUANT_ID[quant], "no quantised launch in the tile family")
            per_weight[quant] = q[0]["bytes"] / float(S.TABLE[i].C ** 2)
        print(f"\n[v4 dims] bytes per weight of the logged output projection in the tile family: {per_weight}")
        assert 0.9 < per_weight[1] < 1.3 and 0.45 < per_weight[2] < 0.8, per_weight

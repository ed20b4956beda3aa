"""GPU (-m gpu): RWKV-4 at weight VALUES the synthetic checkpoints never reach (tests/v4_values_table.py): decays at both ends of -exp(d)
(a decay that does nothing, a state forgotten in one token), keys of tens, large bonus terms, LayerNorm weights spread over two decades,
embedding outliers and a zero-variance row, dead channels, relu^2 operands at the top of f16's range and past it (the +-65504 clamp), and
quantisation blocks planted for the device quantisers.  tests/test_v4_values_cpu.py proves on the CPU that every stressor bites on exactly
these rows, that the checker resolves the device there, and recomputes every derived bound.

Recipes (one engine each; 2 layers, 128 wide, quantised 256 wide), those of tests/test_gpu_values.py: decode (3-token prompt, 48 single-token
steps, 4 slots), chunk8 (4 slots x 8 rows, 6 calls), chunk32 (70 rows, Full), tile (250 rows, Last), long (600 tokens by 100, then 16 greedy
steps).  The reference is one float64 V4Ref run per (stressor, quantisation); with `ffn_saturating` and the quantised runs it clamps GEMM
operands like the engine does.

Bounds: logits 2e-5 (Fp32) / 1e-3 (Fp16) x max(1, |ref row|_inf); state the same factors per layer and row kind (att shift, aa, bb, pp, ffn
shift) against that row's own |ref|_inf; a unit named in v4_values_table.FP32_DERIVED / FP16_DERIVED is held to 2 x its figure there;
finiteness asserted on its own.  Every worst error / tolerance is printed (`-s`) and appended to the file RWKV_V4_SWEEP_JSONL names, if set."""
import json
import os

import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import v4_ref
from tests import v4_values_table as T

pytestmark = pytest.mark.gpu
FP32, FP16, RAW = rt.Precision.Fp32, rt.Precision.Fp16, rt.Precision.Fp16Raw
PRECS = [FP32, FP16]
PREC_ID = {FP32: "fp32", FP16: "fp16", RAW: "raw"}
QUANT_ID = {0: "f16", 1: "int8", 2: "nf4"}
_RUN = {}


def factor(prec):
    return T.FP32_TOL if prec == FP32 else T.FP16_TOL


@pytest.fixture(scope="module")
def log_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("launch_logs")


def log_path(log_dir, stressor, prec, quant):
    return str(log_dir / f"{stressor}_{PREC_ID[prec]}_{QUANT_ID[quant]}.jsonl")


def build(st, log, B, chunk, prec, quant):
    os.environ["RWKV_LAUNCH_LOG"] = log
    try:
        return rt.ModelBuilder(st).quant(T.LAYERS if quant else 0, rt.Quant(quant)).build(max_batch=B, token_chunk_size=chunk, precision=prec)
    finally:
        os.environ.pop("RWKV_LAUNCH_LOG", None)


def feed(eng, batches):
    _, outs = eng.infer(rt.RnnInput(batches))
    return outs


def run_recipe(name, ref, st, log, prec, quant, with_greedy=True):
    t = T.Tally(factor(prec))
    base, B, Last, Full = ref.base, T.NSLOT, rt.RnnOption.Last, rt.RnnOption.Full
    if name == "decode":
        eng = build(st, log, B, 16, prec, quant)
        outs = feed(eng, [rt.RnnInputBatch(base[b][:T.PROMPT], Last) for b in range(B)])
        for b in range(B):
            t.row(outs[b][-1], ref.logits[b][T.PROMPT - 1])
        for s in range(T.PROMPT, T.SHORT):
            outs = feed(eng, [rt.RnnInputBatch([base[b][s]], Last) for b in range(B)])
            for b in range(B):
                t.row(outs[b][-1], ref.logits[b][s])
        for b in range(B):
            t.slab(eng.state.back(b), ref.state[(b, T.SHORT)])
    elif name == "chunk8":
        eng = build(st, log, B, B * T.CHUNK8_ROWS, prec, quant)
        for c in range(T.CHUNK8_CALLS):
            lo, hi = c * T.CHUNK8_ROWS, (c + 1) * T.CHUNK8_ROWS
            outs = feed(eng, [rt.RnnInputBatch(base[b][lo:hi], Last) for b in range(B)])
            for b in range(B):
                assert len(outs[b]) == 1
                t.row(outs[b][-1], ref.logits[b][hi - 1])
        for b in range(B):
            t.slab(eng.state.back(b), ref.state[(b, T.CHUNK8_ROWS * T.CHUNK8_CALLS)])
    elif name == "chunk32":
        eng = build(st, log, 1, T.CHUNK32_ROWS, prec, quant)
        outs = feed(eng, [rt.RnnInputBatch(base[0][:T.CHUNK32_ROWS], Full)])
        assert len(outs[0]) == T.CHUNK32_ROWS
        for r in range(T.CHUNK32_ROWS):
            t.row(outs[0][r], ref.logits[0][r])
        t.slab(eng.state.back(0), ref.state[(0, T.CHUNK32_ROWS)])
    elif name == "tile":
        eng = build(st, log, 1, T.TILE_ROWS, prec, quant)
        outs = feed(eng, [rt.RnnInputBatch(base[0][:T.TILE_ROWS], Last)])
        assert len(outs[0]) == 1
        t.row(outs[0][-1], ref.logits[0][T.TILE_ROWS - 1])
        t.slab(eng.state.back(0), ref.state[(0, T.TILE_ROWS)])
    else:
        eng = build(st, log, 1, T.LONG_CALL, prec, quant)
        for lo in range(0, T.LONG_ROWS, T.LONG_CALL):
            outs = feed(eng, [rt.RnnInputBatch(base[0][lo:lo + T.LONG_CALL], Last)])
            t.row(outs[0][-1], ref.logits[0][lo + T.LONG_CALL - 1])
        t.slab(eng.state.back(0), ref.state[(0, T.LONG_ROWS)])
        if with_greedy:
            t.near_tie = greedy(eng, ref, t)
    eng.close()
    return t


def greedy(eng, ref, t):
    """16 greedy steps through decode_greedy against the checker's ids; the first differing id must be a near-tie of the REFERENCE (its own gap
    at most twice the measured error of that row: the rule of tests/test_gpu_knobs.py), measured by replaying the reference's ids through
    `infer` from a snapshot.  Returns 1 if the ids split on a near-tie."""
    snap = eng.state.read(0)
    got, _ = eng.decode_greedy([ref.greedy_first], T.LONG_GREEDY)
    got = [int(x) for x in np.asarray(got)[:, 0]]
    bad = [s for s in range(T.LONG_GREEDY) if got[s] != ref.greedy_ids[s]]
    eng.state.write(snap, 0)
    cur = ref.greedy_first
    for s in range(T.LONG_GREEDY):                               # the replay also checks every greedy row and the state after them
        outs = feed(eng, [rt.RnnInputBatch([cur], rt.RnnOption.Last)])
        want = ref.greedy_logits[s]
        t.row(outs[0][-1], want)
        if bad and bad[0] == s:
            err = float(np.abs(outs[0][-1] - want).max())
            assert float(want[ref.greedy_ids[s]] - want[got[s]]) <= 2.0 * err, ("greedy ids differ beyond a near-tie", s, got[s], ref.greedy_ids[s], err)
        cur = ref.greedy_ids[s]
    t.slab(eng.state.back(0), ref.greedy_state)
    return int(bool(bad))


def run(stressor, prec, quant, log_dir):
    key = (stressor, prec, quant)
    if key in _RUN:
        return _RUN[key]
    ref = T.reference(stressor, quant)
    st = R.st_serialize(T.tensors(stressor, quant))
    log = log_path(log_dir, stressor, prec, quant)
    out = {name: run_recipe(name, ref, st, log, prec, quant, with_greedy=prec != RAW) for name in T.recipes_of(quant)}
    print(f"\n[v4 values] {stressor} {PREC_ID[prec]} {QUANT_ID[quant]}: worst error / tolerance (logits; att shift, aa, bb, pp, ffn shift) " +
          " ".join(f"{n}={t.worst['logits']:.3f};" + ",".join(f"{t.worst[u]:.3f}" for u in T.ROW_KINDS) for n, t in out.items()))
    if os.environ.get("RWKV_V4_SWEEP_JSONL"):
        with open(os.environ["RWKV_V4_SWEEP_JSONL"], "a") as f:
            f.write(json.dumps({"sweep": "values", "stressor": stressor, "precision": PREC_ID[prec], "quant": QUANT_ID[quant],
                                **{f"{n}_{u}": round(t.worst[u], 4) for n, t in out.items() for u in T.UNITS},
                                "greedy_near_ties": sum(t.near_tie for t in out.values())}) + "\n")
    _RUN[key] = out
    return out


def check(out, stressor, prec, quant):
    assert all(t.finite for t in out.values()), {n: t.finite for n, t in out.items()}      # a NaN is reported as a NaN
    over = {(n, u): (round(t.worst[u], 3), T.cap(stressor, quant, prec == FP32, n, u)) for n, t in out.items() for u in T.UNITS
            if not t.worst[u] <= T.cap(stressor, quant, prec == FP32, n, u)}
    assert not over, f"error / tolerance above the unit's bound {{(recipe, unit): (figure, bound)}}: {over}"
    assert sum(t.near_tie for t in out.values()) <= 1


UCASES = [c for c in T.CASES if not c[1]]
QCASES = [c for c in T.CASES if c[1]]


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_ID[p] for p in PRECS])
@pytest.mark.parametrize("stressor,quant", UCASES, ids=[T.case_id(*c) for c in UCASES])
def test_every_recipe_matches_v4_ref_under_the_stressor(stressor, quant, prec, log_dir):
    check(run(stressor, prec, quant, log_dir), stressor, prec, quant)


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_ID[p] for p in PRECS])
@pytest.mark.parametrize("stressor,quant", QCASES, ids=[T.case_id(*c) for c in QCASES])
def test_planted_quantisation_blocks_match_v4_ref_with_the_same_quantisation(stressor, quant, prec, log_dir):
    check(run(stressor, prec, quant, log_dir), stressor, prec, quant)


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_ID[p] for p in PRECS])
def test_decay_ends_blended_in_by_a_lora_file_match_v4_ref_loaded_the_same_way(prec):
    """`decay_ends` edits `time_decay` alone, so the benign checkpoint plus a LoRA file that carries `time_decay` (the stressed one) and
    `time_first` as whole vectors at alpha = 1 (v = 1 * l + 0 * v) IS the stressed model: the load path that blends a vector and then takes
    -exp of the blend on the device (launch_vec_blend, then V4's op 2: blend first, transform after) at decays that do nothing and decays
    that forget everything.  The checker is loaded the same way, through v4_ref.blend_lora."""
    base, stressed = T.base(), T.tensors("decay_ends")
    lora = {k: stressed[k] for k in stressed if k.endswith("att.time_decay") or k.endswith("att.time_first")}
    assert len(lora) == 2 * T.LAYERS and all(np.array_equal(stressed[k], v) for k, v in base.items() if not k.endswith("att.time_decay"))
    ref = v4_ref.V4Ref(v4_ref.blend_lora(base, lora, 1.0))
    eng = rt.ModelBuilder(R.st_serialize(base)).lora(R.st_serialize(lora), 1.0).build(max_batch=T.NSLOT, token_chunk_size=16, precision=prec)
    toks = [T.base_tokens(b)[:T.SHORT] for b in range(T.NSLOT)]
    states = [ref.init_state() for _ in range(T.NSLOT)]
    t = T.Tally(factor(prec))
    for s in range(T.SHORT):
        outs = feed(eng, [rt.RnnInputBatch([toks[b][s]], rt.RnnOption.Last) for b in range(T.NSLOT)])
        for b in range(T.NSLOT):
            t.row(outs[b][-1], ref.forward([toks[b][s]], states[b])[-1])
    for b in range(T.NSLOT):
        t.slab(eng.state.back(b), states[b])
    eng.close()
    same = T.reference("decay_ends")                              # and the blended checker is the stressed one, bit for bit
    assert all(np.array_equal(states[b], same.state[(b, T.SHORT)]) for b in range(T.NSLOT))
    print(f"\n[v4 values] decay_ends through a LoRA file {PREC_ID[prec]}: worst error / tolerance " + " ".join(f"{u}={v:.3f}" for u, v in t.worst.items()))
    check({"decode": t}, "decay_ends", prec, 0)


def test_raw_f16_stays_finite_under_every_stressor_at_once(log_dir):
    """No bound exists for RWKV_PRECISION_FP16_RAW at these values; every output and the whole state slab are finite."""
    out = run(T.ALL, RAW, 0, log_dir)
    assert all(t.finite for t in out.values()), {n: t.finite for n, t in out.items()}


def test_the_recipes_took_the_paths_they_exist_for(log_dir):
    """From the engines' launch logs: the decode WKV-4 kernel, the chunked one at 8 and at 70 rows per sequence, the tile GEMM, both quantised formats."""
    run("decay_ends", FP32, 0, log_dir)
    rows = [json.loads(l) for l in open(log_path(log_dir, "decay_ends", FP32, 0))]
    wkv = [d for d in rows if d["kind"] == "row" and d["kernel"].startswith("wkv4")]
    blocks = T.width(0) // 64
    assert any(d["kernel"] == "wkv4_kernel" and d["T"] == T.NSLOT for d in wkv)
    assert any(d["kernel"] == "wkv4_chunk_kernel" and d["T"] == T.NSLOT * T.CHUNK8_ROWS and d["grid"] == T.NSLOT * blocks for d in wkv)
    assert any(d["kernel"] == "wkv4_chunk_kernel" and d["T"] == T.CHUNK32_ROWS and d["grid"] == blocks for d in wkv)
    assert any(d["kind"] == "tile" and d["T"] == T.TILE_ROWS for d in rows)
    per_weight = {}
    for quant in (1, 2):
        run(T.QUANT_BLOCKS, FP32, quant, log_dir)
        q = [json.loads(l) for l in open(log_path(log_dir, T.QUANT_BLOCKS, FP32, quant))]
        wo = [d for d in q if d.get("mats") == "blocks.0.att.output.weight"]
        assert wo and any(d["kind"] == "tile" for d in wo) and any(d["kind"] != "tile" for d in wo)
        per_weight[quant] = wo[0]["bytes"] / float(T.width(quant) ** 2)
    print(f"\n[v4 values] bytes per weight of the logged output projection: {per_weight}")
    assert 0.9 < per_weight[1] < 1.3 and 0.45 < per_weight[2] < 0.8, per_weight

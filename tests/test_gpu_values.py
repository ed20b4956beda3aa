"""GPU (-m gpu): parity at weight VALUES the synthetic checkpoints never reach (tests/values_table.py): decays at both ends of exp(-exp(d)),
large bonus terms, LayerNorm / GroupNorm weights spread over two decades, embedding outliers and a zero-variance row, all-zero heads (the
GroupNorm of a zero head, V7's kappa floor), relu^2 operands at the top of f16's range and past it (the +-65504 clamp of the operand
split), and quantisation blocks planted for the device quantisers (zero, constant, one outlier, subnormal and zero scales, f16's top, the
NF4 midpoints).  tests/test_values_cpu.py proves on the CPU that every stressor bites on exactly these rows and that the oracle's
restatements agree there.

Recipes (one engine each; 2 layers, 128 wide, quantised 256 wide): decode (3-token prompt, 48 single-token steps, 4 slots), chunk8 (4 slots
x 8 rows, 6 calls), chunk32 (70 rows, Full), tile (250 rows, Last), long (600 tokens by 100, then 16 greedy steps).  The reference is one
lock-step run of RwkvRefBatch per (version, stressor, quantisation); with `ffn_saturating` and the quantised runs it clamps GEMM operands
like the engine does.

Bounds: logits 2e-5 (Fp32) / 1e-3 (Fp16) x max(1, |ref row|_inf); state the same factors PER (layer, head) 64 x 64 block and per token-shift
row against that block's own |ref|_inf (a slab-wide bound would let a quiet head be wrong by a loud head's tolerance); finiteness asserted
on its own.  Every worst error / tolerance is printed (`-s`) and appended to the file RWKV_VALUES_JSONL names, if set."""
import json
import os

import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from tests import values_table as T

pytestmark = pytest.mark.gpu
FP16_TOL, FP32_TOL = 1e-3, 2e-5
PRECS = [rt.Precision.Fp32, rt.Precision.Fp16]
PREC_ID = {rt.Precision.Fp32: "fp32", rt.Precision.Fp16: "fp16", rt.Precision.Fp16Raw: "raw"}
QUANT_ID = {0: "f16", 1: "int8", 2: "nf4"}
RECIPES = ("decode", "chunk8", "chunk32", "tile", "long")
FP16_DERIVED = T.FP16_DERIVED                                  # simulated Fp16 figures of five quantised runs; their bound is 2 x (values_table)
_RUN = {}


def factor(prec):
    return FP32_TOL if prec == rt.Precision.Fp32 else FP16_TOL


@pytest.fixture(scope="module")
def log_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("launch_logs")


def log_path(log_dir, ver, stressor, prec, quant):
    return str(log_dir / f"v{ver}_{stressor}_{PREC_ID[prec]}_{QUANT_ID[quant]}.jsonl")


def build(st, log, B, chunk, prec, quant):
    os.environ["RWKV_LAUNCH_LOG"] = log
    try:
        return rt.ModelBuilder(st).quant(T.LAYERS if quant else 0, rt.Quant(quant)).build(max_batch=B, token_chunk_size=chunk, precision=prec)
    finally:
        os.environ.pop("RWKV_LAUNCH_LOG", None)


class Tally:
    """Worst error / tolerance of one recipe, and whether anything was not finite."""

    def __init__(self, prec):
        self.f, self.logits, self.state, self.finite = factor(prec), 0.0, 0.0, True

    def row(self, got, want):
        self.finite &= bool(np.isfinite(got).all())
        self.logits = max(self.logits, float(np.abs(got - want).max()) / (self.f * max(1.0, float(np.abs(want).max()))))

    def slab(self, got, want):
        self.finite &= bool(np.isfinite(got).all())
        for (_, g), (_, w) in zip(T.state_blocks(got), T.state_blocks(want)):
            self.state = max(self.state, float(np.abs(g - w).max()) / (self.f * max(1.0, float(np.abs(w).max()))))


def feed(eng, batches):
    _, outs = eng.infer(rt.RnnInput(batches))
    return outs


def run_recipe(name, ref, st, log, prec, quant, tally_only_finite=False):
    t = Tally(prec)
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
        if not tally_only_finite:
            t.near_tie = greedy(eng, ref, t)
    eng.close()
    return t


def greedy(eng, ref, t):
    """16 greedy steps through decode_greedy against the oracle's ids; the first differing id must be a near-tie of the REFERENCE (its own gap
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


def run(ver, stressor, prec, quant, log_dir, recipes=RECIPES):
    key = (ver, stressor, prec, quant)
    if key in _RUN:
        return _RUN[key]
    from oracle import rwkv_ref as R
    ref = T.reference(ver, stressor, quant)
    st = R.st_serialize(ref.tens)
    log = log_path(log_dir, ver, stressor, prec, quant)
    out = {name: run_recipe(name, ref, st, log, prec, quant, tally_only_finite=prec == rt.Precision.Fp16Raw) for name in recipes}
    line = {"version": ver, "stressor": stressor, "precision": PREC_ID[prec], "quant": QUANT_ID[quant],
            **{f"{n}_logits": round(t.logits, 4) for n, t in out.items()}, **{f"{n}_state": round(t.state, 4) for n, t in out.items()}}
    print(f"\n[values] v{ver} {stressor} {PREC_ID[prec]} {QUANT_ID[quant]}: worst error / tolerance " +
          " ".join(f"{n}={t.logits:.3f}/{t.state:.3f}" for n, t in out.items()) + " (logits/state)")
    if os.environ.get("RWKV_VALUES_JSONL"):
        with open(os.environ["RWKV_VALUES_JSONL"], "a") as f:
            f.write(json.dumps(line) + "\n")
    _RUN[key] = out
    return out


def check(out, derived=None):
    assert all(t.finite for t in out.values()), {n: t.finite for n, t in out.items()}      # a NaN is reported as a NaN
    cap = lambda n, what: max(1.0, 2.0 * (derived or {}).get((n, what), 0.0))
    over = {n: (t.logits, t.state) for n, t in out.items() if not (t.logits <= cap(n, "logits") and t.state <= cap(n, "state"))}
    assert not over, f"error / tolerance above 1 (logits, state per block): {over}"


CASES = [(v, s) for v in T.VERSIONS for s in T.STRESSORS + (T.ALL,)]


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_ID[p] for p in PRECS])
@pytest.mark.parametrize("ver,stressor", CASES, ids=[f"v{v}-{s}" for v, s in CASES])
def test_every_recipe_matches_the_oracle_under_the_stressor(ver, stressor, prec, log_dir):
    check(run(ver, stressor, prec, 0, log_dir))


QCASES = [(v, s) for v in T.VERSIONS for s in (T.QUANT_BLOCKS, T.ALL)]


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_ID[p] for p in PRECS])
@pytest.mark.parametrize("quant", [1, 2], ids=["int8", "nf4"])
@pytest.mark.parametrize("ver,stressor", QCASES, ids=[f"v{v}-{s}" for v, s in QCASES])
def test_planted_quantisation_blocks_match_the_oracle_with_the_same_quantisation(ver, stressor, quant, prec, log_dir):
    check(run(ver, stressor, prec, quant, log_dir, recipes=("decode", "tile")),
          FP16_DERIVED.get((ver, stressor, quant)) if prec == rt.Precision.Fp16 else None)


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_ID[p] for p in PRECS])
def test_decay_ends_blended_in_by_a_lora_file_match_the_oracle(prec, log_dir):
    """V5's `decay_ends` edits `time_decay` alone, so the benign checkpoint plus a LoRA file that holds those vectors at alpha = 1
    (v = 1 * l + 0 * v) IS the stressed model: the load path that blends a vector and then takes exp(-exp(d)) of the blend on the device
    (`vec_op`, not the plain conversion every other run goes through) at d where w is exactly 1 and exactly 0."""
    from oracle import rwkv_ref as R
    ref = T.reference(5, "decay_ends")
    lora = {k: v for k, v in ref.tens.items() if k.endswith("att.time_decay")}
    assert len(lora) == T.LAYERS and all(np.array_equal(ref.tens[k], v) for k, v in T.base(5).items() if k not in lora)
    eng = rt.ModelBuilder(R.st_serialize(T.base(5))).lora(R.st_serialize(lora), 1.0).build(max_batch=T.NSLOT, token_chunk_size=16, precision=prec)
    t = Tally(prec)
    for s in range(T.SHORT):
        outs = feed(eng, [rt.RnnInputBatch([ref.base[b][s]], rt.RnnOption.Last) for b in range(T.NSLOT)])
        for b in range(T.NSLOT):
            t.row(outs[b][-1], ref.logits[b][s])
    for b in range(T.NSLOT):
        t.slab(eng.state.back(b), ref.state[(b, T.SHORT)])
    eng.close()
    print(f"\n[values] v5 decay_ends through a LoRA file {PREC_ID[prec]}: worst error / tolerance {t.logits:.3f}/{t.state:.3f} (logits/state)")
    check({"decode": t})


@pytest.mark.parametrize("ver", T.VERSIONS)
def test_raw_f16_stays_finite_under_every_stressor_at_once(ver, log_dir):
    """No bound exists for RWKV_PRECISION_FP16_RAW at these values; every output and the whole state slab are finite."""
    out = run(ver, T.ALL, rt.Precision.Fp16Raw, 0, log_dir)
    assert all(t.finite for t in out.values()), {n: t.finite for n, t in out.items()}


def test_the_recipes_took_the_paths_they_exist_for(log_dir):
    """From the engines' launch logs: the decode WKV, both chunked forms (<= 8 rows per sequence; more), the tile GEMM, both quantised formats."""
    run(6, "decay_ends", rt.Precision.Fp32, 0, log_dir)
    rows = [json.loads(l) for l in open(log_path(log_dir, 6, "decay_ends", rt.Precision.Fp32, 0))]
    H = T.width(0) // 64
    wkv = [d for d in rows if d["kind"] == "row" and d["kernel"].startswith("wkv")]
    assert any(d["kernel"] == "wkv_kernel" and d["T"] == T.NSLOT for d in wkv)
    assert any(d["kernel"] == "wkv_chunk_kernel" and d["T"] == T.NSLOT * T.CHUNK8_ROWS and d["grid"] == T.NSLOT * H for d in wkv)
    assert any(d["kernel"] == "wkv_chunk_kernel" and d["T"] == T.CHUNK32_ROWS and d["grid"] == H for d in wkv)
    assert any(d["kind"] == "tile" and d["T"] == T.TILE_ROWS for d in rows)
    per_weight = {}
    for quant in (1, 2):
        run(6, T.QUANT_BLOCKS, rt.Precision.Fp32, quant, log_dir, recipes=("decode", "tile"))
        q = [json.loads(l) for l in open(log_path(log_dir, 6, T.QUANT_BLOCKS, rt.Precision.Fp32, quant))]
        wo = [d for d in q if d.get("mats") == "blocks.0.att.output.weight"]
        assert wo and any(d["kind"] == "tile" for d in wo) and any(d["kind"] != "tile" for d in wo)
        per_weight[quant] = wo[0]["bytes"] / float(T.width(quant) ** 2)
    print(f"\n[values] bytes per weight of the logged output projection: {per_weight}")
    assert 0.9 < per_weight[1] < 1.3 and 0.45 < per_weight[2] < 0.8, per_weight

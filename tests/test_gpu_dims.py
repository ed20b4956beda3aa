"""GPU (-m gpu): parity at model dimensions the loader accepts and no other test uses (tests/dims_table.py): widths that are no multiple
of 128 (K % 128 != 0: the chunked tile kernel, the TAIL decode kernel with a K split), one head, LoRA ranks between and beyond the
published ones, tiny and odd vocabularies — at single steps of exactly 1, 3, 16, 17, 32, 33, 64, 65, 192, 193 and 250 rows, one engine per
step size (max_batch and token_chunk_size are the step's own, so every buffer is as tight as it gets), in Precision.Fp32 and Fp16.

The reference of a row is ONE lock-step run of the numpy oracle (RwkvRefBatch, an RwkvRef: tests/test_oracle.py pins it to the per-token
form, tests/test_dims_cpu.py to the compiled restatement at these very dims) over twelve base sequences; slot b of every step feeds a prefix
of base sequence b.  Tolerances are the project's: 1e-3 (Fp16) and 2e-5 (Fp32) times max(1, |ref|_inf).

The engines are built with RWKV_LAUNCH_LOG, one file per (row, precision, quantisation); the last test reads them and proves that the
sweep took the paths it exists for.  Every figure is printed (`-s`): worst error / tolerance per row and precision."""
import json
import os

import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import dims_table as D

pytestmark = pytest.mark.gpu
FP16_TOL, FP32_TOL = 1e-3, 2e-5
PRECS = [rt.Precision.Fp32, rt.Precision.Fp16]
PREC_ID = {rt.Precision.Fp32: "fp32", rt.Precision.Fp16: "fp16"}
QUANT_ID = {0: "f16", 1: "int8", 2: "nf4"}


def tol(prec, want):
    return (FP32_TOL if prec == rt.Precision.Fp32 else FP16_TOL) * max(1.0, float(np.abs(want).max()))


class Reference:
    """logits[b][t] and the state after n tokens of base sequence b, for the prefixes the recipes read; computed once per (row, quantisation)."""

    def __init__(self, i, quant):
        self.tens = D.tensors(i)
        self.st = R.st_serialize(self.tens)
        self.rb = rb = R.RwkvRefBatch(self.tens, D.LAYERS if quant else 0, quant)
        self.base = [D.base_tokens(i, b) for b in range(D.NSLOT)]
        need = D.needed_prefixes()
        states = rb.init_states(D.NSLOT)
        self.logits = [np.zeros((len(p), rb.info.num_vocab), np.float32) for p in self.base]
        self.state = {}
        for t in range(max(len(p) for p in self.base)):
            act = [b for b in range(D.NSLOT) if t < len(self.base[b])]
            sub = np.ascontiguousarray(states[act])
            lg = rb.step([self.base[b][t] for b in act], sub)
            states[act] = sub
            for j, b in enumerate(act):
                self.logits[b][t] = lg[j]
                if (b, t + 1) in need:
                    self.state[(b, t + 1)] = sub[j].copy()


_REF, _SWEEP = {}, {}


def reference(i, quant):
    if (i, quant) not in _REF:
        _REF[(i, quant)] = Reference(i, quant)
    return _REF[(i, quant)]


@pytest.fixture(scope="module")
def log_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("launch_logs")


def log_path(log_dir, i, prec, quant):
    return str(log_dir / f"{i}_{PREC_ID[prec]}_{QUANT_ID[quant]}.jsonl")


def build(st, log, B, chunk, prec, quant=0):
    """An engine whose GEMM launches of layers 0 / 1 and the head are appended to `log` (the variable is read at engine creation)."""
    os.environ["RWKV_LAUNCH_LOG"] = log
    try:
        return rt.ModelBuilder(st).quant(D.LAYERS if quant else 0, rt.Quant(quant)).build(max_batch=B, token_chunk_size=chunk, precision=prec)
    finally:
        os.environ.pop("RWKV_LAUNCH_LOG", None)


def greedy_check(eng, rb, first, ref_states, prec):
    """decode_greedy for GREEDY_STEPS steps against the oracle's greedy ids; a slot's first differing id must be a near-tie of the reference (its
    own gap at most twice the measured error of that row: the rule of tests/test_gpu_knobs.py), measured by replaying the reference's ids
    through `infer` from a snapshot.  Returns (slots that diverged on a near-tie, worst error / tolerance of the replayed rows)."""
    B, n = len(first), D.GREEDY_STEPS
    snaps = [eng.state.read(b) for b in range(B)]
    got, _ = eng.decode_greedy(first, n)
    st = np.ascontiguousarray(ref_states)
    want, lgs, cur = np.zeros((n, B), np.int64), [], list(first)
    for s in range(n):
        lg = rb.step(cur, st)
        cur = [int(x) for x in np.argmax(lg, axis=1)]
        lgs.append(lg)
        want[s] = cur
    split = {}
    for b in range(B):
        bad = np.nonzero(got[:, b].astype(np.int64) != want[:, b])[0]
        if bad.size:
            split[b] = int(bad[0])
    worst = 0.0
    if split:
        for b in range(B):
            eng.state.write(snaps[b], b)
        cur = list(first)
        for s in range(max(split.values()) + 1):
            _, outs = eng.infer(rt.RnnInput([rt.RnnInputBatch([cur[b]], rt.RnnOption.Last) for b in range(B)]))
            for b in range(B):
                err = float(np.abs(outs[b][-1] - lgs[s][b]).max())
                worst = max(worst, err / tol(prec, lgs[s][b]))
                if split.get(b) == s:
                    gi, wi = int(got[s, b]), int(want[s, b])
                    assert float(lgs[s][b][wi] - lgs[s][b][gi]) <= 2.0 * err, ("greedy ids differ beyond a near-tie", b, s, gi, wi, err)
            cur = [int(x) for x in want[s]]
    return len(split), worst


def run_sweep(i, prec, quant, log_dir):
    """Every step size, the Full request and the greedy run of one (row, precision, quantisation); returns {case: worst error / tolerance} and
    the structural failures (a step of the wrong size).  Memoised: the path proof reads the logs these runs leave."""
    key = (i, prec, quant)
    if key in _SWEEP:
        return _SWEEP[key]
    ref = reference(i, quant)
    log = log_path(log_dir, i, prec, quant)
    ratios, wrong = {}, []
    for N in D.STEP_SIZES:
        lens = D.step_lengths(N)
        B = len(lens)
        eng = build(ref.st, log, B, N, prec, quant)
        inp = rt.RnnInput([rt.RnnInputBatch(list(ref.base[b][:lens[b]]), rt.RnnOption.Last) for b in range(B)])
        before = inp.num_token()
        plan = rt.plan_chunk(lens, eng.token_chunk_size)
        inp, outs = eng.infer(inp)
        if not (eng.token_chunk_size == N and plan == lens and before - inp.num_token() == sum(plan) == N):
            wrong.append((N, eng.token_chunk_size, plan, before, inp.num_token()))
        worst = 0.0
        for b in range(B):
            want, ws = ref.logits[b][lens[b] - 1], ref.state[(b, lens[b])]
            assert len(outs[b]) == 1, (N, b, len(outs[b]))
            worst = max(worst, float(np.abs(outs[b][-1] - want).max()) / tol(prec, want),
                        float(np.abs(eng.state.back(b) - ws).max()) / tol(prec, ws))
        ratios[f"step{N}"] = worst
        if N == 3:                                                # the greedy run goes on from this step's three slots
            first = [int(np.argmax(ref.logits[b][lens[b] - 1])) for b in range(B)]
            ntie, gw = greedy_check(eng, ref.rb, first, np.stack([ref.state[(b, lens[b])] for b in range(B)]), prec)
            ratios["greedy_replay"] = gw
            ratios["greedy_near_ties"] = float(ntie)
        eng.close()
    eng = build(ref.st, log, 1, D.FULL_ROWS, prec, quant)          # one Full request: every row of the step is an output row
    inp = rt.RnnInput([rt.RnnInputBatch(list(ref.base[0][:D.FULL_ROWS]), rt.RnnOption.Full)])
    inp, outs = eng.infer(inp)
    if inp.num_token() != 0 or len(outs[0]) != D.FULL_ROWS:
        wrong.append(("full", inp.num_token(), len(outs[0])))
    else:
        ratios["full65"] = max(float(np.abs(outs[0][t] - ref.logits[0][t]).max()) / tol(prec, ref.logits[0][t]) for t in range(D.FULL_ROWS))
    eng.close()
    print(f"\n[dims] {D.row_id(i)} {PREC_ID[prec]} {QUANT_ID[quant]}: worst error / tolerance " +
          " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    _SWEEP[key] = (ratios, wrong)
    return _SWEEP[key]


def check_sweep(i, prec, quant, log_dir):
    ratios, wrong = run_sweep(i, prec, quant, log_dir)
    assert not wrong, f"steps of the wrong size (N, chunk, plan, tokens before, after): {wrong}"
    over = {k: v for k, v in ratios.items() if k != "greedy_near_ties" and not v <= 1.0}
    assert not over, f"{D.row_id(i)} {PREC_ID[prec]} {QUANT_ID[quant]}: error / tolerance above 1: {over} (all: {ratios})"
    assert ratios["greedy_near_ties"] <= 1, ratios                  # near-ties are rare: three slots, 24 steps


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_ID[p] for p in PRECS])
@pytest.mark.parametrize("i", D.RUN, ids=[D.row_id(i) for i in D.RUN])
def test_every_step_size_full_request_and_greedy_match_the_oracle(i, prec, log_dir):
    check_sweep(i, prec, 0, log_dir)


QROWS = [i for i in D.RUN if D.quantisable(D.TABLE[i])]


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_ID[p] for p in PRECS])
@pytest.mark.parametrize("quant", [1, 2], ids=["int8", "nf4"])
@pytest.mark.parametrize("i", QROWS, ids=[D.row_id(i) for i in QROWS])
def test_quantisable_rows_match_the_oracle_with_the_same_quantisation(i, quant, prec, log_dir):
    check_sweep(i, prec, quant, log_dir)


@pytest.mark.parametrize("i", [i for i in D.RUN if i not in QROWS], ids=[D.row_id(i) for i in D.RUN if i not in QROWS])
def test_rows_that_cannot_be_quantised_are_refused_before_any_kernel_runs(i, log_dir):
    st = reference(i, 0).st
    log = str(log_dir / f"refused_quant_{i}.jsonl")
    for quant in (1, 2):
        with pytest.raises(rt.RwkvError) as e:
            build(st, log, 2, 16, rt.Precision.Fp16, quant)
        assert e.value.code == -3 and "multiples of 256" in str(e.value)
    assert not os.path.exists(log) or os.path.getsize(log) == 0     # refused at build time: the engine launched nothing


@pytest.mark.parametrize("i", D.REFUSED, ids=[D.row_id(i) for i in D.REFUSED])
def test_rows_outside_the_kernels_reach_are_refused_by_name(i):
    """V6 decay LoRA ranks that are no multiple of 32: the WKV kernels read the rank in four parts of whole 8-element vectors."""
    st = R.st_serialize(D.tensors(i))
    with pytest.raises(rt.RwkvError) as e:
        rt.ModelBuilder(st).build(max_batch=2, token_chunk_size=16)
    assert e.value.code == -3 and D.TABLE[i].refuse in str(e.value) and str(D.TABLE[i].lora[1]) in str(e.value), str(e.value)


@pytest.mark.parametrize("i", D.SAMPLER_ROWS, ids=[D.row_id(i) for i in D.SAMPLER_ROWS])
def test_on_device_sampling_at_small_vocabularies(i, log_dir):
    """infer_sample at V = 16 and V = 272 (nucleus with top_k > V, top_k = V and top_k = 1, typical, mirostat) against the restatements of
    the reference's samplers on the SAME logits (the state is snapshotted, `infer` gives the logits, the snapshot is restored, the device
    samples), with the margin rules of tests/test_gpu_parity.py; at most 1 draw in 8 may be too close to a boundary to compare."""
    from ai00_server_amd.harness import MirostatSampler, NucleusSampler, TypicalSampler
    ref = reference(i, 0)
    cfgs = D.sampler_configs(D.TABLE[i].V)
    B = len(cfgs)
    make = {"nucleus": lambda c: NucleusSampler(presence_penalty=0.0, frequency_penalty=0.0, **c),
            "typical": lambda c: TypicalSampler(presence_penalty=0.0, frequency_penalty=0.0, **c), "mirostat": lambda c: MirostatSampler(**c)}
    dev = [make[k](c) for k, c in cfgs]
    ms = [np.float32(2.0 * c["tau"]) if k == "mirostat" else None for k, c in cfgs]
    eng = build(ref.st, log_path(log_dir, i, rt.Precision.Fp16, 0), B, 16, rt.Precision.Fp16)
    us = D.sampler_uniforms(i)
    checked = skipped = 0
    for s, toks in enumerate(D.sampler_tokens(i)):
        snaps = [eng.state.read(b) for b in range(B)]
        _, outs = eng.infer(rt.RnnInput([rt.RnnInputBatch([toks[b]], rt.RnnOption.Last) for b in range(B)]))
        for b in range(B):
            eng.state.write(snaps[b], b)
        _, got = eng.infer_sample(rt.RnnInput([rt.RnnInputBatch([toks[b]], rt.RnnOption.Last) for b in range(B)]), dev, [float(u) for u in us[s]])
        for b, (kind, cfg) in enumerate(cfgs):
            want, margin, surprise = D.sampler_want(kind, cfg, outs[b][-1], float(us[s, b]), None if ms[b] is None else float(ms[b]))
            if kind == "mirostat":
                assert abs(float(dev[b].max_surprise) - float(ms[b])) < 1e-3
            if margin > D.SAMPLER_MARGIN[kind]:
                assert got[b][0] in want, (s, b, kind, got[b], want, margin)
                if kind == "mirostat":
                    assert abs(got[b][1] - surprise) < 1e-3 * max(1.0, abs(surprise))
                else:
                    assert 0.0 < got[b][1] <= 1.0
                checked += 1
            else:
                skipped += 1
            if kind == "mirostat":                                  # both state machines follow the reference's surprise
                ms[b] = D.mirostat_update(ms[b], surprise, cfg)
                dev[b].update(surprise)
    eng.close()
    print(f"\n[dims] sampling {D.row_id(i)}: {checked} draws compared, {skipped} within the margin")
    assert skipped * 8 <= checked + skipped, (checked, skipped)


def test_the_sweep_took_the_paths_it_exists_for(log_dir):
    """From the engines' own launch logs (the runs above, or run here when this test is selected alone): the chunked tile kernel at
    K % 128 != 0 with hi + lo and with plain operands, the TAIL decode kernel with a K split, the small-K kernel on V7's second LoRA stage
    up to K = 320, never on the 352-wide matrix and never on a step of more than 64 rows.  Prints the distinct (kind, variant, ksplit) per row."""
    def lines(i, prec, quant=0):
        run_sweep(i, prec, quant, log_dir)
        return [d for d in map(json.loads, open(log_path(log_dir, i, prec, quant))) if d["kind"] != "row"]

    def K_of(i, name):                                              # inner dimension of a logged matrix
        r, n = D.TABLE[i], name.split(".", 2)[-1] if name.startswith("blocks.") else name
        if n == "ffn.value.weight":
            return r.F
        if r.ver == 7 and n[:4] == "att." and n[4:] in ("w2", "a2", "v2", "g2"):
            return dict(zip("wavg", r.lora))[n[4]]
        if r.ver == 6 and n.startswith("att.time_mix_w2"):
            return r.lora[0]
        return r.C

    seen = {}
    for i in D.RUN:
        for prec in PRECS:
            for d in lines(i, prec):
                seen.setdefault((D.row_id(i), PREC_ID[prec]), set()).add((d["kind"], d["variant"], d["ksplit"]))
    for k in sorted(seen):
        print(f"\n[dims] paths {k[0]} {k[1]}: {sorted(seen[k])}")
    odd = [i for i in D.RUN if D.TABLE[i].C % 128]
    for prec in PRECS:
        hit = [(D.row_id(i), d["mats"], d["variant"]) for i in odd for d in lines(i, prec)
               if d["kind"] == "tile" and d["variant"] < 10 and any(K_of(i, m) % 128 for m in d["mats"].split("+"))]
        assert hit, f"no chunked tile launch at K % 128 != 0 in {PREC_ID[prec]}"
    # decode with a K split whose per-block range is no whole number of 256-k slices (TAIL): Kb = K / ksplit
    tail = [(D.row_id(i), d["T"], d["mats"], d["ksplit"]) for i in D.RUN for prec in PRECS for d in lines(i, prec)
            if d["kind"] == "decode" and d["ksplit"] > 1 and (K_of(i, d["mats"].split("+")[0]) // d["ksplit"]) % 256]
    assert tail, "no TAIL decode launch with a K split"
    for i in [i for i in D.RUN if D.TABLE[i].ver == 7]:
        sk = [d for prec in PRECS for d in lines(i, prec) if d["kind"] == "smallk"]
        wide = max(D.TABLE[i].lora) > D.SK_KMAX
        if wide:
            assert not [d for d in sk if "att.g2" in d["mats"]], "the 352-wide matrix rode a small-K launch"
            declined = [d for prec in PRECS for d in lines(i, prec) if "att.g2" in d["mats"] and d["T"] <= 64]
            assert declined and all(d["kind"] == "decode" for d in declined)
        else:
            assert any("att.w2" in d["mats"] and "att.g2" in d["mats"] for d in sk), D.row_id(i)
        # (at these widths other launches are short in K too — the head and V5 / V6's projections at C <= 320 — and ride the same kernel)
        assert all(d["T"] <= 64 and all(K_of(i, m) <= D.SK_KMAX for m in d["mats"].split("+")) for d in sk), D.row_id(i)

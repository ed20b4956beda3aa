"""CPU: the resident-generation probe's table, references and checker (tests/gen_cases.py), proved without a GPU — in the manner of
tests/test_sample_cases_cpu.py.

  * coverage from the table alone, and a gap when any group is removed;
  * the references agree with the project's independent host mirrors: the draw with rwkv_gen_uniform, the penalty / bias / Mirostat arithmetic
    with the per-token samplers of harness.py over 40 tokens per kind, the DFA and PDA walks with rwkv_dfa_allow / rwkv_dfa_walk /
    rwkv_pda_allow, the PDA commit (state, stack, halt) with harness.PdaFormatter over rwkv_pda_walk;
  * the inputs are chosen so that the arithmetic mistakes change bits: both wrong associations of x + np + b in at least 100 entries of every
    gen_pre case with V >= 1024, a fused p * decay + freq at the drawn token of every gen_post row that has an entry there;
  * the checks can fail: every one-line mistake of MISTAKES, applied to the reference as a kernel would make it, is reported by check_case;
  * the case file's round trip, and the probe compiles for gfx950."""
import os

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from tests import gen_cases as G
from tests import probe_io as P

F32, F64, U32 = np.float32, np.float64, np.uint32


@pytest.fixture(scope="module")
def cases(built_lib):
    return G.all_cases()


def test_the_table_covers_what_it_must(cases):
    assert G.coverage_gaps(cases) == []
    for g in G.GROUPS:
        assert G.coverage_gaps([c for c in cases if c.group != g]), f"removing group {g} leaves no gap: the coverage does not see it"
    kinds = lambda *ks: [c for c in cases if G.KIND_NAME[c.kind] in ks]
    for k in ("gen_pre", "gen_post", "gen_inject"):
        assert {c.p["V"] for c in kinds(k)} >= {16, 1024, 16384, 16400, 65536}
    for k in ("gen_mask", "gen_pda_mask"):
        assert {c.p["V"] for c in kinds(k)} == {16, 272, 65536}
    for k in ("gen_freeze", "gen_capture"):
        assert {c.p["nsx"] for c in kinds(k)} == {64, 65600} and {c.p["nw"] for c in kinds(k)} == {64, 131136}
    assert {c.p["max_batch"] for c in kinds("gen_publish")} == {1, 3, 257}
    assert {c.p["T"] for c in kinds("gen_tokens")} == {0, 1, 256, 257, 300} and {c.p["T"] for c in kinds("gen_handover")} == {1, 256, 257, 300}
    assert all(c.p["max_batch"] <= 5 for c in cases if c.p["V"] == 65536)
    at = {}
    for c in kinds("gen_post"):
        at.setdefault(c.p["V"], set()).update(c.o["tags"].get("at", ()))
    for V in G.VOCABS:                                             # each lane of a float4, both sides of a block and of a pass, V - 1: in live rows
        assert at[V] == {t for t in (0, 1, 2, 3, 1023, 1024, 16383, 16384, V - 1) if t < V}, V
    live = lambda c: [s for s in G.row_slots(c.o["world"](), c.p)]
    five = [c for c in kinds("gen_pre", "gen_post") if c.p["max_batch"] == 5]
    assert five and all(c.o["world"]()["slots"][live(c)[1]]["finish"] != 0 and live(c) != sorted(live(c)) for c in five)   # a rider between two live rows


def test_the_wide_worlds_are_what_the_table_says(cases):
    """72 slots: 33 logits rows over a scattered slot list with 63, 64 and 71 and two finished riders; mixed, 70 step rows, 34 output rows and
    one slot in mid-prefill.  One such case of each geometry per launcher, and rows past one block of gen_tokens / gen_handover."""
    B = G.WIDE_B
    rs, orows, riders = G.geom(B, 0)
    assert orows is None and len(rs) == len(set(rs)) == 33 and {63, 64, 71} <= set(rs) and rs != sorted(rs) and max(rs) < B
    assert len(riders) == 2 and set(riders) < set(rs) and sum(s >= 64 for s in rs) >= 3 and min(rs) < 32
    ms, mo, mr = G.geom(B, 1)
    out_slots = [ms[r] for r in mo]
    assert len(ms) == 70 and len(mo) == len(set(out_slots)) == 34 and mo == sorted(mo) and {63, 64, 71} <= set(out_slots) and mr == riders
    assert set(ms) - set(out_slots) == {40} and ms.count(40) == 17                            # in mid-prefill: step rows, no logits row
    assert ms.count(10) == 20 and ms[mo[out_slots.index(10)]] == 10 and ms[mo[out_slots.index(10)] + 1] != 10   # a prompt that ends: its last row is sampled
    assert all(ms.count(s) == 1 for s in out_slots if s != 10) and any(b - a > 1 for a, b in zip(mo, mo[1:]))
    wide = [c for c in cases if c.p["max_batch"] == B]
    assert sorted((G.KIND_NAME[c.kind], c.p["mixed"]) for c in wide) == sorted([(k, m) for k in ("gen_pre", "gen_post", "gen_mask", "gen_freeze", "gen_capture") for m in (0, 1)]
                                                                              + [("step", 0)])
    for c in wide:
        W, p = c.o["world"](), c.p
        assert (p["n_rows"], p["T"]) == ((34, 70) if p["mixed"] else (33, 33)) and G.row_slots(W, p) == (out_slots if p["mixed"] else rs), c.name
        if G.KIND_NAME[c.kind] in ("gen_pre", "gen_post", "gen_mask", "gen_capture", "step"):
            assert sorted(s for s in range(B) if W["slots"][s]["finish"]) == sorted(riders), c.name
    assert any(c.p["T"] == 300 for c in cases if c.group == "tokens") and -(-300 // 256) == 2


def test_the_draw_is_rwkv_gen_uniform(built_lib):
    rng = np.random.default_rng(5)
    triples = [(0, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (1 << 63, 0, 2 ** 32 - 1), (0x9E3779B97F4A7C15, 2 ** 32 - 1, 0)]
    triples += [(int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(2)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))) for _ in range(3000)]
    triples += [(int(rng.integers(0, 1 << 63, dtype=np.uint64)) | 1 << 63, 2 ** 32 - 1 - i, 2 ** 32 - 1 - 7 * i) for i in range(100)]
    for seed, stream, step in triples:
        assert G.uniform(seed, stream, step) == F32(rt.gen_uniform(seed, stream, step)), (seed, stream, step)
    assert any(s >> 63 for s, _, _ in triples)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_the_arithmetic_is_the_per_token_samplers_over_40_tokens(kind):
    rng = np.random.default_rng(kind)
    V = 64
    bias = {int(t): float(F32(rng.standard_normal())) for t in rng.choice(V, 20, replace=False)}
    s = H.MirostatSampler(tau=3.0, rate=0.3) if kind == 2 else (H.TypicalSampler if kind else H.NucleusSampler)(presence_penalty=0.3, frequency_penalty=0.3, bias=bias)
    pen = np.full(V, G.ABSENT, U32)
    b = np.zeros(V, F32)
    for t, v in bias.items():
        b[t] = v
    tau = F32(s.max_surprise) if kind == 2 else None
    for step in range(40):
        x = (rng.standard_normal(V) * 3).astype(F32)
        if kind == 2:
            surprise = F32(rng.uniform(0.0, 12.0))
            s.update(float(surprise))
            tau = G.mirostat(tau, surprise, s.target, s.rate)
            assert tau == s.max_surprise
            continue
        want = x.copy()
        for t, a in s.adjustments().items():
            want[t] = F32(x[t] + a)
        assert (G.adjust(x, pen, b).view(U32) == want.view(U32)).all()
        tok = int(rng.integers(0, 8))                                # a small range: tokens repeat, entries take + frequency
        s.update(tok)
        pen = G.decay_row(pen, tok, s.ad, s.af, s.ap)
        assert {t: F32(v) for t, v in s.penalties.items()} == {int(t): pen.view(F32)[t] for t in np.nonzero(pen != G.ABSENT)[0]}


def table_of(W, p):
    return [G.token_word(W, p, v) for v in range(p["n_tok"])]


def test_the_dfa_walk_is_rwkv_dfa_allow(cases):
    seen = 0
    for c in cases:
        if G.KIND_NAME[c.kind] != "gen_mask" or c.p["V"] > 272:
            continue
        W, p = c.o["world"](), c.p
        trans = W["dfa_trans"].reshape(-1, 256)
        dfa = rt.Dfa.from_table(trans, W["dfa_flags"] & 1)
        for q in range(1, p["dfa_states"]):
            e = G.dfa_ends(trans, q, W["tok_off"], W["tok_bytes"], p["n_tok"], p["V"])
            assert ((e != 0) == (dfa.allow(q, table_of(W, p), p["V"]) != 0)).all()
            for v in np.nonzero(e)[0][:20]:
                assert dfa.walk(q, G.token_word(W, p, int(v))) == e[v]
            seen += 1
    assert seen >= 20


def test_the_pda_walk_is_rwkv_pda_allow(cases):
    seen = 0
    for c in cases:
        if G.KIND_NAME[c.kind] != "gen_pda_mask" or c.p["V"] > 272:
            continue
        W, p = c.o["world"](), c.p
        before = W["logits"].copy()
        G.ref_pda_mask(W, p)
        for row in range(p["n_rows"]):
            d = W["pda"][G.slot_of(W, p, row)]
            if d["next"] == -1 or W["slots"][G.slot_of(W, p, row)]["finish"]:
                assert (W["logits"][row].view(U32) == before[row].view(U32)).all()
                continue
            nxt, act, flags = W["pda_next"].reshape(-1, 256), W["pda_act"].reshape(-1, 256), W["pda_flags"]
            pda = rt.Pda.from_table(nxt, act, flags & 1, max_depth=int(d["max_depth"]))
            allow = pda.allow(int(d["state"]), [int(x) for x in d["stack"][:d["depth"]]], table_of(W, p), p["V"]) != 0
            masked = (W["logits"][row] == -np.inf) & (before[row] != -np.inf)
            keep = before[row] != -np.inf
            assert (masked[keep] == ~allow[keep]).all(), c.name
            assert allow.any() and not allow.all()
            seen += 1
    assert seen >= 8


def test_the_pda_commit_is_the_per_token_formatter(cases):
    """pda_update — the entries a token owns, the state and depth behind it, the halt — against harness.PdaFormatter (rwkv_pda_allow and
    rwkv_pda_walk behind it), for EVERY token of the table from every configuration of the small gen_pda_mask cases, both halt modes."""
    seen = allowed = halted = 0
    for c in cases:
        if G.KIND_NAME[c.kind] != "gen_pda_mask" or c.p["V"] > 272:
            continue
        W0, p = c.o["world"](), c.p
        nxt, act, flags = W0["pda_next"].reshape(-1, 256), W0["pda_act"].reshape(-1, 256), W0["pda_flags"]
        table = table_of(W0, p) + [None] * (p["V"] - p["n_tok"])
        for row in range(p["n_rows"]):
            slot = G.slot_of(W0, p, row)
            d0 = W0["pda"][slot]
            if d0["next"] == -1:
                continue
            pda = rt.Pda.from_table(nxt, act, flags & 1, max_depth=int(d0["max_depth"]))
            stack0 = [int(x) for x in d0["stack"][:d0["depth"]]]
            for mode in (0, 1):
                for tok in range(-1, p["V"] + 1):
                    W = {"pda": W0["pda"].copy(), "tok_off": W0["tok_off"], "tok_bytes": W0["tok_bytes"], "pda_next": W0["pda_next"], "pda_act": W0["pda_act"],
                         "pda_flags": flags}
                    W["pda"][slot]["mode"] = mode
                    f = H.PdaFormatter(pda, table, p["V"], int(d0["state"]), stack0, halt=mode)
                    want_halt = f.update(tok)
                    got_halt = G.pda_update(W, p, slot, tok)
                    d = W["pda"][slot]
                    assert (got_halt, int(d["state"]), [int(x) for x in d["stack"][:d["depth"]]]) == (want_halt, f.state, f.stack), (c.name, row, tok)
                    assert (d["stack"][d["depth"]:] == d0["stack"][d["depth"]:]).all() or d["depth"] < d0["depth"]   # above the new depth: old bits
                    seen += 1
                    allowed += (f.state, f.stack) != (int(d0["state"]), stack0)
                    halted += want_halt
    assert seen >= 4000 and allowed >= 200 and halted >= 1


def test_the_inputs_make_the_arithmetic_mistakes_visible(cases):
    rows = 0
    for c in cases:
        W, p = c.o["world"](), c.p
        if G.KIND_NAME[c.kind] == "gen_pre" and p["V"] >= 1024 and "bias" in W:
            left = once = 0
            for row in range(p["n_rows"]):
                slot = G.slot_of(W, p, row)
                g = W["slots"][slot]
                if g["finish"] or g["kind"] == 2 or not g["has_bias"]:
                    continue
                x, pb, b = W["logits"][row], W["penalty"][slot].view(U32), W["bias"][slot]
                right = G.adjust(x, pb, b)
                left += int((G.adjust(x, pb, b, "assoc_left").view(U32) != right.view(U32)).sum())
                both = (pb != G.ABSENT) & (b != 0)
                with np.errstate(invalid="ignore"):
                    single = (x.astype(F64) - pb.view(F32).astype(F64) + b.astype(F64)).astype(F32)   # x + np + b rounded once (exact in float64, then to f32)
                once += int((single.view(U32) != right.view(U32))[both].sum())
            assert left >= 100 and once >= 100, (c.name, left, once)
            rows += 1
        if G.KIND_NAME[c.kind] == "gen_post" and c.group == "post":
            for row in range(p["n_rows"]):
                slot = G.slot_of(W, p, row)
                g, tok = W["slots"][slot], int(W["samp_tok"][row])
                if g["kind"] != 2 and 0 <= tok < p["V"] and W["penalty"][slot].view(U32)[tok] != G.ABSENT and not g["finish"]:
                    assert G.fused_differs(W["penalty"][slot][tok], g["decay"], g["frequency"]), c.name
                    rows += 1
    assert rows >= 30


def test_a_correct_launch_passes_and_an_untouched_one_does_not(cases):
    for c in cases:
        if c.p["V"] > 16400:
            continue
        d = G.make(c)
        res, _ = G.reference_results(c, d)
        assert G.check_case(c, d, res, G.plan_line(c)) == [], c.name
        assert G.check_case(c, d, P.untouched(d), G.plan_line(c)), f"{c.name}: a launch that writes nothing passes"
        assert G.check_case(c, d, res, dict(G.plan_line(c), mixed=1 - c.p["mixed"]))


def test_the_steps_stay_on_exact_rows_and_reach_what_they_are_for(cases):
    """Every row launch_nucleus sees in a `step` case is a family A row of tests/sample_cases.py (Src asserts it; here: counted), and the scenes
    end where the table says."""
    from tests import sample_cases as SC
    seen, made = {}, []
    real = SC.Src

    def counting(x, fam, levels=None):
        made.append(fam)
        return real(x, fam, levels)
    for c in cases:
        if c.group != "step":
            continue
        d = G.make(c)
        SC.Src = counting
        try:
            _, W = G.reference_results(c, d)
        finally:
            SC.Src = real
        seen[c.o["tags"]["scene"]] = (W, c.p, d["W"])
    assert len(made) == sum(p["n_rows"] * p["n_steps"] for _, p, _ in seen.values()) and set(made) == {"A"}
    W, p, W0 = seen["penalties_bias_stop"]
    first = G.row_slots(W0, p)[0]
    assert W["slots"][first]["finish"] == 1 and W["slots"][first]["freeze_at"] == 1 and W["slots"][first]["emitted"] == 2 and "bias" in W0
    assert W["slots"][G.row_slots(W0, p)[1]]["emitted"] == 0 and (W["slots"]["kind"] == 2).any()      # the rider from the start; a Mirostat slot beside
    W, p, W0 = seen["topn_capture_rider"]
    a, b = G.row_slots(W0, p)
    assert W["slots"][b]["finish"] == 2 and W["slots"][b]["freeze_at"] == 1 and W["slots"][a]["finish"] == 0
    assert (W["cap_mem"][b * p["V"]:(b + 1) * p["V"]] == W0["logits_steps"].reshape(3, 2, -1)[1, 1]).all()   # FINISH: the row of the step it finished in
    assert (W["top_ids"].reshape(-1, p["max_batch"], 32)[:3, a, :5] != P.SENT32).all() and (W["top_ids"].reshape(-1, p["max_batch"], 32)[:, b] == P.SENT32).all()
    W, p, W0 = seen["mixed_prompt_item_prefill"]
    assert W["run_step"][0] == 2 and W["slots"]["emitted"].tolist() == [0, 3, 0, 3, 3] and W["slots"]["draws"][4] == 3
    assert (W["cap_mem"][192:192 + p["V"]] == W0["logits_steps"].reshape(3, 3, -1)[0, 0]).all()       # PROMPT: the row of the step the prompt ended in
    W, p, W0 = seen["dfa_beside_pda"]
    a, b = G.row_slots(W0, p)
    assert W["dfa"][a]["state"] != W0["dfa"][a]["state"] or W["slots"][a]["emitted"] == 3
    assert (W["pda"][b]["depth"], W["pda"][b]["state"]) != (W0["pda"][b]["depth"], W0["pda"][b]["state"]) or W["pda"][b]["stack"][:2].tolist() != [1, 2]
    W, p, W0 = seen["watch_cancel"]
    a = G.row_slots(W0, p)[0]
    assert p["cancel_step"] == 1 and p["cancel_slot"] == a and not W0["ring"][2 * G.rec_bytes(3) + 16:].any()   # no word is set when the run begins
    assert W["slots"][a]["finish"] == 4 and W["slots"][a]["freeze_at"] == 1 and W["slots"][a]["emitted"] == 2 and W["watch"][0]["seq"] == 3
    assert (W["shadow_mem"][int(W0["shadow"][a]):][:192] == G.state_parts(W0, p, a)).all()             # gen_freeze of that later step took its state


WHERE = {"fused_decay": "post", "assoc_left": "pre", "by_value": "pre", "by_isnan": "pre", "topn_at_run_step": "topn", "feedback_slot": "post", "row_slot_mixed": "pre", "max_lt": "post",
         "stack_stage_64": "pda", "span_9": "pda", "capture_rider": "state", "freeze_always": "state", "cancel_no_draw": "publish", "stamp_seq": "publish",
         "guard_write": "pre", "neighbour_penalty": "pre"}


@pytest.mark.parametrize("bug", G.MISTAKES)
def test_every_mistake_is_reported(cases, bug):
    """The reference with one line changed as a kernel would get it wrong: check_case must report it in at least one case."""
    found = []
    for c in cases:
        if c.group != WHERE[bug] or c.p["V"] > 16400 or len(found) >= 2:
            continue
        d = G.make(c)
        res, _ = G.reference_results(c, d, bug)
        if G.check_case(c, d, res, G.plan_line(c)):
            found.append(c.name)
    assert found, f"no case of group {WHERE[bug]} reports the mistake {bug}"


def test_the_case_file_round_trip(cases, tmp_path):
    group = [c for c in cases if c.group == "tokens"] + [c for c in cases if c.name == "pre_V16_B3_m1"]
    datas = [G.make(c) for c in group]
    path = str(tmp_path / "cases.bin")
    G.write_cases(path, group, datas)
    back = P.read_cases(path, G.MAGIC)
    assert [b[0] for b in back] == [c.name for c in group]
    for (name, kind, par, bufs), c, d in zip(back, group, datas):
        assert kind == c.kind and list(par) == [c.p[k] for k in G.PARAMS] and len(bufs) == len(d["bufs"])
        for (role, esize, flags, nbytes, off, img), b in zip(bufs, d["bufs"]):
            assert (role, esize, flags, nbytes, off) == (G.ROLE[b.role], b.esize, b.flags, (b.n + 2 * P.GUARD) * b.esize, (P.GUARD + b.off) * b.esize)
            assert img is None if b.flags & 2 else (img == b.image).all()
            assert off % 16 == 0


def test_the_probe_compiles_for_gfx950(tmp_path):
    from ai00_server_amd import build as B
    assert "gen_probe" in B.PROBES
    obj = B.compile_probe("gen_probe", str(tmp_path / "gen_probe.o"))
    assert os.path.getsize(obj) > 0

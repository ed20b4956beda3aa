"""MI355X: resident generation under a stack-automaton constraint (rwkv_gen_set_pda / rwkv_gen_pda_config; gen_pda_mask_kernel, the commit in
gen_post_kernel) against the per-token path.

Modelled on tests/test_gpu_gen_dfa.py, whose helpers it imports unchanged.  Engine A is resident and carries the constraints.  Engine B runs
the per-token loop (`infer_sample`, host samplers, `gen_uniform`) with an `allow` mask per constrained slot from `PdaWalker` of
tests/test_pda_cpu.py — a numpy walk with an array stack per token, not rwkv_pda_allow — and commits / halts over the same walk.  Nothing is
compared with a tolerance: ids, `out_probs` bits, n_emitted, finish, (state, stack) of `gen_pda_config`, `state.back`.  A wrong mask bit moves
the softmax sum and with it the probability bits, so every step checks its whole mask.

The token table is synthetic: a single-byte token for every byte (the liveness rule), `{"` `":` `"},` `]]` `}]}` `],[` `[[`, nine `[` in
one token (the span rule), a token of RWKV_GEN_TOKEN_LEN bytes, unknown ids, an empty token, JSON fragments, and fewer entries than the
vocabulary.  After each case the concatenated output of a constrained slot, walked on the host, ends in the reported configuration, and
where the slot halted under the JSON automaton `json.loads` accepts it."""
import copy
import json

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from tests import test_gpu_gen_dfa as GD
from tests import test_gpu_gen_stop as GS
from tests.test_pda_cpu import PdaWalker, brackets, is_end

pytestmark = pytest.mark.gpu

PAD, MODELS, SEED, N, Fin, bits = GS.PAD, GS.MODELS, GS.SEED, GS.N, rt.GenFinish, GS.bits
J = rt.PdaJson
FRAGMENTS = [b'"a"', b'"b":', b',"c":', b"12", b"true", b"null", b"false", b"[]", b"{}", b":[", b'"}', b'"]', b"],", b"},", b',"', b"0.5", b"-1", b'{"k":',
             b"[1,", b'":"', b"e3", b'\\"', b"\\u00", b"\xc3\xa9", b"aa", b"a,", b",[", b"[a", b"a]", b"].", b"  ", b"\n", b"1]", b"1}"]


def table(V):
    """ids -> bytes (None: unknown).  Ids 1 .. 256 are the single bytes; entries V - 24 .. V - 1 are missing altogether."""
    rng = np.random.default_rng(20260112)
    out = [None] + [bytes([c]) for c in range(256)]
    out += [b'{"', b'":', b'"},', b"]]", b"}]}", b"],[", b"[[", b"[" * 9, b"[" * 8, b"", None, b'"' + b"a" * (rt.GEN_TOKEN_LEN - 2) + b'"', b"a" * rt.GEN_TOKEN_LEN]
    while len(out) < V - 24:
        u = rng.random()
        out.append(None if u < 0.05 else FRAGMENTS[int(rng.integers(0, len(FRAGMENTS)))] if u < 0.8 else
                   FRAGMENTS[int(rng.integers(0, len(FRAGMENTS)))] + FRAGMENTS[int(rng.integers(0, len(FRAGMENTS)))])
    return out


class PdaConstraint:
    """host side of one slot's stack constraint: the `Formatter` (transform = mask, update = commit and maybe halt) by the numpy walk"""

    def __init__(self, pda, walker, halt=rt.PdaHalt.Final, state=None, stack=()):
        self.pda, self.w, self.halt = pda, walker, halt
        self.nxt, self.act, self.acc = pda.table()
        self.q, self.stack = pda.start if state is None else state, list(stack)
        self._at, self._walked = None, None

    def walked(self):
        if self._at != (self.q, tuple(self.stack)):
            self._at, self._walked = (self.q, tuple(self.stack)), self.w.walk(self.nxt, self.act, self.pda.max_depth, self.q, self.stack)
        return self._walked

    def mask(self):
        return (self.walked()[0] != 0).astype(np.uint8)

    def update(self, tok):
        w = self.walked()
        if not w[0][tok]:
            return False
        self.q, self.stack = self.w.config_behind(w, self.stack, tok)
        return not self.stack and bool(self.acc[self.q]) and (self.halt == rt.PdaHalt.Accept or is_end(self.nxt, self.act, self.q))


class Cfg:
    """one slot: a sampler and at most one constraint — `pda` with an optional configuration, or `dfa`"""

    def __init__(self, sampler, pda=None, dfa=None, halt=0, state=None, stack=(), stops=None, max_tokens=N, wide=False):
        self.sampler, self.pda, self.dfa, self.halt, self.state, self.stack = sampler, pda, dfa, halt, state, list(stack)
        self.stops, self.max_tokens, self.wide = stops, max_tokens, wide


def constraints(cfgs, tab, V):
    pw, dw = PdaWalker(tab, V), GD.Walker(tab, V)
    return [PdaConstraint(c.pda, pw, c.halt, c.state, c.stack) if c.pda else GD.Constraint(c.dfa, dw, c.halt) if c.dfa else None for c in cfgs]


def arm(A, cfgs, smp, first, tab):
    A.gen_set_token_bytes(tab)
    for b, c in enumerate(cfgs):
        A.gen_arm(b, first[b], c.max_tokens, copy.deepcopy(smp[b]), seed=SEED, wide_top_k=c.wide)
        if c.pda is not None:
            A.gen_set_pda(b, c.pda, c.state, c.stack, halt=c.halt)
        if c.dfa is not None:
            A.gen_set_constraint(b, c.dfa, halt=c.halt)
        if c.stops is not None:
            A.gen_set_stops(b, c.stops)


def check(A, cfgs, ref, t, p, ne, fin, slabs=True):
    """A emitted exactly B's tokens, bit for bit, and nothing behind them; finish, configuration and slab are B's"""
    for b in range(3):
        k = len(ref["toks"][b])
        c = ref["cons"][b]
        print("slot", b, "finish", ref["fin"][b], "config", (c.q, getattr(c, "stack", None)) if c else None, "tokens", ref["toks"][b])
        assert int(ne[b]) == k
        np.testing.assert_array_equal(t[:k, b], np.array(ref["toks"][b], np.uint32))
        np.testing.assert_array_equal(bits(p[:k, b]), bits(ref["probs"][b]))
        assert (t[k:, b] == PAD).all() and np.isnan(p[k:, b]).all()
        assert int(fin[b]) == ref["fin"][b]
        assert A.gen_pda_config(b) == ((c.q, c.stack) if cfgs[b].pda else (0, []))
        assert A.gen_constraint_state(b) == (c.q if cfgs[b].dfa else 0)
        if slabs:
            np.testing.assert_array_equal(A.state.back(b), ref["slab"][b])


def check_text(cfgs, ref, tab, toks=None):
    """the concatenated output of every slot under a stack constraint, walked byte by byte on the host, ends in the reported configuration; a
    JSON slot that halted wrote a document `json.loads` takes"""
    for b, c in enumerate(cfgs):
        if c.pda is None:
            continue
        cons = ref["cons"][b]
        ws = [tab[x] for x in (toks[b] if toks else ref["toks"][b])]
        ws = ws[:-1] if ws and ref["fin"][b] == Fin.Stop and (ws[-1] is None or toks is None and ref["toks"][b][-1] == 0) else ws     # a stop by token 0 / an unknown id
        assert c.pda.walk(b"".join(ws), c.state, c.stack) == (cons.q, cons.stack) and cons.q != 0
        halted = ref["fin"][b] == Fin.Stop and not cons.stack and cons.acc[cons.q] and c.stops is None and ws and ref["toks"][b][-1] != 0
        if halted and getattr(c, "prefix", None) is not None:
            json.loads((c.prefix + b"".join(ws)).decode("utf-8"))


def run_case(name, quant, cfgs, n=N):
    A, Bn, V, prompts, first = GD.start_pair(name, quant)
    tab = table(V)
    smp = GD.armed_samplers(cfgs, prompts, first)
    arm(A, cfgs, smp, first, tab)
    t, p, ne, fin = A.gen_run(n)
    ref = GD.per_token(Bn, cfgs, smp, first, tab, None, n, cons=constraints(cfgs, tab, V))
    check(A, cfgs, ref, t, p, ne, fin)
    check_text(cfgs, ref, tab)
    A.close()
    Bn.close()
    return ref, t, p, tab


def json_at(flags, prefix, halt=rt.PdaHalt.Final, max_depth=rt.PDA_MAX_DEPTH, sampler=None, **kw):
    """a slot under the JSON automaton in the configuration behind `prefix`"""
    pda = rt.Pda.json(flags, max_depth)
    q, st = pda.walk(prefix)
    assert q != 0
    c = Cfg(sampler or GD.penalised(), pda, halt=halt, state=q, stack=st, **kw)
    c.prefix = prefix
    return c


def bracket_pda(max_depth=3):
    n, a, acc = brackets()
    return rt.Pda.from_table(n, a, acc, max_depth=max_depth)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_a_json_slot_a_dfa_slot_and_a_free_slot_in_one_step(name, quant):
    """Slot 0: JSON(OBJECT | COMPACT) from its start.  Slot 1: a DFA (gen_mask_kernel and gen_pda_mask_kernel both run, each returns at once
    on the other's row).  Slot 2: free; its output equals B, so neither mask touched its row."""
    cfgs = [json_at(J.Object | J.Compact, b""), Cfg(H.NucleusSampler(), dfa=rt.Dfa.compile(rb'([\[\]{}",:]|[a-z0-9])*')), Cfg(H.TypicalSampler(tau=0.9, top_k=32))]
    ref, t, p, tab = run_case(name, quant, cfgs)
    assert tab[ref["toks"][0][0]][:1] in (b"{", b"[")                   # OBJECT: the first token opens a container


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def high_ids():
    """600 states that count DOWN on `a`; `[` pushes the state below as the return state, `]` pops: every stack entry needs the high byte"""
    n, a = np.zeros((601, 256), np.uint16), np.zeros((601, 256), np.uint16)
    n[1, ord("a")] = 1
    for q in range(2, 601):
        n[q, ord("a")] = q - 1
        n[q, ord("[")], a[q, ord("[")] = q - 1, q - 1
        a[q, ord("]")] = rt.PDA_POP
    return rt.Pda.from_table(n, a, (np.arange(601) > 0).astype(np.uint8), start=600, max_depth=5)


CONFIGS = {
    "brackets": lambda: [Cfg(GD.penalised(), bracket_pda(3), state=1, stack=[]),                 # depth 0
                         Cfg(H.NucleusSampler(), bracket_pda(3), state=2, stack=[1, 2, 2]),      # depth max_depth = 3: every push is dead
                         Cfg(H.TypicalSampler(tau=0.9, top_k=32), bracket_pda(3), state=2, stack=[1, 2])],    # `],[` and `]]` are allowed
    "json": lambda: [json_at(0, b"[" * 64),                                                      # JSON at depth 64 = max_depth
                     json_at(J.Compact, b'{"a":[{"b":1', sampler=H.NucleusSampler()),             # `}]}` `]]`-free: `}]}` is allowed here ...
                     json_at(J.Compact, b'[{"b":1', sampler=H.TypicalSampler(tau=0.9, top_k=32))],   # ... and dies on the empty stack here
    "high": lambda: [Cfg(GD.penalised(), high_ids(), state=600, stack=[]), Cfg(H.NucleusSampler(), high_ids(), state=400, stack=[399, 398]),
                     Cfg(H.TypicalSampler(tau=0.9, top_k=32), high_ids(), state=300, stack=[299, 298, 297, 296, 295])],
    "empty": lambda: [Cfg(GD.penalised(), bracket_pda(3), state=2, stack=[1]),                   # `],[` and `]]` die: the pop uncovers TOP
                      Cfg(H.NucleusSampler(), bracket_pda(64), state=2, stack=[1] + [2] * 55),    # eight `[` fit, nine never do
                      Cfg(H.TypicalSampler(tau=0.9, top_k=32), bracket_pda(64), state=2, stack=[1] + [2] * 56)],   # 57 + 8 > 64: eight do not fit either
}


def first_masks_are_as_spelled_out(which, cfgs, tab, V):
    """the masks of the first step, spelled out from the tables by hand: B's numpy walk must give them, and A's probability bits B's"""
    idx = {w: i for i, w in reversed(list(enumerate(tab))) if w}
    masks = [c.mask() for c in constraints(cfgs, tab, V)]

    def allowed(b, *words):
        return [bool(masks[b][idx[w]]) for w in words]
    if which == "brackets":
        assert allowed(0, b"a", b"[", b"[[", b"[" * 8, b"[" * 9, b"]", b"]]", b"],[") == [True, True, True, False, False, False, False, False]   # max_depth 3
        assert allowed(1, b"a", b"[", b"]", b"]]", b"],[", b"[[") == [True, False, True, True, True, False]
        assert allowed(2, b"a", b"[", b"[[", b"]", b"]]", b"],[") == [True, True, False, True, True, True]      # `]]` empties the stack: TOP is live
    if which == "json":
        assert allowed(0, b"[", b"{", b"1", b"]", b"]]", b'"', b"[[", b"[]") == [False, False, True, True, True, True, False, False]
        assert allowed(1, b"}]}", b"}", b"]", b"]]", b",") == [True, True, False, False, True]
        assert allowed(2, b"}]}", b"}", b"},", b"1]", b"1}") == [False, True, True, False, True]
    if which == "empty":
        assert allowed(0, b"]", b"]]", b"],[", b"a]", b"[[") == [True, False, False, True, True]
        assert allowed(1, b"[" * 8, b"[" * 9, b"[[") == [True, False, True]
        assert allowed(2, b"[" * 8, b"[" * 9, b"[[") == [False, False, True]
    if which == "high":
        assert allowed(0, b"a", b"[", b"]", b"[[", b"aa") == [True, True, False, True, True]
        assert allowed(2, b"a", b"[", b"]", b"]]") == [True, False, True, True]


@pytest.mark.parametrize("which", list(CONFIGS))
@pytest.mark.parametrize("name,quant", MODELS[:1])
def test_chosen_configurations_two_steps_each(name, quant, which):
    """Configurations set explicitly through rwkv_gen_set_pda, so that the coverage does not depend on what a random model draws."""
    cfgs = CONFIGS[which]()
    V = 1024
    first_masks_are_as_spelled_out(which, cfgs, table(V), V)
    ref, _, _, _ = run_case(name, quant, cfgs, n=2)
    assert all(len(x) == 2 for x in ref["toks"])


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_both_halt_modes_and_max_tokens(name, quant):
    """Slot 0: HALT_FINAL under OBJECT | COMPACT, two tokens from a possible end.  Slot 1: HALT_ACCEPT under plain JSON behind `[1`, where
    FINAL could never halt (whitespace may always follow).  Slot 2: max_tokens = 5 from the start: RWKV_GEN_LENGTH unless it closed before."""
    cfgs = [json_at(J.Object | J.Compact, b'{"k":nul'), json_at(0, b"[1", halt=rt.PdaHalt.Accept, sampler=H.NucleusSampler()),
            json_at(J.Object | J.Compact, b"", max_tokens=5)]
    ref, t, p, tab = run_case(name, quant, cfgs)
    assert tab[ref["toks"][0][0]] == b"l"                               # the only way on
    for b in (0, 1):
        c = ref["cons"][b]
        assert (ref["fin"][b] == Fin.Stop) == (not c.stack and bool(c.acc[c.q])) and ref["fin"][b] in (Fin.Stop, Fin.Length)
    assert ref["fin"][2] in (Fin.Stop, Fin.Length) and len(ref["toks"][2]) <= 5


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_a_stack_constraint_and_stop_strings_on_one_slot(name, quant):
    """The STOPS instantiation of gen_post_kernel with a stack constraint: slot 0 has a string that matches early (`,` or `:`), slot 1 one that
    never matches, slot 2 none (it takes the token-stop path inside the STOPS launch)."""
    cfgs = [json_at(J.Compact, b'{"k"', stops=[b"zz", b",", b":"]), json_at(J.Compact, b"[", stops=[b"zzz"], sampler=H.NucleusSampler()),
            json_at(J.Object | J.Compact, b"", halt=rt.PdaHalt.Accept, sampler=H.TypicalSampler(tau=0.9, top_k=32))]
    ref, t, p, tab = run_case(name, quant, cfgs)
    text0 = b"".join(tab[x] for x in ref["toks"][0])
    assert ref["fin"][0] == Fin.Stop and len(ref["toks"][0]) == 1 and text0.startswith(b":")   # behind the key only `:` leads on: the string matches at once


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_the_first_draw_of_a_prompt_is_masked_in_a_mixed_step(name, quant):
    """Slot 0 decodes under a stack constraint while slot 1 is admitted with an 11-token prompt (two mixed steps: 7 + 4 tokens next to slot 0's
    row); slot 1's first draw, in the second mixed step, is masked with the start configuration."""
    A, Bn = GS.build(name, quant), GS.build(name, quant)
    V = A.info.num_vocab
    tab = table(V)
    walker = PdaWalker(tab, V)
    pda = rt.Pda.json(J.Object | J.Compact)
    p0, p1 = GS.prompt(V, 61, 5), GS.prompt(V, 62, 11)
    first = []
    for eng in (A, Bn):
        inp = rt.RnnInput([rt.RnnInputBatch(list(p0)), rt.RnnInputBatch(), rt.RnnInputBatch()])
        while inp.num_token() > 0:
            inp, outs = eng.infer(inp)
        first.append(int(np.argmax(outs[0][-1])))
    assert first[0] == first[1]
    s0, s1 = GD.penalised(), H.TypicalSampler(tau=0.9, top_k=32)
    s0.init(p0)
    s0.update(first[0])
    s1.init(p1)
    q0, st0 = pda.walk(b'[{"a":')
    A.gen_set_token_bytes(tab)
    A.gen_arm(0, first[0], N, copy.deepcopy(s0), seed=SEED)
    A.gen_arm_prompt(1, p1, N, copy.deepcopy(s1), seed=SEED)
    A.gen_set_pda(0, pda, q0, st0)
    A.gen_set_pda(1, pda)                                              # the start state, an empty stack
    n = 8
    t, p, ne, fin = A.gen_run(n)
    c0, c1 = PdaConstraint(pda, walker, state=q0, stack=st0), PdaConstraint(pda, walker)
    cur, left, draws1 = [first[0], None], list(p1), 0
    want, done = {0: [], 1: []}, [False, False]
    for d in range(n):
        s0.allow, s1.allow = c0.mask(), c1.mask()
        inp = rt.RnnInput([rt.RnnInputBatch([cur[0]]), rt.RnnInputBatch(list(left) if left else [cur[1]]), rt.RnnInputBatch()])
        inp, res = Bn.infer_sample(inp, [s0, s1, None], [rt.gen_uniform(SEED, 0, d), rt.gen_uniform(SEED, 1, draws1), 0.0])
        left = list(inp.batches[1].tokens) if left else []
        for b, s, c in ((0, s0, c0), (1, s1, c1)):
            if res[b] is None or done[b]:
                want[b].append(None)
                continue
            tok, prob = res[b]
            s.update(tok)
            done[b] = c.update(tok) or tok == 0
            cur[b] = tok
            want[b].append((tok, prob))
            draws1 += b
    assert want[1][0] is None and want[1][1] is not None and not left      # 7 + 4: the first draw is in the second mixed step
    for b in (0, 1):
        got = [(int(t[d, b]), float(p[d, b])) if t[d, b] != PAD else None for d in range(n)]
        print("slot", b, "want", want[b], "got", got)
        assert [g and g[0] for g in got] == [w and w[0] for w in want[b]]
        np.testing.assert_array_equal(bits([g[1] for g in got if g]), bits([w[1] for w in want[b] if w]))
    assert A.gen_pda_config(0) == (c0.q, c0.stack) and A.gen_pda_config(1) == (c1.q, c1.stack)
    assert tab[want[1][1][0]][:1] in (b"{", b"[") and [int(f != 0) for f in fin[:2]] == [int(x) for x in done]
    A.close()
    Bn.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_runs_of_one_step_the_per_token_path_and_back(name, quant):
    """gen_run(1) x 3, then runs of 4 and 6, equal B's 13 steps, the configuration read back after each; then the request goes on per token
    ON ENGINE A with `harness.PdaFormatter` (whose mask is rwkv_pda_allow) started from `gen_pda_config` for 5 steps; then it is armed again
    from the formatter's configuration and runs 5 resident steps.  Plain JSON never halts under HALT_FINAL, so nobody finishes."""
    cfgs = [json_at(0, b"["), json_at(0, b'{"a":[', sampler=H.NucleusSampler()), json_at(0, b"", sampler=H.TypicalSampler(tau=0.9, top_k=32))]
    for c in cfgs:
        c.max_tokens = 99
    A, Bn, V, prompts, first = GD.start_pair(name, quant)
    tab = table(V)
    smp = GD.armed_samplers(cfgs, prompts, first)
    arm(A, cfgs, smp, first, tab)
    host = copy.deepcopy(smp)                                          # the caller's own samplers, replayed over A's output
    done, ref, last, out = 0, None, list(first), [[], [], []]
    keep = ("cons", "matchers", "cur", "emitted")
    for steps in (1, 1, 1, 4, 6):
        t, p, ne, fin = A.gen_run(steps)
        ref = GD.per_token(Bn, cfgs, smp, first, tab, None, steps, d0=done, **({"cons": constraints(cfgs, tab, V)} if ref is None else {k: ref[k] for k in keep}))
        assert ref["fin"] == [0, 0, 0], "a slot drew token 0: choose another prompt base"
        check(A, cfgs, ref, t, p, ne, fin)
        for b in range(3):
            for x in t[:, b]:
                host[b].update(int(x))
                out[b].append(int(x))
            last[b] = int(t[-1, b])
        done += steps
    fms = [H.PdaFormatter(c.pda, tab, V, *A.gen_pda_config(b)) for b, c in enumerate(cfgs)]
    ref = GD.per_token(Bn, cfgs, smp, first, tab, None, 5, d0=done, **{k: ref[k] for k in keep})
    for i, d in enumerate(range(done, done + 5)):
        for b in range(3):
            host[b].allow = fms[b].transform()
        _, res = A.infer_sample(rt.RnnInput([rt.RnnInputBatch([last[b]]) for b in range(3)]), host, [rt.gen_uniform(SEED, b, d) for b in range(3)])
        for b in range(3):
            tok, prob = res[b]
            assert tok == ref["toks"][b][i] and bits(prob) == bits(ref["probs"][b][i]), (d, b)
            host[b].update(tok)
            out[b].append(tok)
            last[b] = tok
            assert fms[b].update(tok) is False
    assert [(f.state, f.stack) for f in fms] == [(c.q, c.stack) for c in ref["cons"]]
    # ... and back: armed again behind `last`, the configuration handed in; the draws of a newly armed slot start at 0 again
    for b, c in enumerate(cfgs):
        host[b].allow = None
        A.gen_arm(b, last[b], 99, copy.deepcopy(host[b]), seed=SEED)
        A.gen_set_pda(b, c.pda, fms[b].state, fms[b].stack)
    t, p, ne, fin = A.gen_run(5)
    ref = GD.per_token(Bn, cfgs, host, first, tab, None, 5, d0=0, cons=ref["cons"], matchers=ref["matchers"], cur=ref["cur"], emitted=[0, 0, 0])
    check(A, cfgs, ref, t, p, ne, fin)
    for b in range(3):
        out[b] += ref["toks"][b]
    check_text(cfgs, ref, tab, toks=out)
    A.close()
    Bn.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_constrained_slots_that_take_the_wide_kernel(name, quant):
    """Slot 0: Mirostat with target 4.5 (4 * target >= 13: the wide kernel for its whole life) under a stack constraint.  Slot 1: Nucleus with
    top_k = 512, armed with RWKV_GEN_WIDE_TOP_K.  Slot 2: narrow, constrained."""
    cfgs = [json_at(J.Object | J.Compact, b"", sampler=H.MirostatSampler(tau=4.5, rate=0.1)),
            json_at(J.Compact, b"[", sampler=H.NucleusSampler(top_p=0.9, top_k=512, temperature=1.1), wide=True), json_at(0, b'{"a":', sampler=H.NucleusSampler())]
    ref, _, _, _ = run_case(name, quant, cfgs, n=16)
    assert all(f in (0, Fin.Stop, Fin.Length) for f in ref["fin"])


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_refusals_and_what_clears_a_constraint():
    name, quant = MODELS[0]
    A = GS.build(name, quant)
    V = A.info.num_vocab
    tab = table(V)
    pda, dfa = rt.Pda.json(J.Object | J.Compact, 4), rt.Dfa.compile(rb"[a-z\[\]]*")

    def code(fn):
        with pytest.raises(rt.RwkvError) as e:
            fn()
        return e.value.code
    assert code(lambda: A.gen_set_pda(0, pda)) == -1                     # nothing armed yet
    smp = H.NucleusSampler()
    A.gen_arm(0, 5, 8, smp, seed=SEED)
    assert code(lambda: A.gen_set_pda(0, pda)) == -1                     # no token table
    A.gen_set_token_bytes(tab)
    assert code(lambda: A.gen_set_pda(1, pda)) == -1                     # slot 1 is not armed
    assert code(lambda: A.gen_pda_config(1)) == -1
    assert code(lambda: A.gen_set_pda(0, pda, state=0)) == -1            # the dead state
    assert code(lambda: A.gen_set_pda(0, pda, state=pda.num_states)) == -1
    assert code(lambda: A.gen_set_pda(0, pda, halt=2)) == -1
    q, st = pda.walk(b"[[[[")
    assert len(st) == 4
    assert code(lambda: A.gen_set_pda(0, pda, q, st + [st[-1]])) == -1   # deeper than max_depth
    assert code(lambda: A.gen_set_pda(0, pda, q, [0] + st[1:])) == -1    # a dead stack entry
    assert code(lambda: A.gen_set_pda(0, pda, q, [pda.num_states] + st[1:])) == -1
    assert code(lambda: A.gen_set_pda(0, pda, *pda.walk(b"[]"))) == -3   # liveness: the configuration's own state has no way on
    assert A.gen_pda_config(0) == (0, [])
    A.gen_set_pda(0, pda, q, st)
    assert A.gen_pda_config(0) == (q, st) and A.gen_constraint_state(0) == 0
    assert code(lambda: A.gen_set_constraint(0, dfa)) == -1              # a slot holds a DFA or a stack constraint
    assert code(lambda: A.gen_set_token_bytes(tab)) == -1                # a slot walks the table
    A.gen_set_constraint(0, None)                                        # NULL through the call of the other kind leaves it alone
    assert A.gen_pda_config(0) == (q, st)
    A.gen_set_pda(0, None)                                               # NULL clears it
    assert A.gen_pda_config(0) == (0, [])
    A.gen_set_constraint(0, dfa)
    assert code(lambda: A.gen_set_pda(0, pda)) == -1                     # ... the other way round
    A.gen_set_pda(0, None)
    assert dfa.start != 0 and A.gen_constraint_state(0) == dfa.start     # ... in both: the state it was set with
    A.gen_set_constraint(0, None)
    A.gen_set_token_bytes(tab)
    no_colon = [None if w == b":" else w for w in tab]
    A.gen_set_token_bytes(no_colon)
    assert code(lambda: A.gen_set_pda(0, pda)) == -3                     # liveness: no single-byte `:` (`":` remains and does not count)
    A.gen_set_token_bytes(tab)
    A.gen_set_pda(0, pda)
    A.gen_arm(0, 5, 8, smp, seed=SEED)                                   # re-arming clears it
    assert A.gen_pda_config(0) == (0, [])
    A.gen_set_token_bytes(tab)
    A.gen_set_pda(0, pda)
    A.gen_disarm(0)                                                      # ... and so does what disarms the slot
    A.gen_set_token_bytes(tab)
    A.gen_arm(0, 5, 8, smp, seed=SEED)
    A.gen_set_pda(0, pda)
    t, _, ne, fin = A.gen_run(8)
    q, st = A.gen_pda_config(0)
    text = b"".join(tab[x] for x in t[:ne[0], 0] if x and tab[x])
    assert ne[0] >= 1 and fin[0] in (Fin.Length, Fin.Stop) and q != 0 and pda.walk(text) == (q, st) and len(st) <= 4
    assert code(lambda: A.gen_set_pda(0, pda)) == -1                     # a finished slot
    A.close()

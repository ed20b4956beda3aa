"""MI355X: resident generation under a byte-automaton constraint (rwkv_gen_set_constraint / _constraint_state; gen_mask_kernel, the halt
in gen_post_kernel) against the per-token path.

Engine A is resident and carries the constraints.  Engine B runs the per-token loop of tests/test_gpu_generate.py (`infer_sample`, host
samplers, `gen_uniform`) with an `allow` mask per constrained slot that `Walker` below computes — a numpy walk written here, not
rwkv_dfa_allow — and advances / halts by `Constraint.update`, over the same walk.  A constraint changes what is drawn, so every case
realises its own B.  Nothing is compared with a tolerance: ids, `out_probs` bits, n_emitted, finish, `gen_constraint_state`, `state.back`.

The token table is synthetic: single-byte tokens for the whole alphabet `abc;` (the liveness rule), words of 2-5 letters, some ending
in `;`, one token of exactly RWKV_GEN_TOKEN_LEN bytes, unknown ids, an empty token, and fewer entries than the vocabulary.

Within one rwkv_gen_run a finished slot rides along, so every step keeps B's three rows (B keeps stepping a finished slot and drops what
it draws); cases that use several runs finish nobody before the last one."""
import copy

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from tests import test_gpu_gen_stop as GS

pytestmark = pytest.mark.gpu

PAD = GS.PAD
MODELS = GS.MODELS
SEED = GS.SEED
N = GS.N
Fin = rt.GenFinish
bits = GS.bits
GROUPS = rb"([abc]{2,8};){1,3}"           # accepts behind every `;`, is FINAL behind the third: at most 27 tokens, at least 6
LOOP = rb"([abc]{1,6};)*"                 # accepts behind every `;` and always leads on: never FINAL


def table(V):
    """ids -> bytes (None: unknown).  Entries V - 24 .. V - 1 are missing altogether."""
    rng = np.random.default_rng(20251118)
    out = [None, b"a", b"b", b"c", b";", b"", b"a" * rt.GEN_TOKEN_LEN]
    while len(out) < V - 24:
        u = rng.random()
        word = bytes(rng.choice([97, 98, 99], int(rng.integers(2, 6))).tolist())
        out.append(None if u < 0.06 else word[:1] + b";" if u < 0.16 else b"d" + word if u < 0.20 else word)
    return out


class Walker:
    """the numpy walk: every token of the table from one state at once, one gather per byte position"""

    def __init__(self, tab, V):
        self.tab, self.V, n = tab, V, len(tab)
        self.lens = np.array([-1 if w is None else len(w) for w in tab])
        self.grid = np.zeros((n, max(1, int(self.lens.max()))), np.uint8)
        for i, w in enumerate(tab):
            if w:
                self.grid[i, :len(w)] = np.frombuffer(w, np.uint8)

    def ends(self, trans, q):
        """state each id of the vocabulary ends in from q, 0 = not allowed"""
        s = np.full(len(self.tab), q, np.int64)
        for k in range(self.grid.shape[1]):
            go = self.lens > k
            s[go] = trans[s[go], self.grid[go, k]]
        s[self.lens <= 0] = 0
        s[0] = 0                                                     # token 0 is never allowed
        out = np.zeros(self.V, np.int64)
        out[:len(s)] = s
        return out


class Constraint:
    """host side of one slot's constraint: the `Formatter` (transform = mask, update = advance and maybe halt) by the numpy walk"""

    def __init__(self, dfa, walker, halt=rt.DfaHalt.Final, state=None):
        self.dfa, self.w, self.halt = dfa, walker, halt
        self.trans, self.acc = dfa.table()
        self.q = dfa.start if state is None else state
        self._ends = None

    def mask(self):
        self._ends = self.w.ends(self.trans, self.q)
        return (self._ends != 0).astype(np.uint8)

    def update(self, tok):
        e = int(self.w.ends(self.trans, self.q)[tok])
        if not e:
            return False
        self.q = e
        return bool(self.acc[e]) and (self.halt == rt.DfaHalt.Accept or not self.trans[e].any())


class Cfg:
    def __init__(self, sampler, dfa=None, halt=rt.DfaHalt.Final, stops=None, max_tokens=N, wide=False):
        self.sampler, self.dfa, self.halt, self.stops, self.max_tokens, self.wide = sampler, dfa, halt, stops, max_tokens, wide


def is_miro(s):
    return getattr(s, "kind", 0) == 2


def armed_samplers(cfgs, prompts, first):
    out = []
    for b, c in enumerate(cfgs):
        s = copy.deepcopy(c.sampler)
        if not is_miro(s):
            s.init(prompts[b])
            s.update(first[b])
        out.append(s)
    return out


def start_pair(name, quant, base=80):
    A, Bn = GS.build(name, quant), GS.build(name, quant)
    V = A.info.num_vocab
    prompts = [GS.prompt(V, base + b, 5 + 2 * b) for b in range(3)]
    first = GS.prefill(A, prompts)
    assert GS.prefill(Bn, prompts) == first
    return A, Bn, V, prompts, first


def per_token(Bn, cfgs, smp, first, tab, walker, n, d0=0, cons=None, matchers=None, cur=None, emitted=None):
    """n steps of all three slots on B from draw d0.  Returns per slot: toks, probs, finish, the constraint state, the slab of the state
    rule (taken at the step the slot finishes in, or after the last step)."""
    cons = cons if cons is not None else [Constraint(c.dfa, walker, c.halt) if c.dfa else None for c in cfgs]
    matchers = matchers if matchers is not None else [H.StopMatcher(c.stops, cap=rt.GEN_STOP_BUF) if c.stops is not None else None for c in cfgs]
    cur = list(first) if cur is None else cur
    emitted = [0, 0, 0] if emitted is None else emitted
    toks, probs, fin, slab = [[], [], []], [[], [], []], [0, 0, 0], [None] * 3
    for d in range(d0, d0 + n):
        for b in range(3):
            smp[b].allow = cons[b].mask() if cons[b] is not None and not fin[b] else None
        us = [rt.gen_uniform(SEED, b, d) for b in range(3)]
        _, res = Bn.infer_sample(rt.RnnInput([rt.RnnInputBatch([cur[b]]) for b in range(3)]), smp, us)
        for b in range(3):
            tok, prob = res[b]
            cur[b] = tok
            if fin[b]:
                continue                                             # a rider: its row is computed and thrown away
            smp[b].update(prob if is_miro(smp[b]) else tok)
            toks[b].append(tok)
            probs[b].append(prob)
            emitted[b] += 1
            halt = cons[b].update(tok) if cons[b] is not None else False
            stop_token, at_max = tok == 0 or halt, emitted[b] >= cfgs[b].max_tokens
            if matchers[b] is not None:
                fin[b] = int(matchers[b].advance(tab[tok] if tok < len(tab) else None, stop_token=stop_token, at_max=at_max)[0])
            else:
                fin[b] = int(Fin.Stop) if stop_token else int(Fin.Length) if at_max else 0
            if fin[b]:
                slab[b] = Bn.state.back(b)
    for b in range(3):
        if slab[b] is None:
            slab[b] = Bn.state.back(b)
    return dict(toks=toks, probs=probs, fin=fin, q=[c.q if c is not None else 0 for c in cons], slab=slab, cons=cons, matchers=matchers, cur=cur,
                emitted=emitted)


def arm(A, cfgs, smp, first, tab):
    A.gen_set_token_bytes(tab)
    for b, c in enumerate(cfgs):
        A.gen_arm(b, first[b], c.max_tokens, copy.deepcopy(smp[b]), seed=SEED, wide_top_k=c.wide)
        if c.dfa is not None:
            A.gen_set_constraint(b, c.dfa, halt=c.halt)
        if c.stops is not None:
            A.gen_set_stops(b, c.stops)


def check(A, ref, t, p, ne, fin, slabs=True):
    """A emitted exactly B's tokens, bit for bit, and nothing behind them; finish, constraint state and slab are B's"""
    for b in range(3):
        k = len(ref["toks"][b])
        print("slot", b, "finish", ref["fin"][b], "state", ref["q"][b], "tokens", ref["toks"][b])
        assert int(ne[b]) == k
        np.testing.assert_array_equal(t[:k, b], np.array(ref["toks"][b], np.uint32))
        np.testing.assert_array_equal(bits(p[:k, b]), bits(ref["probs"][b]))
        assert (t[k:, b] == PAD).all() and np.isnan(p[k:, b]).all()
        assert int(fin[b]) == ref["fin"][b]
        assert A.gen_constraint_state(b) == ref["q"][b]
        if slabs:
            np.testing.assert_array_equal(A.state.back(b), ref["slab"][b])


def run_case(name, quant, cfgs, n=N):
    A, Bn, V, prompts, first = start_pair(name, quant)
    tab = table(V)
    walker = Walker(tab, V)
    smp = armed_samplers(cfgs, prompts, first)
    arm(A, cfgs, smp, first, tab)
    t, p, ne, fin = A.gen_run(n)
    ref = per_token(Bn, cfgs, smp, first, tab, walker, n)
    check(A, ref, t, p, ne, fin)
    for b, c in enumerate(cfgs):                                     # what came out is in the language's prefix set, token by token
        if c.dfa is not None:
            text = b"".join(tab[x] for x in ref["toks"][b])
            assert c.dfa.walk(c.dfa.start, text) == ref["q"][b] != 0
    A.close()
    Bn.close()
    return ref, t, p


def penalised():
    return H.NucleusSampler(top_p=0.8, top_k=32, temperature=1.2, frequency_penalty=0.4)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_constrained_slots_next_to_an_unconstrained_one(name, quant):
    """Slot 0 (Nucleus with penalties) and slot 2 (Typical) are constrained, slot 1 is not: its output equals B AND a resident run in which
    nobody is constrained (the step without gen_mask), bit for bit."""
    dfa = rt.Dfa.compile(LOOP)
    cfgs = [Cfg(penalised(), dfa), Cfg(H.NucleusSampler()), Cfg(H.TypicalSampler(tau=0.9, top_k=32), dfa)]
    ref, t, p = run_case(name, quant, cfgs)
    assert ref["fin"][0] == ref["fin"][2] == Fin.Length                # LOOP never halts under FINAL (slot 1 may draw token 0: B says so too)
    A0, Bn, V, prompts, first = start_pair(name, quant)
    Bn.close()
    free = [Cfg(c.sampler) for c in cfgs]
    arm(A0, free, armed_samplers(free, prompts, first), first, table(V))
    t0, p0, _, _ = A0.gen_run(N)
    np.testing.assert_array_equal(t0[:, 1], t[:, 1])
    np.testing.assert_array_equal(bits(p0[:, 1]), bits(p[:, 1]))
    assert (t0[:, 0] != t[:, 0]).any() and (t0[:, 2] != t[:, 2]).any()    # ... and the constraint did bite on the other two
    assert A0.gen_constraint_state(1) == 0
    A0.close()


# ---- 2, 3, 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_both_halt_modes_and_max_tokens(name, quant):
    """One automaton on all three slots.  Slot 0: HALT_FINAL is reached in mid-run (RWKV_GEN_STOP at that token, the slot rides along,
    the state rule holds).  Slot 1: HALT_ACCEPT stops earlier, at the first `;`.  Slot 2: max_tokens = 5 comes first (FINAL needs six
    tokens at least): RWKV_GEN_LENGTH."""
    dfa = rt.Dfa.compile(GROUPS)
    s = penalised
    cfgs = [Cfg(s(), dfa), Cfg(s(), dfa, halt=rt.DfaHalt.Accept), Cfg(s(), dfa, max_tokens=5)]
    ref, t, p = run_case(name, quant, cfgs)
    n0, n1 = len(ref["toks"][0]), len(ref["toks"][1])
    assert ref["fin"] == [Fin.Stop, Fin.Stop, Fin.Length] and 6 <= n0 <= 27 and 2 <= n1 <= 9 and len(ref["toks"][2]) == 5
    _, acc = dfa.table()
    text0, text1 = (b"".join(table(1024)[x] for x in ref["toks"][b]) for b in (0, 1))
    assert text0.count(b";") == 3 and text0.endswith(b";") and text1.count(b";") == 1 and text1.endswith(b";")
    assert acc[ref["q"][0]] and acc[ref["q"][1]] and not dfa.table()[0][ref["q"][0]].any() and dfa.table()[0][ref["q"][1]].any()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_a_constraint_and_stop_strings_on_one_slot(name, quant):
    """The STOPS instantiation with a constraint.  Slot 0: the string `;` matches at the first `;`, long before the automaton is FINAL: the
    string wins.  Slot 1: a string that never matches: the halt wins.  Slot 2: a buffer that is full (it can never be sent) and a
    HALT_ACCEPT constraint: the halting token does not fit the buffer, and the finish is STOP, not HANDBACK."""
    dfa = rt.Dfa.compile(GROUPS)
    cfgs = [Cfg(penalised(), dfa, stops=[b"zz", b";"]), Cfg(penalised(), dfa, stops=[b"zzz"]), Cfg(penalised(), dfa, halt=rt.DfaHalt.Accept)]
    A, Bn, V, prompts, first = start_pair(name, quant)
    tab = table(V)
    walker = Walker(tab, V)
    smp = armed_samplers(cfgs, prompts, first)
    arm(A, cfgs, smp, first, tab)
    ref = per_token(Bn, cfgs, smp, first, tab, walker, N)            # strings that do not match alter no draw: slot 2's tokens are known now
    words = [tab[x] for x in ref["toks"][2]]
    assert len(words) >= 2
    # a buffer that can never be sent (0xff) and is full when the halting token arrives: everything before it fits exactly, it does not
    full = b"\xff" + b"x" * (rt.GEN_STOP_BUF - sum(len(w) for w in words))
    m = H.StopMatcher([b"zz"], full, cap=rt.GEN_STOP_BUF)
    assert [int(m.advance(w)[0]) for w in words] == [0] * (len(words) - 1) + [Fin.Handback]       # without the halt the device hands back
    A.gen_set_stops(2, [b"zz"], tail=full)
    t, p, ne, fin = A.gen_run(N)
    check(A, ref, t, p, ne, fin)
    assert ref["fin"] == [Fin.Stop] * 3
    text = [b"".join(tab[x] for x in ref["toks"][b]) for b in range(3)]
    assert text[0].count(b";") == 1 and text[1].count(b";") == 3 and text[2].count(b";") == 1
    assert A.gen_stop_tail(2) == full + b"".join(words[:-1])          # a slot that finishes leaves its buffer as it was before its last token
    A.close()
    Bn.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_the_first_draw_of_a_prompt_is_masked_in_a_mixed_step(name, quant):
    """Slot 0 decodes under a constraint while slot 1 is admitted with an 11-token prompt (two mixed steps: 7 + 4 tokens next to slot 0's
    row); slot 1's first draw, in the second mixed step, is masked with the start state."""
    A, Bn = GS.build(name, quant), GS.build(name, quant)
    V = A.info.num_vocab
    tab = table(V)
    walker = Walker(tab, V)
    dfa = rt.Dfa.compile(LOOP)
    p0, p1 = GS.prompt(V, 61, 5), GS.prompt(V, 62, 11)
    first = []
    for eng in (A, Bn):
        inp = rt.RnnInput([rt.RnnInputBatch(list(p0)), rt.RnnInputBatch(), rt.RnnInputBatch()])
        while inp.num_token() > 0:
            inp, outs = eng.infer(inp)
        first.append(int(np.argmax(outs[0][-1])))
    assert first[0] == first[1]
    s0, s1 = penalised(), H.TypicalSampler(tau=0.9, top_k=32)
    s0.init(p0)
    s0.update(first[0])
    s1.init(p1)
    A.gen_set_token_bytes(tab)
    A.gen_arm(0, first[0], N, copy.deepcopy(s0), seed=SEED)
    A.gen_arm_prompt(1, p1, N, copy.deepcopy(s1), seed=SEED)
    A.gen_set_constraint(0, dfa)
    A.gen_set_constraint(1, dfa)                                       # state defaults to the start state
    n = 10
    t, p, ne, fin = A.gen_run(n)
    c0, c1 = Constraint(dfa, walker), Constraint(dfa, walker)
    cur, left, draws1 = [first[0], None], list(p1), 0
    want = {0: [], 1: []}
    for d in range(n):
        s0.allow, s1.allow = c0.mask(), c1.mask()
        inp = rt.RnnInput([rt.RnnInputBatch([cur[0]]), rt.RnnInputBatch(list(left) if left else [cur[1]]), rt.RnnInputBatch()])
        inp, res = Bn.infer_sample(inp, [s0, s1, None], [rt.gen_uniform(SEED, 0, d), rt.gen_uniform(SEED, 1, draws1), 0.0])
        left = list(inp.batches[1].tokens) if left else []
        for b, s, c in ((0, s0, c0), (1, s1, c1)):
            if res[b] is None:
                want[b].append(None)
                continue
            tok, prob = res[b]
            s.update(tok)
            assert c.update(tok) is False and tok != 0
            cur[b] = tok
            want[b].append((tok, prob))
            draws1 += b
    assert want[1][0] is None and want[1][1] is not None and not left      # 7 + 4: the first draw is in the second mixed step
    for b in (0, 1):
        got = [(int(t[d, b]), float(p[d, b])) if t[d, b] != PAD else None for d in range(n)]
        print("slot", b, "want", want[b], "got", got)
        assert [g and g[0] for g in got] == [w and w[0] for w in want[b]]
        np.testing.assert_array_equal(bits([g[1] for g in got if g]), bits([w[1] for w in want[b] if w]))
        np.testing.assert_array_equal(A.state.back(b), Bn.state.back(b))
    assert A.gen_constraint_state(0) == c0.q and A.gen_constraint_state(1) == c1.q and list(ne[:2]) == [n, n - 1] and list(fin) == [0, 0, 0]
    m = walker.ends(c1.trans, dfa.start)
    forbidden = [i for i, w in enumerate(tab) if not w or b"d" in w or len(w) > 7] + list(range(len(tab), V))
    assert m[want[1][1][0]] != 0 and not m[forbidden].any() and len(forbidden) > 100     # the first draw is a token the start state allows
    A.close()
    Bn.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_the_state_carries_over_between_runs_and_to_the_per_token_path(name, quant):
    """Runs of 4, 9 and 10 steps, the constraint state read back after each; then the request goes on per token ON ENGINE A with
    `harness.DfaFormatter` (whose mask is rwkv_dfa_allow) started from `gen_constraint_state`, the samplers replayed over what A emitted,
    and emits what B emits for the remaining 9 steps."""
    dfa = rt.Dfa.compile(LOOP)
    cfgs = [Cfg(penalised(), dfa, max_tokens=99), Cfg(H.NucleusSampler(), rt.Dfa.compile(rb"[abc;]*"), max_tokens=99), Cfg(H.TypicalSampler(tau=0.9, top_k=32), dfa, halt=rt.DfaHalt.Final, max_tokens=99)]
    A, Bn, V, prompts, first = start_pair(name, quant)
    tab = table(V)
    walker = Walker(tab, V)
    smp = armed_samplers(cfgs, prompts, first)
    arm(A, cfgs, smp, first, tab)
    host = copy.deepcopy(smp)                                          # the caller's own samplers, replayed over A's output
    done, ref, last = 0, None, list(first)
    for steps in (4, 9, 10):
        t, p, ne, fin = A.gen_run(steps)
        ref = per_token(Bn, cfgs, smp, first, tab, walker, steps, d0=done, **({} if ref is None else {k: ref[k] for k in ("cons", "matchers", "cur", "emitted")}))
        check(A, ref, t, p, ne, fin)
        for b in range(3):
            for x in t[:, b]:
                host[b].update(int(x))
            last[b] = int(t[-1, b])
        done += steps
    fms = [H.DfaFormatter(cfgs[b].dfa, tab, V, state=A.gen_constraint_state(b)) for b in range(3)]
    ref = per_token(Bn, cfgs, smp, first, tab, walker, N - done, d0=done, **{k: ref[k] for k in ("cons", "matchers", "cur", "emitted")})
    for i, d in enumerate(range(done, N)):
        for b in range(3):
            host[b].allow = fms[b].transform() if fms[b] else None
        _, res = A.infer_sample(rt.RnnInput([rt.RnnInputBatch([last[b]]) for b in range(3)]), host, [rt.gen_uniform(SEED, b, d) for b in range(3)])
        for b in range(3):
            tok, prob = res[b]
            assert tok == ref["toks"][b][i] and bits(prob) == bits(ref["probs"][b][i]), (d, b)
            host[b].update(tok)
            last[b] = tok
            if fms[b]:
                assert fms[b].update(tok) is False
    assert [f.state if f else 0 for f in fms] == ref["q"]
    A.close()
    Bn.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_state_ids_above_255(name, quant):
    """rwkv_dfa_from_table with 512 states that count DOWN from 511, one per letter: every state the run visits before byte 256 needs the
    high byte (the 256-byte token may be drawn too).  Slot 2 takes a compiled table instead."""
    trans = np.zeros((512, 256), np.uint16)
    for q in range(2, 512):
        trans[q, [97, 98, 99]] = q - 1
    down = rt.Dfa.from_table(trans, np.ones(512, np.uint8) * (np.arange(512) > 0), start=511)
    assert down.num_states == 512 and down.start == 511
    cfgs = [Cfg(penalised(), down), Cfg(H.NucleusSampler(), down), Cfg(H.TypicalSampler(tau=0.9, top_k=32), rt.Dfa.compile(rb"[abc]{0,150}[abc]{0,150}"))]
    ref, t, p = run_case(name, quant, cfgs)
    tab = table(1024)
    for b in (0, 1):
        n_bytes = [len(tab[x]) for x in ref["toks"][b]]
        print("slot", b, "states", [511 - sum(n_bytes[:k]) for k in range(len(n_bytes) + 1)])
        assert ref["q"][b] == 511 - sum(n_bytes) and ref["fin"][b] == Fin.Length and 511 - n_bytes[0] > 255


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant", MODELS)
def test_constrained_slots_that_take_the_wide_kernel(name, quant):
    """Slot 0: Mirostat with target 4.5 (4 * target >= 13: the wide kernel for its whole life) under a constraint.  Slot 1: Nucleus with
    top_k = 512, armed with RWKV_GEN_WIDE_TOP_K.  Slot 2: narrow, constrained."""
    dfa = rt.Dfa.compile(GROUPS)
    cfgs = [Cfg(H.MirostatSampler(tau=4.5, rate=0.1), dfa), Cfg(H.NucleusSampler(top_p=0.9, top_k=512, temperature=1.1), dfa, wide=True), Cfg(H.NucleusSampler(), dfa)]
    ref, _, _ = run_case(name, quant, cfgs)
    assert all(f in (Fin.Stop, Fin.Length) for f in ref["fin"])


# ---- 10 --------------------------------------------------------------------------------------------------------------------------------
def test_the_refusals_and_what_clears_a_constraint():
    name, quant = MODELS[0]
    A = GS.build(name, quant)
    V = A.info.num_vocab
    tab = table(V)
    dfa = rt.Dfa.compile(GROUPS)

    def code(fn):
        with pytest.raises(rt.RwkvError) as e:
            fn()
        return e.value.code
    assert code(lambda: A.gen_set_constraint(0, dfa)) == -1             # nothing armed yet
    smp = H.NucleusSampler()
    A.gen_arm(0, 5, 8, smp, seed=SEED)
    assert code(lambda: A.gen_set_constraint(0, dfa)) == -1             # no token table
    A.gen_set_token_bytes(tab)
    assert code(lambda: A.gen_set_constraint(1, dfa)) == -1             # slot 1 is not armed
    assert code(lambda: A.gen_constraint_state(1)) == -1
    assert code(lambda: A.gen_set_constraint(0, dfa, state=0)) == -1    # the dead state
    assert code(lambda: A.gen_set_constraint(0, dfa, state=dfa.num_states)) == -1
    assert code(lambda: A.gen_set_constraint(0, dfa, halt=2)) == -1
    assert code(lambda: A.gen_arm(1, 5, 8, smp, allow=np.ones(V, np.uint8))) == -3      # a host mask stays refused
    assert code(lambda: A.gen_set_constraint(0, rt.Dfa.compile(rb"ax"))) == -3          # liveness: behind `a` only `x` leads on, and no token is `x`
    assert A.gen_constraint_state(0) == 0
    A.gen_set_constraint(0, dfa, state=dfa.walk(1, b"ab"))
    assert A.gen_constraint_state(0) == dfa.walk(1, b"ab")
    assert code(lambda: A.gen_set_token_bytes(tab)) == -1               # a slot walks the table
    A.gen_set_constraint(0, None)                                       # NULL clears it
    assert A.gen_constraint_state(0) == 0
    A.gen_set_token_bytes(tab)
    A.gen_set_constraint(0, dfa)
    A.gen_arm(0, 5, 8, smp, seed=SEED)                                  # re-arming clears it
    assert A.gen_constraint_state(0) == 0
    A.gen_set_token_bytes(tab)
    A.gen_set_constraint(0, dfa)
    A.gen_disarm(0)                                                     # ... and so does what disarms the slot
    A.gen_set_token_bytes(tab)
    A.gen_arm(0, 5, 8, smp, seed=SEED)
    A.gen_set_constraint(0, dfa)
    t, _, ne, fin = A.gen_run(8)
    assert ne[0] >= 1 and fin[0] in (Fin.Length, Fin.Stop) and A.gen_constraint_state(0) != 0
    assert code(lambda: A.gen_set_constraint(0, dfa)) == -1             # a finished slot
    A.close()

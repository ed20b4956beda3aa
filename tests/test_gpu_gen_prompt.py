"""MI355X: admission into resident generation (rwkv_gen_arm_prompt, ABI 9) against the per-token path that exists since ABI 8.

Engine A is armed with PROMPTS and generates on the device: the prompt rides in the resident steps next to the decode rows of the
running slots, the first token is drawn on the device with draw 0 of (seed, stream).  Engine B is the reference sequence: prefill
with `infer_sample` (adjustments from the host sampler after `init`, uniform `gen_uniform(seed, stream, 0)`), update the host
sampler, continue token by token with draws 1, 2, ...  Token ids, `out_probs` bit patterns and state slabs (`state.back`) are compared
with no tolerance.

Two references.  A slot that is alone in the engine takes the same steps on both sides (the prompt in chunks of token_chunk_size, then
single-token steps), so `reference()` — the plain per-token sequence — is exact for it.  With several slots in a step the project's
chunking invariant holds to 2e-5 only across different step shapes (tests/test_gpu_parity.py: bit-exact for the same T whatever the
neighbours hold, 2e-5 across T), and a 1-row step and the same row inside an 8-row mixed step did differ in the last bits of a
probability on the MI355X.  Those cases (admission under load, first-draw stop next to another slot, the three-slot edge cases) use
`lockstep()`: the same per-token calls (`infer_sample`, host samplers, `gen_uniform`), issued with the rows the resident steps carry —
one token per running slot, the rest of the chunk water-filled over the prompts (`rwkv_plan_chunk`'s split, which `infer_sample`
applies itself), a finished slot riding as the resident loop lets it ride.  That reference is exact by construction."""
import copy

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF
SEED = 20251101
CHUNK = 8


def build_pair(name, B, quant=(0, 0), chunk=CHUNK):
    st = R.st_serialize(R.synth_named(name))
    mk = lambda: rt.ModelBuilder(st).quant(quant[0], rt.Quant(quant[1])).build(max_batch=B, token_chunk_size=chunk, precision=rt.Precision.Fp16)
    return mk(), mk()


def prompt(V, slot, n):
    return [t % V for t in R.synth_prompt(slot, n)]


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def is_miro(s):
    return getattr(s, "kind", 0) == 2


def make_sampler(kind):
    if kind == "nucleus":
        return H.NucleusSampler(top_p=0.8, top_k=32, temperature=1.2, presence_penalty=0.3, frequency_penalty=0.4, penalty_decay=0.99)
    if kind == "typical":
        return H.TypicalSampler(tau=0.9, top_k=32, temperature=1.2, presence_penalty=0.2, frequency_penalty=0.4)
    return H.MirostatSampler(tau=2.0, rate=0.3)


def reference(eng, slot, toks, smp, n, stream=None, states=None):
    """The per-token sequence of today for one slot: prefill `toks` with infer_sample (draw 0 on the prompt's last row), update the host
    sampler `smp` (handed in right after init), then n - 1 single-token calls with draws 1, 2, ...  Returns [(token, prob)] * n;
    states[d] is the slab after the call that made draw d (d = 0: the prompt alone)."""
    B = eng.max_batch
    stream = slot if stream is None else stream
    only = lambda x, other: [x if b == slot else other for b in range(B)]
    out = []
    inp = rt.RnnInput([rt.RnnInputBatch(list(toks) if b == slot else []) for b in range(B)])
    for d in range(n):
        u = rt.gen_uniform(SEED, stream, d)
        res = None
        while inp.num_token() > 0:
            inp, r = eng.infer_sample(inp, only(smp, None), only(u, 0.0))
            res = r[slot] if r[slot] is not None else res
        tok, prob = res
        smp.update(prob if is_miro(smp) else tok)
        out.append((tok, prob))
        if states is not None:
            states[d] = eng.state.back(slot)
        inp = rt.RnnInput([rt.RnnInputBatch([tok] if b == slot else []) for b in range(B)])
    return out


class Job:
    """one slot of the lock-step reference: `pending` is the prompt tail or, once decoding, the one token it consumes next.  A slot that
    comes with a past — armed from an item, whose first draw was made from the item's row — starts at draw `draws` with `emitted`, the
    (token, prob) pairs it has already put out; `smp` has seen them."""

    def __init__(self, pending, smp, n, stream, in_prompt, stops=(), draws=0, emitted=()):
        self.pending, self.smp, self.n, self.stream, self.in_prompt, self.stops = list(pending), smp, n, stream, in_prompt, set(stops)
        self.draws, self.out, self.fin, self.fin_seen, self.state = int(draws), list(emitted), 0, False, None


def lockstep(eng, jobs, steps, pseudo=(), rows=None):
    """`steps` resident steps restated with per-token calls: which slots are in a step is decided as rwkv_gen_run decides it (from
    what the HOST knows: prompts pending, max_tokens less what was emitted for certain; who finished is learnt when the run ends).
    Returns (tokens, probs) shaped like gen_run's; jobs[b].state is the slab the state rule promises for slot b.
    `pseudo`: slots armed from an item (rwkv_gen_arm_item).  Their first draw — the last entry of the Job's `emitted`, not restated
    here — is made in the first step of this call from a row that no forward pass computes: it takes one row of the chunk all the
    same, so the prompts of that step share what is left, and the slot decodes from the step behind it.
    `rows` (a list) receives per step (step rows + rows spoken for, decode rows among them)."""
    B = eng.max_batch
    T = np.full((steps, B), PAD, np.uint32)
    P = np.full((steps, B), np.nan, np.float32)
    live = [b for b in sorted(jobs) if not jobs[b].fin_seen]
    remain = {b: jobs[b].n - len(jobs[b].out) for b in live}
    pseudo = [b for b in pseudo if b in live]

    def one_step(k, slots, reserve=0):
        pend = {b: list(jobs[b].pending) for b in slots}
        cut = set()
        if reserve:
            # infer_sample splits the whole chunk; with rows spoken for the split is made here (rwkv_plan_chunk over the smaller budget)
            # and every slot is handed its share alone.  A share that is not the whole prompt looks like one to infer_sample: the row it
            # draws for it is nobody's (one more row under the head, the forward pass has the step's rows)
            take = rt.plan_chunk([len(pend.get(b, ())) for b in range(B)], eng.token_chunk_size - reserve)
            cut = {b for b in slots if take[b] < len(pend[b])}
            given = {b: pend[b][:take[b]] for b in slots}
        else:
            given = pend
        inp = rt.RnnInput([rt.RnnInputBatch(list(given[b]) if b in slots else []) for b in range(B)])
        us = [rt.gen_uniform(SEED, jobs[b].stream, jobs[b].draws) if b in slots else 0.0 for b in range(B)]
        inp, res = eng.infer_sample(inp, [jobs[b].smp if b in slots else None for b in range(B)], us)
        if rows is not None:
            rows.append((sum(len(given[b]) - len(inp.batches[b].tokens) for b in slots) + reserve, sum(not jobs[b].in_prompt for b in slots)))
        for b in slots:
            j = jobs[b]
            if b in cut:
                assert not inp.batches[b].tokens
                j.pending = pend[b][len(given[b]):]
                continue
            if res[b] is None:
                j.pending = list(inp.batches[b].tokens)
                continue
            tok, prob = res[b]
            j.pending, j.in_prompt = [tok], False
            if j.fin:                                                  # a rider: its row is computed and thrown away
                continue
            T[k, b], P[k, b] = tok, prob
            j.smp.update(prob if is_miro(j.smp) else tok)
            j.out.append((tok, prob))
            j.draws += 1
            j.fin = 1 if (tok == 0 or tok in j.stops) else (2 if len(j.out) >= j.n else 0)
            if j.fin:
                j.state = eng.state.back(b)

    k = 0
    while k < steps:
        pro = [b for b in live if jobs[b].in_prompt]
        dec = [b for b in live if not jobs[b].in_prompt and remain[b] > 0 and b not in pseudo]
        if pro or pseudo:
            one_step(k, dec + pro, len(pseudo))
            for b in dec:
                remain[b] -= 1
            for b in pro:
                if not jobs[b].in_prompt:
                    remain[b] -= 1
            pseudo = []                                                # drew in this step; `remain` never counted that draw
            k += 1
        elif not dec:
            break
        else:
            n = min(max(remain[b] for b in dec), steps - k)
            for i in range(n):
                one_step(k + i, dec)
            for b in dec:
                remain[b] = max(0, remain[b] - n)
            k += n
    for b in live:
        if jobs[b].fin:
            jobs[b].fin_seen = True
        else:
            jobs[b].state = eng.state.back(b)
    return T, P


def check_lockstep(A, t, p, T, P, jobs):
    for b, j in jobs.items():
        print("slot", b, "want", T[:, b][T[:, b] != PAD].tolist(), "got", t[:, b][t[:, b] != PAD].tolist())
        np.testing.assert_array_equal(t[:, b], T[:, b])
        on = T[:, b] != PAD                                            # elsewhere: NaN, of whatever payload
        assert np.isnan(p[~on, b]).all()
        np.testing.assert_array_equal(bits(p[on, b]), bits(P[on, b]))
        np.testing.assert_array_equal(A.state.back(b), j.state)


def column(t, p, b):
    """the emitted (token, prob bits) of slot b in step order, and the step of the first one"""
    rows = np.nonzero(t[:, b] != PAD)[0]
    assert np.isnan(p[t[:, b] == PAD, b]).all() and not np.isnan(p[rows, b]).any()
    return t[rows, b], bits(p[rows, b]), (int(rows[0]) if len(rows) else None)


def check_slot(t, p, b, want):
    gt, gp, _ = column(t, p, b)
    wt = [x for x, _ in want]
    assert 0 not in wt[:-1], "token 0 would stop the resident side early: pick another prompt"
    print("slot", b, "want", wt, "got", gt.tolist())
    np.testing.assert_array_equal(gt, np.array(wt, np.uint32))
    np.testing.assert_array_equal(gp, bits([x for _, x in want]))


# ---- cases 1 and 2: one slot, a prompt that spans several steps; V6 / V5 / V7, then Typical and Mirostat ---------------------------
@pytest.mark.parametrize("name,kind", [("v6-tiny", "nucleus"), ("v5-tiny", "nucleus"), ("v7-tiny", "nucleus"),
                                       ("v6-tiny", "typical"), ("v6-tiny", "mirostat")])
def test_one_prompt_slot_equals_prefill_sample_then_the_per_token_loop(name, kind):
    A, Bn = build_pair(name, 2)
    V = A.info.num_vocab
    toks = prompt(V, 31, 2 * CHUNK + 5)                                # three steps: 8 + 8 + 5
    n = 10
    smp = make_sampler(kind)
    smp.init(toks)
    A.gen_arm_prompt(0, toks, n, copy.deepcopy(smp), seed=SEED)
    assert A.gen_prompt_left(0) == len(toks) and A.gen_prompt_left(1) == 0
    t, p, ne, fin = A.gen_run(16)
    assert A.gen_prompt_left(0) == 0
    states = {}
    want = reference(Bn, 0, toks, smp, n, states=states)
    check_slot(t, p, 0, want)
    first = column(t, p, 0)[2]
    assert first == 2, "the first token comes out of the step that exhausts the prompt"
    assert (t[:, 1] == PAD).all()
    assert list(ne) == [n, 0] and list(fin) == [rt.GenFinish.Length, 0]
    if kind == "mirostat":                                              # out_probs[0] is the surprise of the first draw, and max_surprise moved
        s0 = H.MirostatSampler(tau=2.0, rate=0.3)
        s0.update(want[0][1])
        assert s0.max_surprise != np.float32(4.0) and bits(p[first, 0]) == bits(want[0][1])
    np.testing.assert_array_equal(A.state.back(0), states[n - 1])       # consumed the prompt and all it emitted but the last token
    A.close()
    Bn.close()


# ---- case 3: admission under load ------------------------------------------------------------------------------------------------
def prefill_argmax(eng, prompts):
    inp = rt.RnnInput([rt.RnnInputBatch(list(q)) for q in prompts])
    first = [None] * len(prompts)
    while inp.num_token() > 0:
        inp, outs = eng.infer(inp)
        for b, o in enumerate(outs):
            if len(o):
                first[b] = int(np.argmax(o[-1]))
    return first


def test_admission_under_load():
    """Three slots run (one of them Mirostat); two prompts of different lengths are admitted between two runs.  The running slots'
    rows share steps of 8 rows with the prompts, so they are held to the lock-step reference (module docstring), not to a run nobody
    joined: across step shapes the engine promises 2e-5, not bits."""
    A, Bn = build_pair("v6-tiny", 5)
    V = A.info.num_vocab
    prompts = [prompt(V, 60 + b, 6 + 3 * b) if b < 3 else [] for b in range(5)]
    first = prefill_argmax(A, prompts)
    assert prefill_argmax(Bn, prompts) == first
    jobs = {}
    for b in range(3):
        s = make_sampler("nucleus" if b != 1 else "mirostat")
        s.init(prompts[b])
        if not is_miro(s):
            s.update(first[b])
        A.gen_arm(b, first[b], 64, copy.deepcopy(s), seed=SEED)
        jobs[b] = Job([first[b]], s, 64, b, False)
    ta1, pa1, _, _ = A.gen_run(4)
    T1, P1 = lockstep(Bn, jobs, 4)
    check_lockstep(A, ta1, pa1, T1, P1, jobs)
    n_join = 5
    for b, q, kind in [(3, prompt(V, 41, 19), "nucleus"), (4, prompt(V, 42, 7), "typical")]:
        s = make_sampler(kind)
        s.init(q)
        A.gen_arm_prompt(b, q, n_join, copy.deepcopy(s), seed=SEED)
        jobs[b] = Job(q, s, n_join, b, True)
    ta2, pa2, ne, fin = A.gen_run(16)
    T2, P2 = lockstep(Bn, jobs, 16)
    assert (T2[:, :3] != PAD).all(), "a running slot stopped: pick another prompt"
    check_lockstep(A, ta2, pa2, T2, P2, jobs)
    assert list(ne) == [16, 16, 16, n_join, n_join] and list(fin) == [0, 0, 0, rt.GenFinish.Length, rt.GenFinish.Length]
    assert (ta1[:, 3:] == PAD).all()
    # the short prompt is through first (water-filling shares the rows left after the three decode rows)
    assert column(ta2, pa2, 4)[2] < column(ta2, pa2, 3)[2]
    A.close()
    Bn.close()


@pytest.mark.parametrize("chunk,plen", [(64, 150), (256, 600)])
def test_admission_with_the_step_shapes_a_server_issues(chunk, plen):
    """Mixed steps of 64 rows (the chunked WKV form with more than 8 rows per sequence) and of 256 rows (above 192 the prefill GEMM
    family takes the step, sampled rows included), next to two running slots; the second prompt is short and joins the decode rows
    while the long one is still being consumed.  Lock-step reference, as in the case above."""
    A, Bn = build_pair("v6-tiny", 4, chunk=chunk)
    V = A.info.num_vocab
    prompts = [prompt(V, 70 + b, 5 + 2 * b) if b < 2 else [] for b in range(4)]
    first = prefill_argmax(A, prompts)
    assert prefill_argmax(Bn, prompts) == first
    jobs = {}
    for b in range(2):
        s = make_sampler("nucleus" if b == 0 else "typical")
        s.init(prompts[b])
        s.update(first[b])
        A.gen_arm(b, first[b], 64, copy.deepcopy(s), seed=SEED)
        jobs[b] = Job([first[b]], s, 64, b, False)
    ta1, pa1, _, _ = A.gen_run(3)
    T1, P1 = lockstep(Bn, jobs, 3)
    check_lockstep(A, ta1, pa1, T1, P1, jobs)
    n_join = 4
    for b, q, kind in [(2, prompt(V, 43, plen), "nucleus"), (3, prompt(V, 44, 9), "mirostat")]:
        s = make_sampler(kind)
        s.init(q)
        A.gen_arm_prompt(b, q, n_join, copy.deepcopy(s), seed=SEED)
        jobs[b] = Job(q, s, n_join, b, True)
    ta2, pa2, ne, fin = A.gen_run(10)
    T2, P2 = lockstep(Bn, jobs, 10)
    assert (T2[:, :2] != PAD).all(), "a running slot stopped: pick another prompt"
    check_lockstep(A, ta2, pa2, T2, P2, jobs)
    assert list(ne) == [10, 10, n_join, n_join] and list(fin) == [0, 0, rt.GenFinish.Length, rt.GenFinish.Length]
    assert column(ta2, pa2, 3)[2] == 0 and column(ta2, pa2, 2)[2] >= 2   # the long prompt takes at least three steps
    A.close()
    Bn.close()


# ---- case 4: the slot finishes on its first draw ------------------------------------------------------------------------------------
def test_first_draw_finishes_the_slot_with_the_state_of_the_prompt_alone():
    A, Bn = build_pair("v6-tiny", 3)
    V = A.info.num_vocab
    toks = prompt(V, 33, CHUNK + 3)
    smp = make_sampler("nucleus")
    smp.init(toks)
    states = {}
    want = reference(Bn, 0, toks, copy.deepcopy(smp), 1, stream=9, states=states)
    assert want[0][0] != 0
    # max_tokens == 1; the slot rides the steps behind its first draw and is put back
    A.gen_arm_prompt(0, toks, 1, copy.deepcopy(smp), seed=SEED, stream=9)
    t, p, ne, fin = A.gen_run(5)
    check_slot(t, p, 0, want)
    assert list(ne) == [1, 0, 0] and list(fin) == [rt.GenFinish.Length, 0, 0]
    np.testing.assert_array_equal(A.state.back(0), states[0])
    # the same draw on a fresh slot, now as a stop token learnt from the first pass, next to a slot that keeps running
    A.gen_arm_prompt(1, toks, 7, copy.deepcopy(smp), seed=SEED, stream=9, stop_tokens=[want[0][0]])
    other = prompt(V, 34, 4)
    s2 = make_sampler("nucleus")
    s2.init(other)
    A.gen_arm_prompt(2, other, 4, copy.deepcopy(s2), seed=SEED)
    t, p, ne, fin = A.gen_run(6)
    jobs = {1: Job(toks, copy.deepcopy(smp), 7, 9, True, stops=[want[0][0]]), 2: Job(other, s2, 4, 2, True)}
    Bn.state.load(Bn.state.init(), 0)
    T, P = lockstep(Bn, jobs, 6)
    check_lockstep(A, t, p, T, P, jobs)
    assert list(ne) == [0, 1, 4] and list(fin) == [rt.GenFinish.Length, rt.GenFinish.Stop, rt.GenFinish.Length]
    assert [x for x, _ in jobs[1].out] == [want[0][0]]                  # the same first draw, now a stop token
    # slot 1 shared its steps with slot 2, so its state after the prompt alone is the lock-step one; against the solitary prefill it
    # agrees to the engine's cross-shape bound
    assert np.abs(A.state.back(1) - states[0]).max() <= 2e-5 * max(1.0, float(np.abs(states[0]).max()))
    t, p, ne, fin = A.gen_run(2)                                        # everything finished: nothing moves
    assert (t == PAD).all() and list(ne) == [0, 0, 0]
    A.close()
    Bn.close()


# ---- case 5: chunk boundary, one-token prompt, non-zero starting state ----------------------------------------------------------------
def test_chunk_boundary_one_token_prompt_and_a_loaded_state():
    A, Bn = build_pair("v6-tiny", 3)
    V = A.info.num_vocab
    prefill_argmax(A, [[], [], prompt(V, 35, 11)])
    slab = A.state.back(2)                                              # an earlier slab: a prefix-cache hit, say
    assert np.abs(slab).max() > 0
    A.state.load(slab, 2)
    Bn.state.load(slab, 2)
    prompts = {0: prompt(V, 36, 2 * CHUNK), 1: prompt(V, 37, 1), 2: prompt(V, 38, 5)}
    n = 6
    jobs = {}
    for b, q in prompts.items():
        smp = make_sampler(["nucleus", "typical", "nucleus"][b])
        smp.init(q)
        A.gen_arm_prompt(b, q, n, copy.deepcopy(smp), seed=SEED)
        jobs[b] = Job(q, smp, n, b, True)
    t, p, ne, fin = A.gen_run(12)
    assert list(ne) == [n] * 3 and list(fin) == [rt.GenFinish.Length] * 3
    assert column(t, p, 1)[2] == 0, "a one-token prompt emits in the very first step"
    assert column(t, p, 0)[2] > 0 and all(0 not in [x for x, _ in j.out][:-1] for j in jobs.values())
    T, P = lockstep(Bn, jobs, 12)
    check_lockstep(A, t, p, T, P, jobs)
    A.close()
    Bn.close()


# ---- case 6: disarm rules and refusals ---------------------------------------------------------------------------------------------
def test_disarm_rules_and_refusals():
    A, Bn = build_pair("v6-tiny", 3)
    Bn.close()
    V = A.info.num_vocab
    toks = prompt(V, 39, 20)
    smp = make_sampler("nucleus")
    smp.init(toks)
    A.gen_arm_prompt(0, toks, 5, smp, seed=SEED)
    A.gen_arm_prompt(1, toks, 5, smp, seed=SEED)
    A.gen_arm_prompt(2, toks, 5, smp, seed=SEED)
    t, _, ne, fin = A.gen_run(1)
    assert (t == PAD).all() and list(ne) == [0, 0, 0] and list(fin) == [0, 0, 0]
    left = [A.gen_prompt_left(b) for b in range(3)]
    assert all(0 < x < 20 for x in left) and sum(left) == 60 - CHUNK
    prefill_argmax(A, [[3, 4], [], []])                                 # rwkv_infer with tokens for a slot in mid-prompt drops the prompt
    A.state.load(A.state.back(1), 1)                                    # ... and so does rwkv_state_load
    A.gen_disarm(2)
    assert [A.gen_prompt_left(b) for b in range(3)] == [0, 0, 0]
    A.gen_arm_prompt(2, toks, 5, smp, seed=SEED)
    A.state.write(A.state.read(1), 2)                                   # ... and rwkv_state_write
    assert A.gen_prompt_left(2) == 0
    t, _, ne, fin = A.gen_run(4)                                        # no slot is armed any more
    assert (t == PAD).all() and list(ne) == [0, 0, 0] and list(fin) == [0, 0, 0]
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm_prompt(0, [], 5, smp)                                 # n_tokens == 0 / tokens == NULL
    assert e.value.code == -1
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm_prompt(0, [1, V], 5, smp)
    assert e.value.code == -1
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm_prompt(0, toks, 0, smp)
    assert e.value.code == -1
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm_prompt(0, toks, 5, smp, allow=np.ones(V, np.uint8))
    assert e.value.code == -3
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm_prompt(0, toks, 5, H.NucleusSampler(top_k=300))
    assert e.value.code == -3
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm_prompt(0, toks, 5, smp, stop_tokens=list(range(1, 10)))
    assert e.value.code == -3
    assert A.gen_prompt_left(0) == 0 and (A.gen_run(1)[0] == PAD).all()  # a refused arm arms nothing
    A.close()


def test_more_live_slots_than_a_chunk_is_refused_before_any_step_runs():
    """A throw from the middle of an enqueue would lose the tokens of the steps already run: the run is refused up front, and goes
    through once a slot has been disarmed."""
    st = R.st_serialize(R.synth_named("v6-tiny"))
    A = rt.ModelBuilder(st).build(max_batch=5, token_chunk_size=4, precision=rt.Precision.Fp16)
    V = A.info.num_vocab
    smp = make_sampler("nucleus")
    for b in range(4):
        A.gen_arm(b, 5 + b, 8, smp, seed=SEED)
    A.gen_arm_prompt(4, prompt(V, 45, 6), 8, smp, seed=SEED)
    with pytest.raises(rt.RwkvError) as e:
        A.gen_run(4)
    assert e.value.code == -1 and A.gen_prompt_left(4) == 6              # nothing ran
    A.gen_disarm(3)
    t, _, ne, _ = A.gen_run(4)
    assert list(ne[:3]) == [4, 4, 4] and A.gen_prompt_left(4) == 2 and (t[:, 4] == PAD).all()
    A.close()


def test_vocabulary_above_65536_is_refused():
    st = R.st_serialize(R.synth_checkpoint(6, 1, 128, 448, 65536 + 16))
    A = rt.ModelBuilder(st).build(max_batch=1, token_chunk_size=8, precision=rt.Precision.Fp16)
    smp = make_sampler("nucleus")
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm_prompt(0, [1, 2, 3], 5, smp)
    assert e.value.code == -3 and A.gen_prompt_left(0) == 0
    A.close()


# ---- case 7: the prompt straddles two rwkv_gen_run calls ----------------------------------------------------------------------------
def test_prompt_straddles_two_runs():
    A, Bn = build_pair("v6-tiny", 2)
    V = A.info.num_vocab
    toks = prompt(V, 40, 2 * CHUNK + 5)
    n = 6
    smp = make_sampler("nucleus")
    smp.init(toks)
    A.gen_arm_prompt(1, toks, n, copy.deepcopy(smp), seed=SEED)
    t1, p1, ne, fin = A.gen_run(2)
    assert (t1 == PAD).all() and list(ne) == [0, 0] and list(fin) == [0, 0] and A.gen_prompt_left(1) == 5
    t2, p2, ne, fin = A.gen_run(3)                                      # the last 5 prompt tokens + first draw, then two more tokens
    assert list(ne) == [0, 3] and list(fin) == [0, 0]
    t3, p3, ne, fin = A.gen_run(8)
    assert list(ne) == [0, 3] and list(fin) == [0, rt.GenFinish.Length]
    states = {}
    want = reference(Bn, 1, toks, smp, n, states=states)
    check_slot(np.concatenate([t1, t2, t3]), np.concatenate([p1, p2, p3]), 1, want)
    np.testing.assert_array_equal(A.state.back(1), states[n - 1])
    A.close()
    Bn.close()

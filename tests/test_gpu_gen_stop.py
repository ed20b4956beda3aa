"""MI355X: stop STRINGS matched on the device inside the resident step (rwkv_gen_set_token_bytes / _set_stops / _stop_tail) against the
per-token path with the host matcher.

Engine A is resident and carries the strings.  Engine B runs the per-token loop of tests/test_gpu_generate.py (`infer_sample`, host
samplers, `gen_uniform`) once per model — strings do not alter a draw before the stop, so one realised sequence serves every case — and
`harness.StopMatcher` over the bytes of B's tokens says where the request stops, what its buffer holds after every token, and which state
the stop leaves (B's slab after all but the last emitted token).  The token table is synthetic: ids map to 1-5 bytes over a three-letter
alphabet plus halves of multi-byte characters, and a case overrides the bytes of the ids it needs, so that a match lands on a chosen token.
Nothing is compared with a tolerance: ids, `out_probs` bits, n_emitted, finish, `gen_stop_tail` bytes, `state.back`.

Within one rwkv_gen_run a finished slot rides along, so every step keeps B's three rows; cases that use several runs finish in the last one."""
import copy

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import test_gpu_gen_prompt as GP

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF
MODELS = [("v6-small", (3, 1)), ("v7-small", (3, 2))]          # Int8 / NF4 on every layer, default precision
SEED = 20251110
N = 32
Fin = rt.GenFinish


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def build(name, quant, B=3):
    st = R.st_serialize(R.synth_named(name))
    return rt.ModelBuilder(st).quant(quant[0], rt.Quant(quant[1])).build(max_batch=B, token_chunk_size=8, precision=rt.Precision.Fp16)


def prompt(V, slot, n):
    return [t % V for t in R.synth_prompt(slot, n)]


def prefill(eng, prompts):
    inp = rt.RnnInput([rt.RnnInputBatch(list(p)) for p in prompts])
    first = [None] * len(prompts)
    while inp.num_token() > 0:
        inp, outs = eng.infer(inp)
        for b, o in enumerate(outs):
            if len(o):
                first[b] = int(np.argmax(o[-1]))
    return first


def samplers(prompts, first):
    smp = [H.NucleusSampler(top_p=0.8, top_k=32, temperature=1.2, frequency_penalty=0.4), H.NucleusSampler(), H.TypicalSampler(tau=0.9, top_k=32)]
    for b, s in enumerate(smp):
        s.init(prompts[b])
        s.update(first[b])
    return smp


_REF = {}
PROMPT_BASES = (80, 90, 100, 110, 120, 130)


def realise(name, quant, base):
    """N per-token steps of all three slots on a fresh engine, behind the prompts of `base`"""
    Bn = build(name, quant)
    V = Bn.info.num_vocab
    prompts = [prompt(V, base + b, 5 + 2 * b) for b in range(3)]
    first = prefill(Bn, prompts)
    smp = samplers(prompts, first)
    cur, toks, probs, states = list(first), {b: [] for b in range(3)}, {b: [] for b in range(3)}, {}
    for d in range(N):
        us = [rt.gen_uniform(SEED, b, d) for b in range(3)]
        _, res = Bn.infer_sample(rt.RnnInput([rt.RnnInputBatch([cur[b]]) for b in range(3)]), smp, us)
        for b in range(3):
            tok, prob = res[b]
            smp[b].update(tok)
            toks[b].append(tok)
            probs[b].append(prob)
            cur[b] = tok
            states[(b, d)] = Bn.state.back(b)
    Bn.close()
    return dict(V=V, prompts=prompts, first=first, toks=toks, probs=probs, states=states)


def reference(name, quant):
    """B's realised sequence, once per model.  tokens[b], probs[b], states[(b, d)] = slab after the step that made draw d (it has consumed
    first_token and the draws 0 .. d - 1).  Token 0 stops a slot whatever its strings are (run.rs:855), and the cases here place their
    stops themselves: the prompts are the first of PROMPT_BASES behind which no slot draws it (and none starts from it)."""
    if name not in _REF:
        for base in PROMPT_BASES:
            ref = realise(name, quant, base)
            if all(0 not in ref["toks"][b] and ref["first"][b] != 0 for b in range(3)):
                break
            print(name, "prompts", base, "draw token 0: next prompts")
        else:
            raise AssertionError("every prompt set draws token 0: extend PROMPT_BASES")
        for b in range(3):
            print(name, "prompts", base, "slot", b, ref["toks"][b])
        _REF[name] = ref
    return _REF[name]


def table(V, overrides=None, known=(), with_pieces=True):
    """ids -> bytes: seeded; 1-5 letters of `abc`, or a piece of a multi-byte character (its head, its rest, or a lone continuation byte),
    and about one id in 16 unknown — but never one of `known` (the realised tokens).  `overrides` wins."""
    rng = np.random.default_rng(77)
    pieces = ["中".encode()[:2], "中".encode()[2:] + b"a", "é".encode()[:1], "é".encode()[1:], b"\xf0\x9f", b"\x98\x80"]
    out = []
    for i in range(V):
        u = rng.random()
        word = bytes(rng.choice([97, 98, 99], int(rng.integers(1, 6))).tolist())
        piece = pieces[int(rng.integers(0, len(pieces)))]
        out.append(None if u < 0.06 and i not in known else piece if u < 0.25 and with_pieces else word)
    for k, v in (overrides or {}).items():
        out[k] = v
    return out


def arm_all(A, ref, max_tokens=N):
    smp = samplers(ref["prompts"], ref["first"])
    for b in range(3):
        A.gen_arm(b, ref["first"][b], max_tokens, smp[b], seed=SEED)


def resident(name, quant, ref, tab):
    A = build(name, quant)
    assert prefill(A, ref["prompts"]) == ref["first"]
    A.gen_set_token_bytes(tab)
    arm_all(A, ref)
    return A


def host_trace(tab, toks, stops, tail=b"", max_tokens=N):
    """harness.StopMatcher over B's tokens: (finish, index of the finishing token or None, [buffer after token i])"""
    m = H.StopMatcher(stops, tail, cap=rt.GEN_STOP_BUF)
    tails = []
    for i, t in enumerate(toks):
        fin, _ = m.advance(tab[t], stop_token=t == 0, at_max=i + 1 >= max_tokens)
        tails.append(m.tail())
        if fin:
            return fin, i, tails
    return 0, None, tails


def check_slot(A, ref, b, got_t, got_p, n_emit, n_before=0):
    """slot b emitted exactly B's tokens [n_before, n_before + n_emit) in this call, bit for bit, and nothing after them"""
    np.testing.assert_array_equal(got_t[:n_emit, b], np.array(ref["toks"][b][n_before:n_before + n_emit], np.uint32))
    np.testing.assert_array_equal(bits(got_p[:n_emit, b]), bits(ref["probs"][b][n_before:n_before + n_emit]))
    assert (got_t[n_emit:, b] == PAD).all() and np.isnan(got_p[n_emit:, b]).all()


def pick_stop(tab, toks, lo, hi):
    """a stop string cut out of the bytes of B's tokens so that the reference walk matches exactly at a token in [lo, hi) and the string
    spans at least two tokens"""
    words = [tab[t] for t in toks]
    for m in range(lo, hi):
        for back in (1, 2):
            for cut in range(len(words[m - back])):
                stop = words[m - back][cut:] + b"".join(words[m - back + 1:m + 1])
                if len(stop) >= 3 and host_trace(tab, toks, [stop])[:2] == (1, m):
                    return stop, m
    raise AssertionError("no stop string lands in the window: change the table seed")


@pytest.mark.parametrize("name,quant", MODELS)
def test_a_stop_string_ends_a_slot_in_the_middle_of_a_run(name, quant):
    """Slot 1 carries strings, slots 0 and 2 do not: slot 1 stops where the host matcher stops, with the state of the rule; the other two
    equal B (no strings anywhere) AND a resident run in which no slot had strings, bit for bit."""
    ref = reference(name, quant)
    tab = table(ref["V"], known=set(ref["toks"][1]))
    stop, m = pick_stop(tab, ref["toks"][1], 10, 22)
    print("stop", stop, "lands on token", m)
    A = resident(name, quant, ref, tab)
    A.gen_set_stops(1, [b"zzz", stop, b"zzzzzz"])
    t, p, ne, fin = A.gen_run(N)
    assert list(ne) == [N, m + 1, N] and list(fin) == [Fin.Length, Fin.Stop, Fin.Length]
    for b in range(3):
        check_slot(A, ref, b, t, p, int(ne[b]))
        np.testing.assert_array_equal(A.state.back(b), ref["states"][(b, int(ne[b]) - 1)])
    _, _, tails = host_trace(tab, ref["toks"][1], [b"zzz", stop, b"zzzzzz"])
    assert A.gen_stop_tail(1) == (tails[m - 1] if m else b"") and A.gen_stop_tail(0) == b""
    A0 = resident(name, quant, ref, tab)                              # nobody has strings: the <., false> kernels
    t0, p0, _, _ = A0.gen_run(N)
    for b in (0, 2):
        np.testing.assert_array_equal(t0[:, b], t[:, b])
        np.testing.assert_array_equal(bits(p0[:, b]), bits(p[:, b]))
    A.close()
    A0.close()


@pytest.mark.parametrize("name,quant", MODELS)
def test_the_buffer_carries_over_between_runs(name, quant):
    """Runs of 1, 5 and 18 steps; the match lands in the last one.  After every run the device's buffer is the host matcher's."""
    ref = reference(name, quant)
    tab = table(ref["V"], known=set(ref["toks"][1]) | set(ref["toks"][2]))
    stop, m = pick_stop(tab, ref["toks"][1], 8, 22)
    A = resident(name, quant, ref, tab)
    A.gen_set_stops(1, [stop])
    A.gen_set_stops(2, [b"zz"])                                      # never matches; slot 2's buffer holds what is not UTF-8 yet
    tr = {b: host_trace(tab, ref["toks"][b], s) for b, s in ((1, [stop]), (2, [b"zz"]))}
    assert tr[2][0] == Fin.Length
    done = 0
    for steps in (1, 5, 18):
        t, p, ne, fin = A.gen_run(steps)
        e1 = min(m + 1 - done, steps)
        assert list(ne) == [steps, e1, steps]
        for b in range(3):
            check_slot(A, ref, b, t, p, int(ne[b]), done)
        done += steps
        assert A.gen_stop_tail(1) == (tr[1][2][done - 1] if done <= m else tr[1][2][m - 1])
        assert A.gen_stop_tail(2) == tr[2][2][done - 1]
    assert list(fin) == [0, Fin.Stop, 0] and 6 <= m < 24
    np.testing.assert_array_equal(A.state.back(1), ref["states"][(1, m)])
    np.testing.assert_array_equal(A.state.back(0), ref["states"][(0, 23)])
    A.close()


@pytest.mark.parametrize("name,quant", MODELS)
def test_a_substring_the_reference_walk_misses_does_not_stop_the_slot(name, quant):
    ref = reference(name, quant)
    toks = ref["toks"][2]
    # the walk misses a string when a partial match that fails inside it swallows the string's first byte: tokens "xx" | "xy" give
    # "xxxy", over which "xxy" is compared x-x, x-x, x-y (mismatch, and that x is not retried as a start), y-x: never matched
    i = next(k for k in range(4, N - 2) if toks.count(toks[k]) == 1 and toks.count(toks[k + 1]) == 1)
    tab = table(ref["V"], {toks[i]: b"xx", toks[i + 1]: b"xy"}, known=set(toks))
    stream = b"".join(tab[t] for t in toks)
    fin, _, tails = host_trace(tab, toks, [b"xxy"])
    assert fin == Fin.Length and b"xxy" in stream                     # a substring search would stop at token i + 1
    A = resident(name, quant, ref, tab)
    A.gen_set_stops(2, [b"xxy"])
    t, p, ne, fin = A.gen_run(N)
    assert list(ne) == [N, N, N] and list(fin) == [Fin.Length] * 3
    for b in range(3):
        check_slot(A, ref, b, t, p, N)
    assert A.gen_stop_tail(2) == (tails[N - 2] if N > 1 else b"")
    A.close()


@pytest.mark.parametrize("name,quant", MODELS)
def test_a_split_character_is_held_back_then_released_and_an_unknown_id_stops(name, quant):
    ref = reference(name, quant)
    toks = ref["toks"][2]
    i = next(k for k in range(2, 8) if len({toks[k - 1], toks[k], toks[k + 1], toks[k + 2], toks[k + 3]}) == 5 and toks.count(toks[k + 3]) == 1)
    zhong = "中".encode()
    tab = table(ref["V"], {toks[i - 1]: b"ab", toks[i]: zhong[:2], toks[i + 1]: zhong[2:] + b"c", toks[i + 2]: b"b", toks[i + 3]: None}, known=set(toks),
                with_pieces=False)                                   # letters only: nothing older sits in the buffer when the character arrives
    A = resident(name, quant, ref, tab)
    A.gen_set_stops(2, [b"zz"])
    fin, at, tails = host_trace(tab, toks, [b"zz"])
    assert (fin, at) == (Fin.Stop, i + 3)                             # the id that is not in the vocabulary stops it
    assert (tails[i - 1], tails[i], tails[i + 1]) == (b"", zhong[:2], b"")   # held while the character is incomplete, released with its last byte
    for d in range(i + 3):
        t, p, ne, f = A.gen_run(1)                                    # the buffer after EVERY token
        assert list(ne) == [1, 1, 1] and list(f) == [0, 0, 0]
        assert A.gen_stop_tail(2) == tails[d], (d, tails[d])
    t, p, ne, f = A.gen_run(4)
    assert list(ne) == [4, 4, 1] and list(f) == [0, 0, Fin.Stop]
    assert int(t[0, 2]) == toks[i + 3] and A.gen_stop_tail(2) == tails[i + 2]
    np.testing.assert_array_equal(A.state.back(2), ref["states"][(2, i + 3)])
    A.close()


@pytest.mark.parametrize("name,quant", MODELS)
def test_handback_and_an_initial_tail(name, quant):
    ref = reference(name, quant)
    tab = table(ref["V"], known=set(ref["toks"][0]) | set(ref["toks"][1]))
    A = resident(name, quant, ref, tab)
    # slot 0: a buffer that can never be sent (0xff) and is almost full: the device cannot take the token that passes 512 bytes
    full = b"\xff" + b"x" * 505
    A.gen_set_stops(0, [b"zz"], tail=full)
    fin0, h, tails0 = host_trace(tab, ref["toks"][0], [b"zz"], tail=full)
    assert fin0 == Fin.Handback and 1 <= h < 8
    # slot 1: the caller matched "Q!" itself before arming; the string is completed by the first two tokens drawn on the device
    w = [tab[t] for t in ref["toks"][1][:2]]
    stop = b"Q!" + w[0] + w[1]
    assert host_trace(tab, ref["toks"][1], [stop], tail=b"Q!")[:2] == (Fin.Stop, 1) and host_trace(tab, ref["toks"][1], [stop])[0] != Fin.Stop
    A.gen_set_stops(1, [stop], tail=b"Q!")
    assert A.gen_stop_tail(0) == full and A.gen_stop_tail(1) == b"Q!"
    t, p, ne, fin = A.gen_run(16)
    assert list(ne) == [h + 1, 2, 16] and list(fin) == [Fin.Handback, Fin.Stop, 0]
    for b in range(3):
        check_slot(A, ref, b, t, p, int(ne[b]))
        np.testing.assert_array_equal(A.state.back(b), ref["states"][(b, int(ne[b]) - 1)])
    assert A.gen_stop_tail(0) == (tails0[h - 1] if h else full) and len(A.gen_stop_tail(0)) + len(tab[ref["toks"][0][h]]) > rt.GEN_STOP_BUF
    assert A.gen_stop_tail(1) == host_trace(tab, ref["toks"][1], [stop], tail=b"Q!")[2][0]
    A.close()


def test_prompt_slots_first_draw_and_a_match_inside_a_mixed_step():
    """rwkv_gen_arm_prompt with strings.  Reference: `lockstep()` of tests/test_gpu_gen_prompt.py, told to stop at the token the host
    matcher stops at (a token that occurs nowhere earlier in the slot's output).  Slot 0 decodes behind a 3-token prompt and matches a
    two-token string at its third draw, while slot 1 is still inside a 40-token prompt (every step so far was a mixed step); slot 2's
    string is the bytes of its first draw: it finishes having consumed exactly its prompt."""
    name, n = "v6-tiny", 12
    D, D2 = GP.build_pair(name, 3)                                     # discover the realised tokens (no strings)
    D2.close()
    V = D.info.num_vocab
    prompts = {0: prompt(V, 41, 3), 1: prompt(V, 42, 40), 2: prompt(V, 43, 11)}

    def jobs(stops):
        out = {}
        for b, pr in prompts.items():
            s = GP.make_sampler("nucleus")
            s.init(pr)
            out[b] = GP.Job(pr, s, n, b, True, stops.get(b, ()))
        return out
    j0 = jobs({})
    GP.lockstep(D, j0, 8)
    D.close()
    o0, o2 = [x for x, _ in j0[0].out], [x for x, _ in j0[2].out]
    assert len(o0) >= 3 and len(set(o0[:3])) == 3 and len(o2) >= 1 and 0 not in o0[:3] + o2[:1], "pick other prompts"
    assert j0[1].in_prompt or len(j0[1].out) <= 2
    tab = table(V, {o0[0]: b"x", o0[1]: b"<e", o0[2]: b"nd>", o2[0]: b"END"}, known=set(o0) | set(o2))
    if o2[0] in o0[:3]:
        pytest.fail("slot 2's first token collides with slot 0's: pick other prompts")
    A, Bn = GP.build_pair(name, 3)
    A.gen_set_token_bytes(tab)
    jb = jobs({0: {o0[2]}, 2: {o2[0]}})
    for b, pr in prompts.items():
        A.gen_arm_prompt(b, pr, n, copy.deepcopy(jb[b].smp), seed=GP.SEED)
    A.gen_set_stops(0, [b"zz", b"<end>"])
    A.gen_set_stops(2, [b"END"])
    t, p, ne, fin = A.gen_run(8)
    T, P = GP.lockstep(Bn, jb, 8)
    GP.check_lockstep(A, t, p, T, P, jb)
    assert list(ne)[0] == 3 and list(ne)[2] == 1 and fin[0] == Fin.Stop and fin[2] == Fin.Stop
    assert ne[1] <= 8 - 3 - 1                                          # slot 1 drew nothing before step 4: slot 0's match (step 2) was in a mixed step
    assert A.gen_stop_tail(0) == b"<e" and A.gen_stop_tail(2) == b""
    A.close()
    Bn.close()


def test_rearming_clears_the_strings_and_the_refusals():
    name, quant = MODELS[0]
    A = build(name, quant)
    V = A.info.num_vocab
    tab = table(V)
    with pytest.raises(rt.RwkvError) as e:
        A.gen_set_stops(0, [b"x"])                                    # nothing armed yet
    assert e.value.code == -1
    smp = H.NucleusSampler()
    A.gen_arm(0, 5, 8, smp, seed=SEED)
    with pytest.raises(rt.RwkvError) as e:
        A.gen_set_stops(0, [b"x"])                                    # no token table
    assert e.value.code == -1
    with pytest.raises(rt.RwkvError) as e:
        A.gen_set_token_bytes([b"a" * (rt.GEN_TOKEN_LEN + 1)])
    assert e.value.code == -3
    A.gen_set_token_bytes(tab)
    for bad, code in ((dict(stops=[b"x"] * 9), -3), (dict(stops=[b"x" * 129]), -3), (dict(stops=[b"x"], tail=b"y" * 513), -3)):
        with pytest.raises(rt.RwkvError) as e:
            A.gen_set_stops(0, **bad)
        assert e.value.code == code
    with pytest.raises(rt.RwkvError) as e:
        A.gen_set_stops(1, [b"x"])                                    # slot 1 is not armed
    assert e.value.code == -1
    with pytest.raises(rt.RwkvError) as e:
        A.gen_stop_tail(1)
    assert e.value.code == -1
    A.gen_set_stops(0, [b"x" * 128] * 8, tail=b"y" * 512)             # the limits themselves are fine
    A.gen_set_stops(0, [b"x"], tail=b"abc")
    assert A.gen_stop_tail(0) == b"abc"
    with pytest.raises(rt.RwkvError) as e:
        A.gen_set_token_bytes(tab)                                    # a slot matches against the table
    assert e.value.code == -1
    A.gen_arm(0, 5, 8, smp, seed=SEED)                                # re-arming clears strings and buffer
    assert A.gen_stop_tail(0) == b""
    A.gen_set_token_bytes(tab)
    A.gen_set_stops(0, [b"x"], tail=b"abc")
    A.gen_set_stops(0, [], tail=b"")                                  # n = 0 clears them
    assert A.gen_stop_tail(0) == b""
    A.gen_set_token_bytes(tab)
    t, _, ne, fin = A.gen_run(8)
    assert ne[0] >= 1 and fin[0] in (Fin.Length, Fin.Stop)
    with pytest.raises(rt.RwkvError) as e:
        A.gen_set_stops(0, [b"x"])                                    # a finished slot
    assert e.value.code == -1
    A.close()

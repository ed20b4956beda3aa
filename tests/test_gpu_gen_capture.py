"""MI355X: resident generation fills and uses the prefix cache (rwkv_gen_set_capture / _take_item / _item_* / _arm_item; gen_capture_kernel,
gen_inject_kernel) against what the engine already does without them.

An item is a (state, raw row) pair.  Its state is held against `state.back` of a twin engine that stops where the item was taken, its row
against the row `rwkv_infer` returns for the same tokens in steps of the same shape, and a slot armed from an item against the slot that
was armed with the prompt itself.  Every comparison is on bit patterns: ids as they are, floats through `view(np.uint32)`; no tolerance
anywhere.  Fixtures as in tests/test_gpu_gen_prompt.py: synthetic tiny checkpoints, token_chunk_size 8, its samplers."""
import copy

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import test_gpu_gen_prompt as GP
from tests import v4_ref
from tests.test_gpu_gen_pda import table

pytestmark = pytest.mark.gpu

PAD, SEED, CHUNK, bits, make_sampler = GP.PAD, GP.SEED, GP.CHUNK, GP.bits, GP.make_sampler
Cap, Fin = rt.GenCapture, rt.GenFinish
BOTH = Cap.Prompt | Cap.Finish
KINDS = ["nucleus", "typical", "mirostat"]
_ST = {}


def build(name, B, quant=(0, 0)):
    if name not in _ST:
        _ST[name] = R.st_serialize(v4_ref.synth_v4(name) if name.startswith("v4") else R.synth_named(name))
    return rt.ModelBuilder(_ST[name]).quant(quant[0], rt.Quant(quant[1])).build(max_batch=B, token_chunk_size=CHUNK, precision=rt.Precision.Fp16)


def prompt(V, slot, n):
    return [t % V for t in R.synth_prompt(slot, n)]


def sampler(kind, toks):
    s = make_sampler(kind)
    s.init(list(toks))
    return s


def code(f):
    with pytest.raises(rt.RwkvError) as e:
        f()
    return e.value.code


def last_row(eng, slot, toks):
    """the row rwkv_infer (`Last`) returns for `toks` on `slot`, in steps of token_chunk_size"""
    inp = rt.RnnInput([rt.RnnInputBatch(list(toks) if b == slot else []) for b in range(eng.max_batch)])
    row = None
    while inp.num_token() > 0:
        inp, outs = eng.infer(inp)
        if len(outs[slot]):
            row = np.array(outs[slot][-1], np.float32)
    return row


def emitted(t, p, b):
    on = t[:, b] != PAD
    return t[on, b].tolist(), bits(p[on, b]).tolist()


def same_run(a, b):
    """two results of gen_run (or gen_run with `top`) agree in everything: NaN payloads included, they come from the same memset"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def same_item(a, b):
    (sa, ra), (sb, rb) = a, b
    np.testing.assert_array_equal(bits(sa), bits(sb))
    np.testing.assert_array_equal(bits(ra), bits(rb))


# ---- the three-slot scene of tests 1 and 4 -------------------------------------------------------------------------------------------
SCENE_MAX = (10, 5, 8)


def scene(capture, stop, extras):
    """Slot 0 is armed with a prompt and decodes for one run; then slot 1 (19 tokens: three steps at chunk 8) and slot 2 (3 tokens) are
    admitted next to it.  Nucleus / Typical / Mirostat.  `stop`: slot 2's stop token.  `capture`: PROMPT | FINISH on every slot that
    admits it (slot 0 is decoding: FINISH alone).  `extras`: top-n lists of 32 places on every slot and a watch.
    Returns the engine and everything it showed."""
    eng = build("v6-tiny", 3)
    V = eng.info.num_vocab
    ps = [prompt(V, 41, 5), prompt(V, 42, 19), prompt(V, 43, 3)]
    top = 32 if extras else 0
    watch = eng.gen_watch_open(64) if extras else None
    runs = []
    eng.gen_arm_prompt(0, ps[0], SCENE_MAX[0], sampler(KINDS[0], ps[0]), seed=SEED)
    if extras:
        eng.gen_set_topn(0, top)
    runs.append(eng.gen_run(3, top=top))
    for b in (1, 2):
        eng.gen_arm_prompt(b, ps[b], SCENE_MAX[b], sampler(KINDS[b], ps[b]), seed=SEED, stop_tokens=[stop] if b == 2 and stop is not None else ())
        if extras:
            eng.gen_set_topn(b, top)
    if capture:
        eng.gen_set_capture(0, Cap.Finish)
        eng.gen_set_capture(1, BOTH)
        eng.gen_set_capture(2, BOTH)
    runs.append(eng.gen_run(6, top=top))
    runs.append(eng.gen_run(6, top=top))
    records = watch.read(64) if extras else None
    states = [eng.state.back(b) for b in range(3)]
    return eng, runs, records, states


_STOP = {}


def scene_stop():
    """discovery: the token slot 2 emits fourth when nothing stops it"""
    if "tok" not in _STOP:
        eng, runs, _, _ = scene(False, None, False)
        toks = [x for r in runs for x in emitted(r[0], r[1], 2)[0]]
        eng.close()
        assert len(toks) >= 4 and toks[3] not in toks[:3] and 0 not in toks[:4], f"slot 2 emits {toks}: pick another prompt"
        _STOP["tok"] = toks[3]
    return _STOP["tok"]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "topn+watch"])
def test_capture_is_invisible(extras):
    stop = scene_stop()
    A, ra, wa, sa = scene(True, stop, extras)
    Bn, rb, wb, sb = scene(False, stop, extras)
    for x, y in zip(ra, rb):
        print("tokens", x[0].T.tolist(), "finish", x[3].tolist())
        same_run(x, y)
    fin = ra[-1][3]
    assert int(fin[2]) == Fin.Stop and sum(int(r[2][2]) for r in ra) == 4, "slot 2 stops at its 4th token"
    assert int(fin[0]) and int(fin[1])
    for b in range(3):
        np.testing.assert_array_equal(bits(sa[b]), bits(sb[b]))
    if extras:
        same_run(wa[:3], wb[:3])
        assert wa[3] == wb[3] == 0 and len(wa[0]) >= 10
    for b, flags in ((0, [Cap.Finish]), (1, [Cap.Prompt, Cap.Finish]), (2, [Cap.Prompt, Cap.Finish])):
        for f in flags:
            A.gen_take_item(b, f).close()
    A.close()
    Bn.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant,lens", [("v6-tiny", (0, 0), (3, 8, 19)), ("v5-tiny", (0, 0), (19,)), ("v7-tiny", (0, 0), (19,)),
                                             ("v4-tiny", (0, 0), (19,)), ("v6-small", (3, 1), (19,))],   # Int8 needs C % 256 == 0: v6-small is the smallest V6 that loads
                         ids=["v6", "v5", "v7", "v4", "v6-int8"])
def test_prompt_item_of_a_slot_alone(name, quant, lens):
    A, T1, T2 = build(name, 1, quant), build(name, 1, quant), build(name, 1, quant)
    V = A.info.num_vocab
    init = A.state.init()
    for n in lens:
        P = prompt(V, 50 + n, n)
        for eng in (A, T1, T2):
            eng.state.load(init, 0)
        A.gen_arm_prompt(0, P, 4, sampler("nucleus", P), seed=SEED)
        A.gen_set_capture(0, Cap.Prompt)
        t, p, ne, fin = A.gen_run(8)
        assert int(ne[0]) >= 1
        item = A.gen_take_item(0, Cap.Prompt)                      # the slot has decoded three tokens past its prompt by now
        st, row = item.back()
        T1.gen_arm_prompt(0, P, 1, sampler("nucleus", P), seed=SEED)   # the base case of the STATE RULE: everything but the one emitted token
        T1.gen_run(8)
        np.testing.assert_array_equal(bits(st), bits(T1.state.back(0)))
        want = last_row(T2, 0, P)
        print(name, quant, "prompt of", n, "row[:4]", row[:4], "want", want[:4])
        np.testing.assert_array_equal(bits(row), bits(want))
        np.testing.assert_array_equal(bits(item.row()), bits(want))
        item.close()
    for eng in (A, T1, T2):
        eng.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_finish_item_of_a_slot_alone():
    A, T, D = build("v6-tiny", 1), build("v6-tiny", 1), build("v6-tiny", 1)
    V = A.info.num_vocab
    P = prompt(V, 61, 11)
    n = 4
    # discovery, and RWKV_GEN_LENGTH yields an item as well
    D.gen_arm_prompt(0, P, 8, sampler("nucleus", P), seed=SEED)
    D.gen_set_capture(0, Cap.Finish)
    t, p, ne, fin = D.gen_run(16)
    free = emitted(t, p, 0)[0]
    assert int(fin[0]) == Fin.Length and len(free) == 8
    assert free[n - 1] not in free[:n - 1] and 0 not in free[:n], f"{free}: pick another prompt"
    item = D.gen_take_item(0, Cap.Finish)
    np.testing.assert_array_equal(bits(item.back()[0]), bits(D.state.back(0)))
    length_row = item.row()
    item.close()
    stop = free[n - 1]
    # the slot stops at its 4th token and rides 8 more steps of the same run: the row is the finishing step's
    A.gen_arm_prompt(0, P, 12, sampler("nucleus", P), seed=SEED, stop_tokens=[stop])
    A.gen_set_capture(0, Cap.Finish)
    assert code(lambda: A.gen_take_item(0, Cap.Finish)) == -1
    t, p, ne, fin = A.gen_run(16)
    assert emitted(t, p, 0)[0] == free[:n] and int(fin[0]) == Fin.Stop
    item = A.gen_take_item(0, Cap.Finish)
    st, row = item.back()
    np.testing.assert_array_equal(bits(st), bits(A.state.back(0)))
    T.gen_arm_prompt(0, P, n - 1, sampler("nucleus", P), seed=SEED, stop_tokens=[stop])
    tt, tp, tne, tfin = T.gen_run(16)
    assert emitted(tt, tp, 0)[0] == free[:n - 1] and int(tfin[0]) == Fin.Length
    want = last_row(T, 0, [free[n - 2]])
    np.testing.assert_array_equal(bits(row), bits(want))
    np.testing.assert_array_equal(bits(st), bits(T.state.back(0)))
    assert not np.array_equal(bits(row), bits(length_row))
    item.close()
    # a slot that stops on its first draw: FINISH == PROMPT
    D.state.load(D.state.init(), 0)
    D.gen_arm_prompt(0, P, 8, sampler("nucleus", P), seed=SEED, stop_tokens=[free[0]])
    D.gen_set_capture(0, BOTH)
    t, p, ne, fin = D.gen_run(16)
    assert int(ne[0]) == 1 and int(fin[0]) == Fin.Stop
    ip, itf = D.gen_take_item(0, Cap.Prompt), D.gen_take_item(0, Cap.Finish)
    same_item(ip.back(), itf.back())
    for eng in (A, T, D):
        eng.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_items_next_to_neighbours_hold_the_rows_the_lists_were_made_of():
    stop = scene_stop()
    A, runs, _, _ = scene(True, stop, True)
    lists = {b: [] for b in range(3)}
    for t, p, ne, fin, tok_logp, ids, lp in runs:
        for k in range(t.shape[0]):
            for b in range(3):
                if t[k, b] != PAD:
                    lists[b].append((ids[k, b].copy(), lp[k, b].copy()))
    for b, flag, at in ((1, Cap.Prompt, 0), (2, Cap.Prompt, 0), (0, Cap.Finish, -1), (1, Cap.Finish, -1), (2, Cap.Finish, -1)):
        item = A.gen_take_item(b, flag)
        ids, lp = A.topn_rows([item.row()], 32)
        print("slot", b, flag.name, "ids", ids[0][:6].tolist(), "published", lists[b][at][0][:6].tolist())
        np.testing.assert_array_equal(ids[0], lists[b][at][0])
        np.testing.assert_array_equal(bits(lp[0]), bits(lists[b][at][1]))
        item.close()
    A.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def arm_from_item_case(kind, n, stops=None, pda=None):
    A, Bn = build("v6-tiny", 1), build("v6-tiny", 1)
    V = A.info.num_vocab
    P = prompt(V, 70 + n, n)
    tab = table(V) if (stops is not None or pda is not None) else None
    out = []
    for eng in (A, Bn):
        if tab is not None:
            eng.gen_set_token_bytes(tab)
        if eng is A:
            eng.gen_arm_prompt(0, P, 6, sampler(kind, P), seed=SEED)
            eng.gen_set_capture(0, Cap.Prompt)
        else:
            eng.gen_arm_item(0, item_b, 6, sampler(kind, P), seed=SEED)
            assert eng.gen_prompt_left(0) == 0
        if stops is not None:
            eng.gen_set_stops(0, stops)
        if pda is not None:
            eng.gen_set_pda(0, pda)
        t, p, ne, fin = eng.gen_run(10)
        out.append((emitted(t, p, 0), int(ne[0]), int(fin[0]), eng.state.back(0), eng.gen_pda_config(0), eng.gen_stop_tail(0), t))
        if eng is A:
            item = eng.gen_take_item(0, Cap.Prompt)
            item_b = rt.GenItem.from_host(Bn, *item.back())
            same_item(item.back(), item_b.back())
            item.close()
    a, b = out
    print(kind, n, "A", a[0][0], "B", b[0][0], "finish", a[2], b[2])
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[4] == b[4] and a[5] == b[5]
    np.testing.assert_array_equal(bits(a[3]), bits(b[3]))
    assert b[6][0, 0] != PAD, "the item-armed slot draws in the first step of its first run"
    A.close()
    Bn.close()
    return a


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [3, 19])
def test_arm_from_an_item_equals_arm_with_the_prompt(kind, n):
    a = arm_from_item_case(kind, n)
    assert a[1] == 6 or a[2] == Fin.Stop


def test_arm_from_an_item_under_a_stop_string_and_under_json():
    free = arm_from_item_case("nucleus", 19)[0][0]
    tab = table(512)
    word = next((tab[x] for x in free[1:5] if x < len(tab) and tab[x]), None)
    assert word, f"no token of {free[1:5]} has bytes: pick another prompt"
    a = arm_from_item_case("nucleus", 19, stops=[word])
    assert a[2] == Fin.Stop and a[1] < 6
    arm_from_item_case("nucleus", 19, pda=rt.Pda.json(rt.PdaJson.Object | rt.PdaJson.Compact))


def test_two_slots_armed_from_one_item_at_the_same_time():
    """A runs the prompt on both slots, streams 5 and 9; B arms both slots from the ONE item A's slot 0 made.  Both engines decode in steps
    of two rows, so every token and probability is comparable bit for bit."""
    A, Bn = build("v6-tiny", 2), build("v6-tiny", 2)
    V = A.info.num_vocab
    P = prompt(V, 77, 3)
    for b, stream in ((0, 5), (1, 9)):
        A.gen_arm_prompt(b, P, 6, sampler("nucleus", P), seed=SEED, stream=stream)
    A.gen_set_capture(0, Cap.Prompt)
    ta, pa, nea, fina = A.gen_run(8)
    item = A.gen_take_item(0, Cap.Prompt)
    for b, stream in ((0, 5), (1, 9)):
        Bn.gen_arm_item(b, item, 6, sampler("nucleus", P), seed=SEED, stream=stream)
    item.close()                                                      # the slots hold what they need
    tb, pb, neb, finb = Bn.gen_run(8)
    for b in range(2):
        print("slot", b, emitted(ta, pa, b)[0], emitted(tb, pb, b)[0])
        assert emitted(ta, pa, b) == emitted(tb, pb, b)
        np.testing.assert_array_equal(bits(A.state.back(b)), bits(Bn.state.back(b)))
    assert list(nea) == list(neb) and list(fina) == list(finb)
    A.close()
    Bn.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_arm_from_an_item_next_to_decoding_slots():
    S = build("v6-tiny", 1)
    V = S.info.num_vocab
    ps = [prompt(V, 81, 5), prompt(V, 82, 6), prompt(V, 83, 11)]
    S.gen_arm_prompt(0, ps[2], 6, sampler("typical", ps[2]), seed=SEED, stream=2)
    S.gen_set_capture(0, Cap.Prompt)
    S.gen_run(8)
    item = S.gen_take_item(0, Cap.Prompt)
    host = item.back()
    S.gen_arm_item(0, item, 6, sampler("typical", ps[2]), seed=SEED, stream=2)
    t, p, ne, fin = S.gen_run(8)
    alone = (int(t[0, 0]), int(bits(p[0, 0])))
    S.close()
    got = []
    for _ in range(2):
        E = build("v6-tiny", 3)
        it = rt.GenItem.from_host(E, *host)
        runs = []
        for b in (0, 1):
            E.gen_arm_prompt(b, ps[b], 8, sampler(KINDS[b], ps[b]), seed=SEED)
        runs.append(E.gen_run(2))
        E.gen_arm_item(2, it, 6, sampler("typical", ps[2]), seed=SEED, stream=2)
        runs.append(E.gen_run(8))
        states = [E.state.back(b) for b in range(3)]
        # every live slot is item-armed: all first tokens come out of step 0, which runs no forward pass
        for b in range(3):
            E.gen_arm_item(b, it, 3, sampler(KINDS[b], ps[2]), seed=SEED, stream=10 + b)
        runs.append(E.gen_run(4))
        got.append((runs, states))
        it.close()
        E.close()
    (ra, sa), (rb, sb) = got
    for x, y in zip(ra, rb):
        same_run(x, y)
    for b in range(3):
        np.testing.assert_array_equal(bits(sa[b]), bits(sb[b]))
    t, p = ra[1][0], ra[1][1]
    print("alone", alone, "next to two decoding slots", (int(t[0, 2]), int(bits(p[0, 2]))))
    assert (int(t[0, 2]), int(bits(p[0, 2]))) == alone
    assert int(ra[1][2][2]) == 6 or int(ra[1][3][2]) == Fin.Stop
    assert (ra[2][0][0] != PAD).all(), "three item-armed slots draw their first tokens in step 0"


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_hand_over_pieces():
    A, E5 = build("v6-tiny", 2), build("v5-tiny", 1)
    V = A.info.num_vocab
    P = prompt(V, 91, 9)
    A.gen_arm_prompt(0, P, 3, sampler("nucleus", P), seed=SEED)
    A.gen_set_capture(0, BOTH)
    A.gen_run(4)
    item = A.gen_take_item(0, Cap.Prompt)
    st, row = item.back()
    A.state.write(item.state(), 1)                                    # a partial prefix hit continues from the item's state
    np.testing.assert_array_equal(bits(A.state.back(1)), bits(st))
    A.gen_arm_prompt(0, P, 3, sampler("nucleus", P), seed=SEED)       # re-arming drops the FINISH item nobody took, not the one taken
    assert code(lambda: A.gen_take_item(0, Cap.Finish)) == -1
    A.gen_run(2)
    A.gen_disarm(0)
    same_item(item.back(), (st, row))
    P5 = prompt(E5.info.num_vocab, 92, 4)
    E5.gen_arm_prompt(0, P5, 2, sampler("nucleus", P5), seed=SEED)
    E5.gen_set_capture(0, Cap.Prompt)
    E5.gen_run(2)
    item5 = E5.gen_take_item(0, Cap.Prompt)
    assert code(lambda: A.gen_arm_item(1, item5, 3, sampler("nucleus", P), seed=SEED)) == -1
    assert code(lambda: item5.back(A)) == -1
    np.testing.assert_array_equal(bits(A.state.back(1)), bits(st))     # the refused arm left slot 1 alone
    item.close()
    item5.close()
    A.close()
    E5.close()
    same = rt.lib().rwkv_gen_item_state(None)
    assert not same


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    """A makes every refused call at the point where it is refused; its twin T makes only the valid ones.  They agree on every run and item."""
    A, T = build("v6-tiny", 3), build("v6-tiny", 3)
    V = A.info.num_vocab
    P0, P1 = prompt(V, 95, 19), prompt(V, 96, 19)
    wide = H.NucleusSampler(top_p=0.8, top_k=300, temperature=1.0)
    wide.init(P0)
    log = {}
    for eng in (A, T):
        bad = eng is A
        runs, items = [], []
        w = eng.gen_watch_open(64)
        if bad:
            assert code(lambda: eng.gen_set_capture(0, Cap.Finish)) == -1          # nothing was ever armed
        eng.gen_arm_prompt(0, P0, 6, sampler("nucleus", P0), seed=SEED)
        eng.gen_set_capture(0, BOTH)
        if bad:
            assert code(lambda: eng.gen_take_item(0, Cap.Prompt)) == -1            # before the prompt is exhausted
            assert code(lambda: eng.gen_take_item(0, Cap.Finish)) == -1            # still running
            assert code(lambda: eng.gen_take_item(0, BOTH)) == -1                  # exactly one bit
            assert code(lambda: eng.gen_set_capture(0, 4)) == -1                   # an unknown bit
            assert code(lambda: eng.gen_set_capture(0, BOTH | 8)) == -1
            assert code(lambda: eng.gen_set_capture(1, Cap.Finish)) == -1          # an unarmed slot
        runs.append(eng.gen_run(1))                                                # 8 of 19 prompt tokens
        if bad:
            assert code(lambda: eng.gen_take_item(0, Cap.Prompt)) == -1
        runs.append(eng.gen_run(3))                                                # the prompt ends in the second of these
        assert eng.gen_prompt_left(0) == 0
        if bad:
            assert code(lambda: eng.gen_take_item(0, Cap.Finish)) == -1            # still running
        items.append(eng.gen_take_item(0, Cap.Prompt).back())
        if bad:
            assert code(lambda: eng.gen_take_item(0, Cap.Prompt)) == -1            # twice
            assert code(lambda: eng.gen_set_capture(0, BOTH)) == -1                # PROMPT on a slot that is already decoding
            assert code(lambda: eng.gen_set_capture(0, Cap.Prompt)) == -1
        eng.gen_arm_prompt(1, P1, 6, sampler("typical", P1), seed=SEED)
        eng.gen_set_capture(1, BOTH)
        runs.append(eng.gen_run(1))
        w.cancel(1)                                                                # inside its prompt
        runs.append(eng.gen_run(8))
        assert int(runs[-1][3][1]) == Fin.Cancelled and int(runs[-1][3][0]) == Fin.Length
        if bad:
            assert code(lambda: eng.gen_take_item(1, Cap.Prompt)) == -1            # cancelled inside the prompt: neither item exists
            assert code(lambda: eng.gen_take_item(1, Cap.Finish)) == -1
            assert code(lambda: eng.gen_set_capture(0, Cap.Finish)) == -1          # a finished slot
            assert code(lambda: eng.gen_set_capture(0, Cap(0))) == -1
        it = eng.gen_take_item(0, Cap.Finish)
        items.append(it.back())
        if bad:
            assert code(lambda: eng.gen_take_item(0, Cap.Finish)) == -1            # twice
            allow = np.ones(V, np.uint8)
            assert code(lambda: eng.gen_arm_item(2, it, 4, sampler("nucleus", P0), seed=SEED, allow=allow)) == -1
            assert code(lambda: eng.gen_arm_item(2, it, 4, wide, seed=SEED)) == -1  # top_k > 256 without RWKV_GEN_WIDE_TOP_K
            assert code(lambda: eng.gen_arm_item(2, None, 4, sampler("nucleus", P0), seed=SEED)) == -1
        runs.append(eng.gen_run(2))                                                # nobody is live: slot 2 was never armed
        assert (runs[-1][0] == PAD).all()
        eng.gen_arm_item(2, it, 4, sampler("nucleus", P0), seed=SEED)              # and the item still arms a slot
        runs.append(eng.gen_run(4))
        assert int(runs[-1][2][2]) >= 1
        log[bad] = (runs, items, [eng.state.back(b) for b in range(3)])
        it.close()
        w.close()
        eng.close()
    for x, y in zip(log[True][0], log[False][0]):
        same_run(x, y)
    for x, y in zip(log[True][1], log[False][1]):
        same_item(x, y)
    for x, y in zip(log[True][2], log[False][2]):
        np.testing.assert_array_equal(bits(x), bits(y))

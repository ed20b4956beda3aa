"""MI355X: a WATCH on resident generation (rwkv_gen_watch_*; gen_publish_kernel, csrc/gen_watch.h): another thread reads every step of a
running rwkv_gen_run as it ends and cancels slots inside it.

Engine A has a watch open, engine B has none; both are resident and armed alike, so nothing needs the per-token path and nothing is
compared with a tolerance: token ids, `out_probs` bits, n_emitted, finish, `gen_stop_tail` bytes, the constraint state, `state.back`.
Three slots, chunk 8 (the `build` of tests/test_gpu_gen_stop.py).  Every slot carries a bias of -60 on token 0, which stops a slot whatever
its settings are (run.rs:855): with 1024 ids and runs of 1024 steps it would otherwise be drawn, and the cases here end their slots
themselves.  The readers that poll have a deadline and sleep between polls."""
import threading
import time

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from tests import test_gpu_gen_stop as GS

pytestmark = pytest.mark.gpu

PAD = GS.PAD
MODELS = GS.MODELS
SEED = GS.SEED
Fin = rt.GenFinish
bits = GS.bits
BIAS = {0: -60.0}
LOOP = rb"([abc]{1,6};)*"                 # accepts behind every `;` and always leads on
STOPS = [b"abcab", b"ccbcc"]
RING = 1024                               # GEN_RING_STEPS of the engine: a longer run is split into enqueues of this many steps
LONG = 4000                               # max_tokens of a slot no case wants to see end


def start(name, quant, ring_steps=None):
    """an engine behind the three prompts, with a watch of `ring_steps` (A) or without (B)"""
    E = GS.build(name, quant)
    V = E.info.num_vocab
    prompts = [GS.prompt(V, 80 + b, 5 + 2 * b) for b in range(3)]
    first = GS.prefill(E, prompts)
    tab = GS.table(V, overrides={1: b"a", 2: b"b", 3: b"c", 4: b";"}, known=set(range(V)), with_pieces=False)   # no unknown id: no slot stops on one
    E.gen_set_token_bytes(tab)
    w = E.gen_watch_open(ring_steps) if ring_steps else None
    return E, w, V, prompts, first


def sampler(b, prompts, first=None):
    s = [H.NucleusSampler(top_p=0.8, top_k=32, temperature=1.2, frequency_penalty=0.4), H.TypicalSampler(tau=0.9, top_k=32),
         H.MirostatSampler(tau=3.0, rate=0.1)][b]
    s.init(prompts[b])
    if first is not None and b < 2:
        s.update(first[b])
    return s


def arm(E, b, prompts, first, max_tokens=LONG, stops=False, dfa=False):
    """slot b decoding from its first token: Nucleus (0), Typical (1), Mirostat (2)"""
    E.gen_arm(b, first[b], max_tokens, sampler(b, prompts, first), seed=SEED, bias=BIAS)
    if stops:
        E.gen_set_stops(b, STOPS)
    if dfa:
        E.gen_set_constraint(b, rt.Dfa.compile(LOOP))


def arm_prompt(E, b, V, n_tokens, max_tokens=LONG):
    """slot b armed by a prompt of n_tokens (chunk 8: n_tokens / 8 chunks when it is alone)"""
    p = GS.prompt(V, 300 + b, n_tokens)
    E.gen_arm_prompt(b, p, max_tokens, sampler(b, [p] * 3), seed=SEED, bias=BIAS)


def same_run(got, want, cols=(0, 1, 2), rows=slice(None)):
    np.testing.assert_array_equal(got[0][rows][:, cols], want[0][rows][:, cols])
    np.testing.assert_array_equal(bits(got[1][rows][:, cols]), bits(want[1][rows][:, cols]))


def same_slot_state(A, Bn, b):
    np.testing.assert_array_equal(A.state.back(b), Bn.state.back(b))
    assert A.gen_stop_tail(b) == Bn.gen_stop_tail(b)
    assert A.gen_constraint_state(b) == Bn.gen_constraint_state(b)


def read_all(w, at_most=4096):
    """everything behind the watch's cursor: (tokens, probs, finish, lost)"""
    t, p, f, lost = w.read(at_most)
    assert len(w.read(1)[0]) == 0 and w.cursor == w.head()
    return t, p, f, lost


def records_are_rows(rec, run, n_exec, fin_before):
    """the records of a run are the rows it executed, bit for bit; the rows behind them are padding; the finish column is 0 up to the step
    a slot finished in and its reason from there on"""
    t, p, f, lost = rec
    rt_, rp, _, fin = run
    assert lost == 0 and len(t) == n_exec, (lost, len(t), n_exec)
    np.testing.assert_array_equal(t, rt_[:n_exec])
    np.testing.assert_array_equal(bits(p), bits(rp[:n_exec]))
    assert (rt_[n_exec:] == PAD).all() and np.isnan(rp[n_exec:]).all()
    for b in range(t.shape[1]):
        want = np.zeros(n_exec, np.int32)
        if fin_before[b]:
            want[:] = fin_before[b]
        elif fin[b]:
            emitted = np.nonzero(rt_[:n_exec, b] != PAD)[0]
            want[emitted[-1]:] = fin[b]
        np.testing.assert_array_equal(f[:, b], want, err_msg=f"finish column of slot {b}")


def arm_mixed(E, V, prompts, first):
    """the arming of case 1: Nucleus with stop strings, Typical under a DFA, Mirostat armed by a prompt of three chunks"""
    arm(E, 0, prompts, first, max_tokens=20, stops=True)
    arm(E, 1, prompts, first, max_tokens=24, dfa=True)
    arm_prompt(E, 2, V, 24, max_tokens=9)


@pytest.mark.parametrize("name,quant", MODELS)
def test_watching_changes_nothing(name, quant):
    A, w, V, prompts, first = start(name, quant, 64)
    Bn, _, _, _, firstb = start(name, quant)
    assert first == firstb
    arm_mixed(A, V, prompts, first)
    arm_mixed(Bn, V, prompts, first)
    for n in (5, 30):
        ra, rb = A.gen_run(n), Bn.gen_run(n)
        print(name, n, "tokens", ra[0].T.tolist(), "n_emitted", ra[2], "finish", ra[3])
        same_run(ra, rb)
        assert list(ra[2]) == list(rb[2]) and list(ra[3]) == list(rb[3])
        for b in range(3):
            same_slot_state(A, Bn, b)
    assert all(ra[3]) and Fin.Cancelled not in list(ra[3])
    assert w.head() > 0
    A.close()
    Bn.close()


@pytest.mark.parametrize("name,quant", MODELS)
def test_records_are_the_rows_of_the_run(name, quant):
    A, w, V, prompts, first = start(name, quant, 2048)
    none = [0, 0, 0]
    for b in range(3):
        arm(A, b, prompts, first)
    run = A.gen_run(6)                                                # one row set, decode only: the first step direct, the rest the captured graph
    records_are_rows(read_all(w), run, 6, none)
    assert w.head() == 6
    r1, r2 = A.gen_run(3), A.gen_run(2)                               # two runs back to back: the sequence carries on
    t, p, f, lost = read_all(w)
    assert w.head() == 11 and lost == 0 and len(t) == 5
    records_are_rows((t[:3], p[:3], f[:3], 0), r1, 3, none)
    records_are_rows((t[3:], p[3:], f[3:], 0), r2, 2, none)
    run = A.gen_run(RING + 6)                                         # the engine splits this run into two enqueues
    records_are_rows(read_all(w), run, RING + 6, none)
    assert w.head() == 11 + RING + 6
    arm_prompt(A, 2, V, 40, max_tokens=3)                             # five chunks beside two decoding slots: mixed steps, then its three draws
    run = A.gen_run(12)
    assert run[2][2] == 3 and run[3][2] == Fin.Length and list(run[2][:2]) == [12, 12]
    first_draw = int(np.nonzero(run[0][:, 2] != PAD)[0][0])
    assert first_draw >= 5                                            # the prompt took that many steps: they carried prompt rows
    records_are_rows(read_all(w), run, 12, none)
    A.gen_disarm(0)
    A.gen_disarm(1)
    arm_prompt(A, 2, V, 40)                                           # only a prompt slot is live: steps that emit no row still publish
    head = w.head()
    run = A.gen_run(3)
    assert (run[0] == PAD).all() and A.gen_prompt_left(2) == 40 - 24
    records_are_rows(read_all(w), run, 3, none)
    assert w.head() == head + 3
    A.gen_disarm(2)
    for b in range(3):                                                # slots that end by themselves inside the run: 2, 3 and 4 tokens of 8 steps
        arm(A, b, prompts, first, max_tokens=2 + b)
    run = A.gen_run(8)
    assert list(run[2]) == [2, 3, 4] and list(run[3]) == [Fin.Length] * 3
    records_are_rows(read_all(w), run, 4, none)                       # the run executed four steps; the rows behind them are padding
    run = A.gen_run(2)                                                # nothing is live: no step, no record
    assert len(read_all(w)[0]) == 0 and (run[0] == PAD).all()
    A.close()


def test_a_reader_that_was_overrun_gets_the_youngest_records():
    name, quant = MODELS[0]
    A, w, V, prompts, first = start(name, quant, 4)
    for b in range(3):
        arm(A, b, prompts, first)
    run = A.gen_run(16)
    t, p, f, lost = w.read(64)
    assert lost == 12 and len(t) == 4 and w.cursor == 16 == w.head()
    np.testing.assert_array_equal(t, run[0][12:])
    np.testing.assert_array_equal(bits(p), bits(run[1][12:]))
    assert (f == 0).all()
    A.close()


def poll(w, stop, deadline_s, on_records):
    """the reader thread's loop: read, hand on, sleep; ends once `stop` is set and the ring is drained, or at the deadline"""
    deadline = time.monotonic() + deadline_s
    while time.monotonic() < deadline:
        done = stop.is_set()                                          # looked at BEFORE the read
        t, p, f, lost = w.read(256)
        if len(t) or lost:
            on_records(t, p, f, lost)
        elif done:
            return True
        else:
            time.sleep(0.0005)
    return False


def test_a_reader_thread_sees_the_run_while_it_runs():
    name, quant = MODELS[0]
    A, w, V, prompts, first = start(name, quant, 2048)
    for b in range(3):
        arm(A, b, prompts, first)
    returned, got, early, lost_all, ok = threading.Event(), [], [0], [0], [False]

    def on_records(t, p, f, lost):
        if not returned.is_set():                                     # looked at AFTER the read: these records were read while gen_run ran
            early[0] += len(t)
        got.append((t, p))
        lost_all[0] += lost

    th = threading.Thread(target=lambda: ok.__setitem__(0, poll(w, returned, 120.0, on_records)))
    th.start()
    try:
        run = A.gen_run(RING)
    finally:
        returned.set()
        th.join()
    print("records read before gen_run returned:", early[0], "of", RING)
    assert ok[0] and lost_all[0] == 0
    assert early[0] >= 1, "no record was visible during 1024 steps: the run cannot be watched"
    np.testing.assert_array_equal(np.concatenate([t for t, _ in got]), run[0])
    np.testing.assert_array_equal(bits(np.concatenate([p for _, p in got])), bits(run[1]))
    A.close()


@pytest.mark.parametrize("name,quant", MODELS)
def test_cancel_before_the_run_ends_the_slot_in_its_first_step(name, quant):
    A, w, V, prompts, first = start(name, quant, 64)
    Bn, _, _, _, _ = start(name, quant)
    for E in (A, Bn):
        arm(E, 0, prompts, first)
        arm(E, 1, prompts, first, stops=True, dfa=True)
        arm(E, 2, prompts, first)
    w.cancel(1)
    ra = A.gen_run(8)
    assert list(ra[2]) == [8, 1, 8] and list(ra[3]) == [Fin.Running, Fin.Cancelled, Fin.Running]
    assert (ra[0][1:, 1] == PAD).all() and np.isnan(ra[1][1:, 1]).all()
    rb1 = Bn.gen_run(1)                                               # B's slot 1 after one step, still running: what A's slot 1 must be
    assert list(rb1[3]) == [Fin.Running] * 3
    same_run(ra, rb1, rows=slice(0, 1))
    same_slot_state(A, Bn, 1)
    rb2 = Bn.gen_run(7)
    np.testing.assert_array_equal(ra[0][1:][:, [0, 2]], rb2[0][:, [0, 2]])
    np.testing.assert_array_equal(bits(ra[1][1:][:, [0, 2]]), bits(rb2[1][:, [0, 2]]))
    for b in (0, 2):
        same_slot_state(A, Bn, b)
    t, p, f, lost = read_all(w)
    np.testing.assert_array_equal(f, np.array([[0, Fin.Cancelled, 0]] * 8, np.int32))
    np.testing.assert_array_equal(t, ra[0])
    A.close()
    Bn.close()


@pytest.mark.parametrize("name,quant", MODELS)
def test_cancel_from_the_reader_inside_a_run(name, quant):
    A, w, V, prompts, first = start(name, quant, 2048)
    for b in range(3):
        arm(A, b, prompts, first)
    returned, seen, ok = threading.Event(), [0], [False]

    def on_records(t, p, f, lost):
        before = seen[0]
        seen[0] += int((t[:, 1] != PAD).sum())
        if before < 5 <= seen[0]:
            w.cancel(1)

    th = threading.Thread(target=lambda: ok.__setitem__(0, poll(w, returned, 120.0, on_records)))
    th.start()
    try:
        ra = A.gen_run(RING)
    finally:
        returned.set()
        th.join()
    n = int(ra[2][1])
    print(name, "slot 1 was cancelled after", n, "tokens")
    assert ok[0] and 5 <= n < RING
    assert list(ra[3]) == [Fin.Running, Fin.Cancelled, Fin.Running] and list(ra[2][[0, 2]]) == [RING, RING]
    Bn, _, _, _, _ = start(name, quant)                               # the uncancelled run
    for b in range(3):
        arm(Bn, b, prompts, first)
    rb = Bn.gen_run(RING)
    same_run(ra, rb, cols=(0, 2))                                     # the other slots are untouched
    same_run(ra, rb, cols=(1,), rows=slice(0, n))                     # a prefix of the uncancelled output
    assert (ra[0][n:, 1] == PAD).all() and np.isnan(ra[1][n:, 1]).all()
    for b in (0, 2):
        np.testing.assert_array_equal(A.state.back(b), Bn.state.back(b))
    Bn.close()
    Bs, _, _, _, _ = start(name, quant)                               # B after n steps: slot 1 has consumed everything but its n-th token
    for b in range(3):
        arm(Bs, b, prompts, first)
    Bs.gen_run(n)
    np.testing.assert_array_equal(A.state.back(1), Bs.state.back(1))
    Bs.close()
    A.close()


def test_precedence_and_the_life_of_a_flag():
    name, quant = MODELS[1]
    A, w, V, prompts, first = start(name, quant, 64)
    Bn, _, _, _, _ = start(name, quant)
    snap = A.state.back(1)
    arm(A, 0, prompts, first, max_tokens=1)                           # finishes by itself in the step that sees the flag: its own reason stands
    arm(A, 1, prompts, first)
    w.cancel(0)
    w.cancel(2)                                                       # not armed: nothing happens
    r = A.gen_run(4)
    assert list(r[2]) == [1, 4, 0] and list(r[3]) == [Fin.Length, Fin.Running, Fin.Running]
    w.cancel(0)                                                       # finished: nothing happens
    w.cancel(1)
    r = A.gen_run(4)
    assert list(r[2]) == [0, 1, 0] and list(r[3]) == [Fin.Length, Fin.Cancelled, Fin.Running]
    r = A.gen_run(4)                                                  # a cancelled slot takes no part in the next run
    assert list(r[2]) == [0, 0, 0] and list(r[3]) == [Fin.Length, Fin.Cancelled, Fin.Running] and (r[0] == PAD).all()
    # cancel, re-arm, run: arming clears the flag (slot 2's was set while it was unarmed, slot 1's ended its last request)
    for E in (A, Bn):
        E.state.load(snap, 1)                                         # slot 1 as both engines held it behind the prompt (this disarms it)
        arm(E, 1, prompts, first, max_tokens=6)
        arm(E, 2, prompts, first, max_tokens=6)
    ra, rb = A.gen_run(8), Bn.gen_run(8)
    assert list(ra[2]) == [0, 6, 6] and list(ra[3]) == [Fin.Length, Fin.Length, Fin.Length]
    same_run(ra, rb, cols=(1, 2))
    w.cancel(1)
    A.gen_disarm(1)                                                   # disarming clears it too
    arm(A, 1, prompts, first, max_tokens=2)
    r = A.gen_run(4)
    assert r[2][1] == 2 and r[3][1] == Fin.Length
    A.close()
    Bn.close()


def test_cancel_inside_a_prompt():
    name, quant = MODELS[0]
    A, w, V, prompts, first = start(name, quant, 64)
    A2, w2, _, _, _ = start(name, quant, 16)                          # a second watched engine with the same cancelled arm
    Bn, _, _, _, _ = start(name, quant)                               # no watch, and slot 1 not armed at all
    for E in (A, A2, Bn):
        arm(E, 0, prompts, first)
    for E in (A, A2):
        arm_prompt(E, 1, V, 48)                                       # six chunks
    before = A.state.back(1)
    w.cancel(1)
    w2.cancel(1)
    ra, ra2, rb = A.gen_run(4), A2.gen_run(4), Bn.gen_run(4)
    assert list(ra[2]) == [4, 0, 0] and list(ra[3]) == [Fin.Running, Fin.Cancelled, Fin.Running]
    assert (ra[0][:, 1] == PAD).all()
    assert A.gen_prompt_left(1) == 48                                 # the flag was seen at the first plan: nothing was fed
    np.testing.assert_array_equal(A.state.back(1), before)
    same_run(ra, ra2, cols=(0,))
    # the slot was never planned, so the neighbour's steps are those of an engine on which it was never armed: the same step shapes, and
    # therefore the same bits ("what a joiner does to the others" concerns steps that carry prompt rows; there were none)
    same_run(ra, rb, cols=(0,))
    np.testing.assert_array_equal(A.state.back(0), Bn.state.back(0))
    t, p, f, lost = read_all(w)
    np.testing.assert_array_equal(t, ra[0])
    assert (f == 0).all()                                             # the host marks the slot when the run returns ...
    r = A.gen_run(2)
    assert list(r[2]) == [2, 0, 0] and r[3][1] == Fin.Cancelled       # ... and it takes no part in the next run
    assert (read_all(w)[2][:, 1] == Fin.Cancelled).all()
    # a prompt that is under way: cancelled between two runs, it keeps what was left and the state of the tokens fed so far
    arm_prompt(A, 2, V, 48)
    A.gen_run(2)
    left = A.gen_prompt_left(2)
    assert 0 < left < 48
    mid = A.state.back(2)
    w.cancel(2)
    r = A.gen_run(3)
    assert r[2][2] == 0 and r[3][2] == Fin.Cancelled and A.gen_prompt_left(2) == left
    np.testing.assert_array_equal(A.state.back(2), mid)
    for E in (A, A2, Bn):
        E.close()


def test_a_second_watch_publishes_through_the_graphs_of_the_first():
    name, quant = MODELS[0]
    A, w, V, prompts, first = start(name, quant, 16)
    for b in range(3):
        arm(A, b, prompts, first)
    run = A.gen_run(6)                                                # the row set's graph is captured under the first watch
    records_are_rows(read_all(w), run, 6, [0, 0, 0])
    w.close()
    run = A.gen_run(3)                                                # no watch: the unwatched step
    assert (run[0] != PAD).all()
    w = A.gen_watch_open(7)
    assert w.head() == 0
    run = A.gen_run(5)                                                # the same row set: the cached graph, the new ring
    records_are_rows(read_all(w), run, 5, [0, 0, 0])
    run = A.gen_run(9)                                                # and around the new ring's end
    t, p, f, lost = read_all(w)
    assert lost == 2 and w.head() == 14
    np.testing.assert_array_equal(t, run[0][2:])
    np.testing.assert_array_equal(bits(p), bits(run[1][2:]))
    A.close()                                                         # with the watch open: the destructor closes it


def test_refusals():
    import ctypes as C
    name, quant = MODELS[0]
    A, w, V, prompts, first = start(name, quant, 8)

    def code(f):
        with pytest.raises(rt.RwkvError) as e:
            f()
        return e.value.code

    assert code(lambda: A.gen_watch_open(8)) == -1                    # a second watch
    w.close()
    assert code(lambda: A.gen_watch_open(0)) == -1
    assert code(lambda: A.gen_watch_open(rt.GEN_WATCH_MAX_STEPS + 1)) == -1
    w = A.gen_watch_open(rt.GEN_WATCH_MAX_STEPS)
    w.close()
    w = A.gen_watch_open(8)
    assert code(lambda: w.cancel(-1)) == -1 and code(lambda: w.cancel(3)) == -1
    l, h = rt.lib(), w._h
    cur, n, lost, seq = C.c_uint64(0), C.c_int32(0), C.c_uint64(0), C.c_uint64(0)
    tok = (C.c_uint32 * 24)()
    assert l.rwkv_gen_watch_open(A._h, 8, None) == -1
    assert l.rwkv_gen_watch_close(A._h, None) == -1
    assert l.rwkv_gen_watch_head(h, None) == -1 and l.rwkv_gen_watch_head(None, C.byref(seq)) == -1
    assert l.rwkv_gen_watch_read(h, None, 8, tok, None, None, C.byref(n), C.byref(lost)) == -1
    assert l.rwkv_gen_watch_read(h, C.byref(cur), 8, None, None, None, C.byref(n), C.byref(lost)) == -1
    assert l.rwkv_gen_watch_read(h, C.byref(cur), 8, tok, None, None, None, C.byref(lost)) == -1
    assert l.rwkv_gen_watch_read(h, C.byref(cur), 8, tok, None, None, C.byref(n), None) == -1
    assert l.rwkv_gen_watch_read(h, C.byref(cur), -1, tok, None, None, C.byref(n), C.byref(lost)) == -1
    assert l.rwkv_gen_watch_read(h, C.byref(cur), 8, tok, None, None, C.byref(n), C.byref(lost)) == 0 and n.value == 0
    assert l.rwkv_gen_watch_cancel(None, 0) == -1
    A.close()


def test_the_stream_yields_what_generate_resident_returns():
    name, quant = MODELS[0]
    A, _, V, prompts, first = start(name, quant)
    Bn, _, _, _, _ = start(name, quant)
    p = GS.prompt(V, 400, 11)

    def smp():
        s = H.NucleusSampler(top_p=0.8, top_k=32, temperature=1.2, frequency_penalty=0.4, bias=BIAS)
        s.init(p)
        return s

    want = H.generate_resident(Bn, 0, p, 24, smp(), seed=SEED)
    got = list(H.generate_resident_stream(A, 0, p, 24, smp(), seed=SEED))
    assert len(want) == 24 and [t for t, _ in got] == [t for t, _ in want]
    np.testing.assert_array_equal(bits([q for _, q in got]), bits([q for _, q in want]))
    g = H.generate_resident_stream(A, 1, p, LONG, smp(), seed=SEED, steps_per_run=RING)
    head = [next(g) for _ in range(3)]
    g.close()                                                         # the client is gone
    assert [t for t, _ in head] == [t for t, _ in H.generate_resident(Bn, 1, p, 3, smp(), seed=SEED)]
    r = A.gen_run(1)
    assert r[3][1] == Fin.Cancelled and r[2][1] == 0
    w = A.gen_watch_open(8)                                           # the generator closed its watch
    w.close()
    A.close()
    Bn.close()

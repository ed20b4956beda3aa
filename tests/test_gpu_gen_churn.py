"""MI355X: resident generation through eviction of `gen_graphs`, the 64-entry cache of captured decode steps (`gen_decode_steps`).

A captured generation step fixes its row count, its launch set and every pointer; only the row metadata is uploaded fresh.  A replay under
the wrong key would produce tokens and nothing would complain — unless the tokens are compared.  tests/gen_churn.py holds the visit list (70
distinct row sets over seven seats of a 72-slot engine, then the three oldest and the three newest again) and
tests/test_gen_churn_cpu.py proves on the real rwkv::GraphCache that it evicts nine entries, captures three evicted keys again and replays
three cached ones.  Here every visit arms the seats of its row set with max_tokens 3 and runs three steps: on a new key one direct step, the
capture and two replays; on a key that was evicted the capture and three replays; on a cached key three replays.

Each seat is ONE uninterrupted request: every arm behind the first is `gen_arm(seat, first_token = its last emitted token, ...)` on the
state the state rule left, with the same sampler object carried on and a stream of its own per visit, and the lock-step reference of
tests/test_gpu_gen_prompt.py just continues per token.  Token ids, `out_probs` bits, n_emitted, finish and the states of the visit's seats are
compared with no tolerance in every visit, the states of all seven seats at the end.  Three bands of visits change the key's flag word and the
launch set of the captured step — an open watch, a seat that lists top-n, a seat that carries a stop string which cannot match — and promise
to change no token."""
import copy

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from tests import gen_churn as CH
from tests import test_gpu_gen_prompt as GP
from tests import test_gpu_gen_stop as GS
from tests import test_gpu_generate as GG

pytestmark = pytest.mark.gpu

PAD, SEED = GP.PAD, GP.SEED
NO_ZERO = {0: -100.0}                                              # token 0 ends a request: no seat ever draws it


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def seat_sampler(i):
    kind = CH.KINDS[i % 3]
    if kind == "nucleus":
        return H.NucleusSampler(top_p=0.8, top_k=32, temperature=1.2, presence_penalty=0.3, frequency_penalty=0.4, penalty_decay=0.99, bias=NO_ZERO)
    if kind == "typical":
        return H.TypicalSampler(tau=0.9, top_k=32, temperature=1.2, presence_penalty=0.2, frequency_penalty=0.4, bias=NO_ZERO)
    return GG.BiasedMirostat(bias=NO_ZERO, tau=2.0, rate=0.3)


def test_seven_seats_through_seventy_row_sets_and_back():
    A, Bn = GP.build_pair("v6-tiny", CH.MAX_BATCH, chunk=8)
    V, B, Fin = A.info.num_vocab, CH.MAX_BATCH, rt.GenFinish
    tab = GS.table(V, known=set(range(V)))                            # no id is unknown: an unknown id ends a slot that carries strings
    assert all(w is not None and b"z" not in w for w in tab)
    A.gen_set_token_bytes(tab)                                        # before the first visit: a new table clears gen_graphs
    prompts = [[] for _ in range(B)]
    for i, slot in enumerate(CH.SEATS):
        prompts[slot] = GG.prompt(V, 300 + i, 4 + i)
    first = GG.prefill(A, prompts)
    assert GG.prefill(Bn, prompts) == first
    smp, cur, state = {}, {}, {}
    for i, slot in enumerate(CH.SEATS):
        smp[i] = seat_sampler(i)
        smp[i].init(prompts[slot])
        if not GP.is_miro(smp[i]):
            smp[i].update(first[slot])
        cur[i] = first[slot]
    watch = None
    for v, seats in enumerate(CH.VISITS):
        band = CH.band(v)
        if band == "watch" and watch is None:
            watch = A.gen_watch_open(8)
        if band != "watch" and watch is not None:
            watch.close()
            watch = None
        jobs = {}
        for i in seats:
            slot = CH.SEATS[i]
            A.gen_arm(slot, cur[i], 3, copy.deepcopy(smp[i]), seed=SEED, stream=CH.stream(v, i))
            if i in state:
                Bn.state.load(state[i], slot)                         # what the state rule left (the reference engine may have ridden past it)
            jobs[slot] = GP.Job([cur[i]], smp[i], 3, CH.stream(v, i), False)
        feat = CH.SEATS[CH.featured(v)]
        if band == "topn":
            A.gen_set_topn(feat, CH.TOPN_N)
        if band == "stops":
            A.gen_set_stops(feat, [CH.STOP_STRING])
        got = A.gen_run(3, top=CH.TOPN_N if band == "topn" else 0)
        t, p, ne, fin = got[:4]
        T, P = GP.lockstep(Bn, jobs, 3)
        print("visit", v, "key", " ".join(f"{w:x}" for w in CH.key(v)), "band", band, {s: [x for x, _ in j.out[-3:]] for s, j in jobs.items()})
        for slot in range(B):
            on = T[:, slot] != PAD
            assert (t[:, slot] == T[:, slot]).all(), (v, slot, "want", T[:, slot].tolist(), "got", t[:, slot].tolist())
            assert np.isnan(p[~on, slot]).all() and (bits(p[on, slot]) == bits(P[on, slot])).all(), (v, slot, "probs")
            assert int(ne[slot]) == int(on.sum()), (v, slot, int(ne[slot]))
        for slot, j in jobs.items():
            assert int(fin[slot]) == j.fin == int(Fin.Length) and len(j.out) == 3, (v, slot, int(fin[slot]), j.fin)
            assert (bits(A.state.back(slot)) == bits(j.state)).all(), (v, slot, "state")
        if band == "watch":                                           # the records are the rows of the run
            wt, wp, wf, lost = watch.read(8)
            assert len(wt) == 3 and lost == 0 and watch.head() == 3 * (v - CH.BANDS["watch"][0] + 1), (v, len(wt), lost, watch.head())
            assert (wt == t).all() and (bits(wp) == bits(p)).all(), v
            assert all(int(wf[2, slot]) == int(fin[slot]) for slot in jobs) and not any(wf[:2, slot].any() for slot in jobs), v
        if band == "topn":
            tok_lp, top_ids, top_lp = got[4:]
            for k in range(3):
                ids, lp = top_ids[k, feat], top_lp[k, feat]
                assert (ids != rt.TOPN_NONE).all() and len(set(ids.tolist())) == CH.TOPN_N and (np.diff(lp) <= 0).all(), (v, k, ids, lp)
                hit = np.nonzero(ids == t[k, feat])[0]
                assert not np.isnan(tok_lp[k, feat]), (v, k)
                if len(hit):
                    assert bits(lp[hit[0]]) == bits(tok_lp[k, feat]), (v, k)
                else:                                                 # not listed: no likelier than the last place
                    assert tok_lp[k, feat] <= lp[-1], (v, k)
                for slot in jobs:
                    if slot != feat:                                  # a seat that lists nothing: padding
                        assert (top_ids[k, slot] == rt.TOPN_NONE).all() and np.isnan(tok_lp[k, slot]), (v, k, slot)
        for i in seats:
            j = jobs[CH.SEATS[i]]
            cur[i], state[i] = j.out[-1][0], j.state
    assert watch is None and len(state) == len(CH.SEATS)
    for i, slot in enumerate(CH.SEATS):
        assert (bits(A.state.back(slot)) == bits(state[i])).all(), ("at the end", slot)
    A.close()
    Bn.close()

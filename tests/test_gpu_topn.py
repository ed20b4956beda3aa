"""GPU (-m gpu): top-n lists through the ABI — `rwkv_topn_rows` (the kernel behind the softmax task's staging), `rwkv_infer_topn` (behind the
head GEMM of a prefill step) and `rwkv_gen_set_topn` / `rwkv_gen_run_topn` (inside the resident step) — against `tests/topn_cases.topn_ref` on
the rows `rwkv_infer` returns from a second engine fed the same way.

Nothing is compared with a tolerance: the ids of a list are a function of the row's bits, and every listed ln-probability is `rwkv_score_rows`'
value for that row and id, bit for bit (the float64 bound on that value is tests/test_gpu_score.py's and tests/test_gpu_topn_exact.py's)."""
import ctypes as C

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import topn_cases as T
from tests.test_gpu_gen_dfa import LOOP, table

pytestmark = pytest.mark.gpu
NONE, PAD, SKIP = rt.TOPN_NONE, 0xFFFFFFFF, rt.SCORE_SKIP
SEED = 20251201


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def prompt(V, slot, n):
    return [t % V for t in R.synth_prompt(slot, n)]


def check_list(scorer, row, n, ids, logp, what):
    """`ids` / `logp` (any stride >= n; places behind n must be padding) are the list of `row`: ids exact, logp bit-equal to score_rows."""
    want, want_lp = T.topn_ref(row, n)
    assert ids[:n].tolist() == want.tolist(), (what, ids[:n].tolist(), want.tolist())
    assert (ids[n:] == NONE).all() and (logp[n:] == -np.inf).all(), what
    live = want != NONE
    if np.isnan(want_lp).all():
        assert np.isnan(logp[:n]).all(), what
        return
    assert (logp[:n][~live] == -np.inf).all(), what
    if live.any():
        got = scorer.score_rows([row] * int(live.sum()), want[live])
        np.testing.assert_array_equal(bits(logp[:n][live]), bits(got), err_msg=str(what))


# ------------------------------------------------------------------------------------------------
# 1. the kernel through rwkv_topn_rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", T.VOCABS)
def test_kernel_through_topn_rows(V):
    # max_batch 2: the staging holds two rows, so a five-row call is processed in pieces
    eng = rt.ModelBuilder(R.st_serialize(R.synth_checkpoint(7, 1, 64, 256, V, seed=77, lora_dims=(32, 32, 32, 32)))).build(max_batch=2, token_chunk_size=16)
    rows = T.rows_of(V)
    names = list(rows)
    for n in (T.NS if V < 4096 else (5, 32)):
        for i0 in range(0, len(names), 5):
            part = names[i0:i0 + 5]
            ids, lp = eng.topn_rows([rows[nm] for nm in part], n)
            assert ids.shape == lp.shape == (len(part), n) and ids.dtype == np.uint32 and lp.dtype == np.float32
            for r, nm in enumerate(part):
                check_list(eng, rows[nm], n, ids[r], lp[r], (V, n, nm))
    # refusals leave the outputs untouched (the raw call: the wrapper allocates its own outputs)
    two = [rows["normal0"], rows["equal"]]
    pi = (C.c_void_p * 2)(*[r.ctypes.data for r in two])
    ids, lp = np.full(64, 7, np.uint32), np.full(64, 7.0, np.float32)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    for n in (0, -3, 33):
        assert rt.lib().rwkv_topn_rows(eng._h, pi, n, ids.ctypes.data_as(u32p), lp.ctypes.data_as(f32p), 2) == -1
    pi[1] = None
    assert rt.lib().rwkv_topn_rows(eng._h, pi, 5, ids.ctypes.data_as(u32p), lp.ctypes.data_as(f32p), 2) == -1
    assert (ids == 7).all() and (lp == 7.0).all()
    eng.close()


# ------------------------------------------------------------------------------------------------
# 2. rwkv_infer_topn against the rows rwkv_infer returns from a second engine fed the same way
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v5-tiny", "v6-tiny", "v7-tiny"])
def test_infer_topn_against_the_rows_of_a_second_engine(name):
    st = R.st_serialize(R.synth_named(name))
    A = rt.ModelBuilder(st).build(max_batch=3, token_chunk_size=16, precision=rt.Precision.Fp16)
    Bn = rt.ModelBuilder(st).build(max_batch=3, token_chunk_size=16, precision=rt.Precision.Fp16)
    V, n = A.info.num_vocab, 5
    prompts = [prompt(V, 40 + b, k) for b, k in enumerate((19, 21, 18))]         # a few tokens over the chunk: every call splits
    opts = [rt.RnnOption.Full, rt.RnnOption.Last, rt.RnnOption.NoOutput]
    targets = [[(p[i + 1] if i % 4 else (p[i] * 7 + 3) % V) for i in range(len(p) - 1)] + [SKIP] for p in prompts[:1]] + [None, None]
    ia = rt.RnnInput([rt.RnnInputBatch(list(p), o) for p, o in zip(prompts, opts)])
    ib = rt.RnnInput([rt.RnnInputBatch(list(p), o) for p, o in zip(prompts, opts)])
    tg = [None if t is None else list(t) for t in targets]
    done, calls = [0, 0, 0], 0
    while ia.num_token() > 0:
        before = [len(b.tokens) for b in ia.batches]
        ia, tg, lists = A.infer_topn(ia, n, tg)
        ib, outs = Bn.infer(ib)
        calls += 1
        assert [len(b.tokens) for b in ia.batches] == [len(b.tokens) for b in ib.batches]        # n_consumed as rwkv_infer's
        for b in range(3):
            rows = list(outs[b])
            if opts[b] == rt.RnnOption.NoOutput:
                assert lists[b] is None and not rows
                continue
            ids, lp, tok_lp = lists[b]
            assert len(ids) == len(lp) == len(rows), (b, len(ids), len(rows))                    # n_rows as rwkv_infer's
            for r, row in enumerate(rows):
                check_list(Bn, row, n, ids[r], lp[r], (name, b, done[b] + r))
            if b == 0:
                t = np.array(targets[0][done[0]:done[0] + len(rows)], np.uint32)
                np.testing.assert_array_equal(bits(tok_lp), bits(Bn.score_rows(rows, t)))          # NaN where skipped, the same NaN
            else:
                assert tok_lp is None
        for b in range(3):
            done[b] += before[b] - len(ia.batches[b].tokens)
    assert calls >= 4 and done == [19, 21, 18]
    for b in range(3):
        np.testing.assert_array_equal(bits(A.state.back(b)), bits(Bn.state.back(b)))
    # the `Last` rows of the other slots are undisturbed: a piece through rwkv_infer on both engines
    piece = prompt(V, 50, 9)
    got = []
    for eng in (A, Bn):
        inp = rt.RnnInput([rt.RnnInputBatch(), rt.RnnInputBatch(list(piece), rt.RnnOption.Last), rt.RnnInputBatch()])
        while inp.num_token():
            inp, outs = eng.infer(inp)
        got.append(outs[1][-1])
    np.testing.assert_array_equal(bits(got[0]), bits(got[1]))
    # out_tok_logp is rwkv_infer_score's value: the same call shapes (one Full slot with targets, one state-only) through both entry points
    doc = prompt(V, 51, 21)
    dt = doc[1:] + [SKIP]
    for eng in (A, Bn):
        for b in range(3):
            eng.state.load(eng.state.init(), b)
    ia = rt.RnnInput([rt.RnnInputBatch(list(doc), rt.RnnOption.Full), rt.RnnInputBatch(), rt.RnnInputBatch(list(piece), rt.RnnOption.NoOutput)])
    ib = rt.RnnInput([rt.RnnInputBatch(list(doc), rt.RnnOption.Full), rt.RnnInputBatch(), rt.RnnInputBatch(list(piece), rt.RnnOption.NoOutput)])
    ta, tb = [list(dt), None, None], [list(dt), None, None]
    while ia.num_token() > 0:
        ia, ta, lists = A.infer_topn(ia, 32, ta)
        ib, tb, scores = Bn.infer_score(ib, tb)
        np.testing.assert_array_equal(bits(lists[0][2]), bits(scores[0]))
        for r in range(len(scores[0])):                                                         # the token's entry in the list, when listed
            t = dt[len(dt) - len(ta[0]) - len(scores[0]) + r]
            hit = np.nonzero(lists[0][0][r] == t)[0]
            if t != SKIP and len(hit):
                assert bits(lists[0][1][r][hit[0]]) == bits(scores[0][r])
    # refusals: a slot that wants rows but lists nothing; targets on a `Last` slot; nothing consumed
    inp = rt.RnnInput([rt.RnnInputBatch([1, 2], rt.RnnOption.Last), rt.RnnInputBatch(), rt.RnnInputBatch()])
    with pytest.raises(rt.RwkvError) as e:
        A.infer_topn(inp, 5, None, listing=[False, False, False])
    assert e.value.code == -1 and len(inp.batches[0].tokens) == 2
    with pytest.raises(rt.RwkvError) as e:
        A.infer_topn(inp, 5, [[2, SKIP], None, None])
    assert e.value.code == -1 and len(inp.batches[0].tokens) == 2
    A.close()
    Bn.close()


# ------------------------------------------------------------------------------------------------
# 3. resident generation
# ------------------------------------------------------------------------------------------------
STEPS, RUNS, MAXTOK, PLEN = 12, (5, 5, 2), 12, 11


def samplers(prompts, first):
    s0 = H.NucleusSampler(top_p=0.8, top_k=32, temperature=1.2, presence_penalty=0.3, frequency_penalty=0.4, penalty_decay=0.99)
    s0.init(prompts[0])
    s0.update(first[0])
    s2 = H.NucleusSampler(top_p=0.9, top_k=64, temperature=1.0, presence_penalty=0.2, frequency_penalty=0.2, penalty_decay=0.99)
    s2.init(prompts[2])
    return s0, H.MirostatSampler(tau=2.0, rate=0.3), s2


def prefill(eng, prompts):
    inp = rt.RnnInput([rt.RnnInputBatch(list(p)) for p in prompts])
    first = [None] * len(prompts)
    while inp.num_token() > 0:
        inp, outs = eng.infer(inp)
        for b, o in enumerate(outs):
            if len(o):
                first[b] = int(np.argmax(o[-1]))
    return first


def arm(eng, prompts, first, tab, dfa, stop1, lists):
    """slot 0: Nucleus with penalties and a bias; slot 1: Mirostat, stops early by a stop token; slot 2: armed with its PROMPT, constrained"""
    V = eng.info.num_vocab
    s0, s1, s2 = samplers(prompts, first)
    eng.gen_set_token_bytes(tab)
    eng.gen_arm(0, first[0], MAXTOK, s0, seed=SEED, bias={3 % V: 1.5, 17 % V: -2.0})
    eng.gen_arm(1, first[1], MAXTOK, s1, seed=SEED, stop_tokens=stop1)
    eng.gen_arm_prompt(2, prompts[2], MAXTOK, s2, seed=SEED)
    eng.gen_set_constraint(2, dfa)
    if lists:
        eng.gen_set_topn(0, 5)
        eng.gen_set_topn(1, 0)
        eng.gen_set_topn(2, 32)


def run(eng, top):
    """12 steps in runs of 5, 5 and 2: a run boundary falls inside.  Returns the per-run results and the concatenated step-major arrays."""
    per_run = [eng.gen_run(k, top=top) for k in RUNS]
    return per_run, [np.concatenate([r[i] for r in per_run]) for i in ((0, 1, 4, 5, 6) if top else (0, 1))]


def test_resident_generation_lists_the_raw_rows_and_changes_nothing():
    st = R.st_serialize(R.synth_named("v6-tiny"))
    mk = lambda: rt.ModelBuilder(st).build(max_batch=3, token_chunk_size=8, precision=rt.Precision.Fp16)
    D, A, A0, Bn = mk(), mk(), mk(), mk()
    V = A.info.num_vocab
    tab, dfa = table(V), rt.Dfa.compile(LOOP)
    prompts = [prompt(V, 90, 5), prompt(V, 91, 7), prompt(V, 92, PLEN)]
    first = prefill(D, prompts[:2] + [[]])
    for eng in (A, A0, Bn):
        assert prefill(eng, prompts[:2] + [[]]) == first
    # a dry run finds the token slot 1 emits fourth: with it as stop token the slot stops early
    arm(D, prompts, first, tab, dfa, (), False)
    _, (t, _) = run(D, 0)
    col1 = t[:, 1][t[:, 1] != PAD].tolist()
    k_stop = next(i for i in range(2, len(col1)) if col1[i] not in col1[:i] and col1[i] != 0)
    assert k_stop < 8, col1
    stop1 = (col1[k_stop],)
    D.close()
    arm(A, prompts, first, tab, dfa, stop1, True)
    arm(A0, prompts, first, tab, dfa, stop1, False)
    # an n_top smaller than a slot's n is refused before any step: the runs below equal A0's, which never saw the call
    with pytest.raises(rt.RwkvError) as e:
        A.gen_run(3, top=16)
    assert e.value.code == -1
    runs, (tok, prob, tok_lp, top_ids, top_lp) = run(A, 32)
    runs0, (tok0, prob0) = run(A0, 0)
    # (a) listing changes nothing: tokens, probabilities, counts, finish reasons, constraint state and state slabs are bit-identical
    np.testing.assert_array_equal(tok, tok0)
    np.testing.assert_array_equal(np.isnan(prob), np.isnan(prob0))
    np.testing.assert_array_equal(bits(prob[~np.isnan(prob)]), bits(prob0[~np.isnan(prob0)]))
    for r, r0 in zip(runs, runs0):
        np.testing.assert_array_equal(r[2], r0[2])
        np.testing.assert_array_equal(r[3], r0[3])
    assert A.gen_constraint_state(2) == A0.gen_constraint_state(2)
    for b in range(3):
        np.testing.assert_array_equal(bits(A.state.back(b)), bits(A0.state.back(b)))
    emitted = [int((tok[:, b] != PAD).sum()) for b in range(3)]
    assert emitted[1] == k_stop + 1 and runs[-1][3][1] == int(rt.GenFinish.Stop) and emitted[0] >= 6 and emitted[2] >= 6, emitted
    assert tok[0, 2] == PAD and tok[1, 2] != PAD                      # the 11-token prompt takes two steps at chunk 8: the first draw is step 1's
    # (b) the run replayed per token on B with the rows each resident step carries, the raw rows taken from rwkv_infer
    pending = [[first[0]], [first[1]], list(prompts[2])]
    in_prompt, fin_seen, count = [False, False, True], [False] * 3, [0] * 3
    raw = {}

    def step(k, slots):
        inp = rt.RnnInput([rt.RnnInputBatch(list(pending[b]) if b in slots else []) for b in range(3)])
        inp, outs = Bn.infer(inp)
        for b in slots:
            if not len(outs[b]):
                pending[b] = list(inp.batches[b].tokens)                 # still in its prompt
                continue
            in_prompt[b] = False
            if tok[k, b] != PAD:
                raw[(k, b)] = outs[b][-1]
                pending[b] = [int(tok[k, b])]
            # else: a rider (it finished earlier in this run): its row is thrown away, it feeds what it fed

    k0 = 0
    for steps, res in zip(RUNS, runs):
        live = [b for b in range(3) if not fin_seen[b]]
        remain = {b: MAXTOK - count[b] for b in live}
        k = 0
        while k < steps:
            pro = [b for b in live if in_prompt[b]]
            dec = [b for b in live if not in_prompt[b] and remain[b] > 0]
            if pro:
                step(k0 + k, dec + pro)
                for b in dec:
                    remain[b] -= 1
                for b in pro:
                    if not in_prompt[b]:
                        remain[b] -= 1
                k += 1
            elif not dec:
                break
            else:
                m = min(max(remain[b] for b in dec), steps - k)
                for i in range(m):
                    step(k0 + k + i, dec)
                for b in dec:
                    remain[b] = max(0, remain[b] - m)
                k += m
        for b in live:
            count[b] += int(res[2][b])
            fin_seen[b] = bool(res[3][b])
        k0 += steps
    assert len(raw) == sum(emitted)
    for k in range(STEPS):
        for b, n in enumerate((5, 0, 32)):
            ids, lp = top_ids[k, b], top_lp[k, b]
            if tok[k, b] == PAD:                                         # nothing emitted: in its prompt, finished, or behind its max_tokens
                assert (ids == NONE).all() and np.isnan(lp).all() and np.isnan(tok_lp[k, b]), (k, b)
                continue
            row = raw[(k, b)]
            if n == 0:                                                   # the slot lists nothing: its columns are padding
                assert (ids == NONE).all() and (lp == -np.inf).all() and np.isnan(tok_lp[k, b]), (k, b)
                continue
            check_list(Bn, row, n, ids, lp, ("gen", k, b))
            assert bits(tok_lp[k, b]) == bits(Bn.score_rows([row], [int(tok[k, b])])[0]), (k, b)
            hit = np.nonzero(ids == tok[k, b])[0]
            if len(hit):
                assert bits(lp[hit[0]]) == bits(tok_lp[k, b])
    # rwkv_gen_run stays callable on listing slots, and re-arming resets a slot's count: slot 0 armed again lists nothing
    s0, _, _ = samplers(prompts, first)
    A.gen_disarm(2)
    A.gen_arm(0, first[0], 4, s0, seed=SEED)
    r = A.gen_run(2, top=1)                                              # n_top 1 would be refused if slot 0 still listed 5
    assert (r[0][:, 0] != PAD).all() and np.isnan(r[4][:, 0]).all() and (r[5][:, 0] == NONE).all() and (r[6][:, 0] == -np.inf).all()
    with pytest.raises(rt.RwkvError):
        A.gen_set_topn(0, 33)
    for eng in (A, A0, Bn):
        eng.close()

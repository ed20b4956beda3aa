"""GPU (-m gpu): target tokens scored on the device — `rwkv_score_rows` (the kernel, directly) and `rwkv_infer_score` (the kernel behind the
head GEMM) — against a float64 log-softmax.

Bound, everywhere: |got - want| <= 2e-5 * max(1, |want|), the project's fp32-class bound (include/rwkv_abi.h, Precision::Fp32): one rounding each of
x[t] - m, of the logarithm and of the final subtraction, plus a relative (V / 1024 + log2 1024) * 2^-24 on the sum — together under 1e-5 at
V = 65,536 for |want| <= 32; the relative form covers the rows of large magnitude.  Each test prints the largest error it saw."""
import ctypes as C

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R

pytestmark = pytest.mark.gpu
SKIP = rt.SCORE_SKIP
BOUND = 2e-5


def logp64(row, t):
    """float64 log-softmax of one row at one target"""
    x = np.asarray(row, dtype=np.float64)
    if x[t] == -np.inf:
        return -np.inf
    m = x.max()
    return float((x[t] - m) - np.log(np.exp(x - m).sum()))


def err_of(got, want):
    """error in units of the bound's scale: |got - want| / max(1, |want|); exact agreement for -inf"""
    if np.isinf(want):
        return 0.0 if got == want else np.inf
    return abs(float(got) - want) / max(1.0, abs(want))


def prompt(V, slot, n):
    return [t % V for t in R.synth_prompt(slot, n)]


# ------------------------------------------------------------------------------------------------
# 1. the kernel through rwkv_score_rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [16, 272, 65520, 65536])
def test_kernel_through_score_rows(V):
    # max_batch 2: the softmax staging holds two rows, so a five-row call is processed in pieces
    eng = rt.ModelBuilder(R.st_serialize(R.synth_checkpoint(7, 1, 64, 256, V, seed=77, lora_dims=(32, 32, 32, 32)))).build(max_batch=2, token_chunk_size=16)
    rng = np.random.default_rng(V)
    normal = (rng.standard_normal(V) * 8).astype(np.float32)
    equal = np.full(V, 1.25, np.float32)
    k = V // 2
    spike = normal.copy()
    spike[k] = 1e4                                                   # exp(1e4) overflows: the reference's form gives inf / inf here
    masked = normal.copy()
    masked[::2] = -np.inf
    cases = [(normal, 0), (normal, V - 1), (normal, V // 3), (equal, 0), (equal, V - 1), (spike, k), (spike, (k + 1) % V),
             (masked, 1), (masked, 0), (masked, V - 1 if (V - 1) % 2 else V - 2)]
    worst = 0.0
    singles = []
    for row, t in cases:                                             # one row per call
        got = eng.score_rows([row], [t])
        assert got.shape == (1,) and got.dtype == np.float32
        worst = max(worst, err_of(got[0], logp64(row, t)))
        singles.append(got[0])
    assert singles[3] == singles[4] and abs(float(singles[3]) + np.log(V)) <= BOUND * max(1.0, np.log(V))   # all-equal row: -ln V
    assert singles[8] == -np.inf and np.isfinite(singles[7])        # a masked target is exactly -inf, a finite one next to masked entries is scored
    assert np.isfinite(singles[5]) and np.isfinite(singles[6])      # the spike row stays finite, on and off the spike
    # five rows per call: the same values bit for bit (a row's result does not depend on n_rows or on its neighbours)
    for i0 in (0, 5):
        batch = cases[i0:i0 + 5]
        got = eng.score_rows([r for r, _ in batch], [t for _, t in batch])
        np.testing.assert_array_equal(got.view(np.uint32), np.array(singles[i0:i0 + 5], np.float32).view(np.uint32))
    # RWKV_SCORE_SKIP: not scored, NaN — alone and between scored rows; a row holding +inf or NaN gives NaN
    assert np.isnan(eng.score_rows([normal], [SKIP])[0])
    poisoned, nan_row = normal.copy(), normal.copy()
    poisoned[V - 3] = np.inf
    nan_row[2] = np.nan
    got = eng.score_rows([normal, normal, poisoned, nan_row, normal], [0, SKIP, 0, V - 1, V - 1])
    assert got[0] == singles[0] and np.isnan(got[1]) and np.isnan(got[2]) and np.isnan(got[3]) and got[4] == singles[1]
    # a target >= V that is not the skip value: RWKV_ERR_INVALID, out_logp untouched (the raw call: the wrapper allocates its own output)
    rows = [normal, equal]
    pi = (C.c_void_p * 2)(*[r.ctypes.data for r in rows])
    out = np.full(2, 7.0, np.float32)
    for bad in (V, V + 5, 0xFFFFFFFE):
        tg = np.array([0, bad], np.uint32)
        rc = rt.lib().rwkv_score_rows(eng._h, pi, tg.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(C.c_float)), 2)
        assert rc == -1 and (out == 7.0).all()
    eng.close()
    print(f"score_rows V={V}: max error {worst:.3e} of the bound's scale (bound {BOUND:.0e})")
    assert worst <= BOUND


# ------------------------------------------------------------------------------------------------
# 2. rwkv_infer_score against the Full rows of the same engine
# ------------------------------------------------------------------------------------------------
def run_full(eng, prompts, options):
    """the prompts through rwkv_infer; returns (rows per slot, n_consumed per call)"""
    inp = rt.RnnInput([rt.RnnInputBatch(list(p), o) for p, o in zip(prompts, options)])
    rows, consumed = [[] for _ in prompts], []
    while inp.num_token() > 0:
        before = [len(b.tokens) for b in inp.batches]
        inp, outs = eng.infer(inp)
        consumed.append([n - len(b.tokens) for n, b in zip(before, inp.batches)])
        for b, o in enumerate(outs):
            rows[b].extend(list(o))
    return rows, consumed


def run_scored(eng, prompts, options, targets):
    inp = rt.RnnInput([rt.RnnInputBatch(list(p), o) for p, o in zip(prompts, options)])
    targets = [None if t is None else list(t) for t in targets]
    scores, consumed = [[] for _ in prompts], []
    while inp.num_token() > 0:
        before = [len(b.tokens) for b in inp.batches]
        inp, targets, out = eng.infer_score(inp, targets)
        consumed.append([n - len(b.tokens) for n, b in zip(before, inp.batches)])
        for b, o in enumerate(out):
            scores[b].extend(list(o))
    return scores, consumed


@pytest.mark.parametrize("state_only_slot", [False, True], ids=["all-scored", "slot2-state-only"])
@pytest.mark.parametrize("prec", [rt.Precision.Fp32, rt.Precision.Fp16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", ["v5-tiny", "v6-tiny", "v7-tiny"])
def test_infer_score_against_full_rows_of_the_same_engine(name, prec, state_only_slot):
    eng = rt.ModelBuilder(R.st_serialize(R.synth_named(name))).build(max_batch=3, token_chunk_size=16, precision=prec)
    V = eng.info.num_vocab
    prompts = [prompt(V, 60 + b, n) for b, n in enumerate((11, 18, 27))]          # ragged, straddling calls
    full_opts = [rt.RnnOption.Full, rt.RnnOption.Full, rt.RnnOption.NoOutput if state_only_slot else rt.RnnOption.Full]
    rows, consumed_full = run_full(eng, prompts, full_opts)
    states = [eng.state.back(b) for b in range(3)]
    for b in range(3):
        eng.state.load(eng.state.init(), b)
    # targets: the next token, a token that is not the next one now and then, the skip value on the last row
    targets = [[(p[i + 1] if i % 4 else (p[i] * 7 + 3) % V) for i in range(len(p) - 1)] + [SKIP] for p in prompts]
    if state_only_slot:
        targets[2] = None
    # the option of a scored slot is ignored: hand the scored slots `Last`
    score_opts = [rt.RnnOption.Last, rt.RnnOption.Last, rt.RnnOption.NoOutput if state_only_slot else rt.RnnOption.Last]
    scores, consumed = run_scored(eng, prompts, score_opts, targets)
    assert consumed == consumed_full and len(consumed) >= 4
    worst = 0.0
    for b in range(3):
        if targets[b] is None:
            assert scores[b] == [] and rows[b] == []
            continue
        assert len(scores[b]) == len(prompts[b]) == len(rows[b])
        assert np.isnan(scores[b][-1])
        for i, t in enumerate(targets[b][:-1]):
            worst = max(worst, err_of(scores[b][i], logp64(rows[b][i], t)))
    for b in range(3):
        np.testing.assert_array_equal(eng.state.back(b).view(np.uint32), states[b].view(np.uint32))   # bit-identical state
    # refusals: a slot without targets that wants rows; a target outside the vocabulary (nothing consumed, nothing written)
    inp = rt.RnnInput([rt.RnnInputBatch([1, 2], rt.RnnOption.Last), rt.RnnInputBatch([3], rt.RnnOption.Last), rt.RnnInputBatch()])
    with pytest.raises(rt.RwkvError) as e:
        eng.infer_score(inp, [[2, SKIP], None, None])
    assert e.value.code == -1 and len(inp.batches[0].tokens) == 2
    with pytest.raises(rt.RwkvError) as e:
        eng.infer_score(rt.RnnInput([rt.RnnInputBatch([1, 2]), rt.RnnInputBatch(), rt.RnnInputBatch()]), [[2, V], None, None])
    assert e.value.code == -1
    for b in range(3):
        np.testing.assert_array_equal(eng.state.back(b).view(np.uint32), states[b].view(np.uint32))
    eng.close()
    print(f"infer_score {name} {prec.name} state_only_slot={state_only_slot}: max error {worst:.3e} of the bound's scale (bound {BOUND:.0e})")
    assert worst <= BOUND


# ------------------------------------------------------------------------------------------------
# 3. determinism
# ------------------------------------------------------------------------------------------------
def test_two_slots_with_the_same_work_get_the_same_bits():
    eng = rt.ModelBuilder(R.st_serialize(R.synth_named("v6-tiny"))).build(max_batch=2, token_chunk_size=16, precision=rt.Precision.Fp16)
    V = eng.info.num_vocab
    p = prompt(V, 71, 29)
    tg = p[1:] + [SKIP]
    scores, consumed = run_scored(eng, [p, p], [rt.RnnOption.Full] * 2, [tg, tg])
    assert len(consumed) >= 2 and all(c[0] == c[1] for c in consumed)
    a, b = np.array(scores[0], np.float32), np.array(scores[1], np.float32)
    assert len(a) == 29 and np.isfinite(a[:-1]).all()
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    eng.close()


# ------------------------------------------------------------------------------------------------
# 4. end to end: harness.perplexity_scored, harness.perplexity and the oracle
# ------------------------------------------------------------------------------------------------
def test_perplexity_scored_end_to_end():
    t = R.synth_named("v7-small")
    eng = rt.ModelBuilder(R.st_serialize(t)).build(max_batch=2, token_chunk_size=6, precision=rt.Precision.Fp32)
    ref = R.RwkvRef(t)
    V = ref.info.num_vocab
    loop = H.InferLoop(eng)
    choice = prompt(V, 9, 13)
    # without head
    old = H.perplexity(loop, 0, choice)
    eng.state.load(eng.state.init(), 0)
    new = H.perplexity_scored(loop, 0, choice)
    want = R.perplexity_ref(ref.forward([0] + choice, ref.init_state(), full=True), choice)
    print(f"perplexity (no head): rows {old:.7f}, scored {new:.7f}, oracle {want:.7f}")
    assert abs(new - old) < 1e-4 and abs(new - want) < 1e-4 and abs(old - want) < 1e-4
    # with head: the probability of choice[0] on the prompt's last row, from score_rows
    p = prompt(V, 8, 17)
    eng.state.load(eng.state.init(), 0)
    req = loop.submit(H.InferRequest(0, p, rt.RnnOption.Last))
    loop.run_pending()
    last = req.outputs[-1][-1]
    snap = eng.state.read(0)
    head = float(np.exp(eng.score_rows([last], [choice[0]])[0]))
    s = ref.init_state()
    last_ref = ref.forward(p, s)[-1]
    assert abs(head - float(R.softmax_ref(last_ref)[choice[0]])) <= 1e-4
    old = H.perplexity(loop, 0, choice, head)
    eng.state.write(snap, 0)
    new = H.perplexity_scored(eng, 0, choice, head)
    want = R.perplexity_ref(ref.forward(choice, s, full=True), choice, head)
    print(f"perplexity (head {head:.6f}): rows {old:.7f}, scored {new:.7f}, oracle {want:.7f}")
    assert abs(new - old) < 1e-4 and abs(new - want) < 1e-4 and abs(old - want) < 1e-4
    eng.close()


# ------------------------------------------------------------------------------------------------
# 5. neighbours undisturbed
# ------------------------------------------------------------------------------------------------
def test_scoring_calls_do_not_disturb_last_rows_of_other_slots():
    st = R.st_serialize(R.synth_named("v6-tiny"))
    A = rt.ModelBuilder(st).build(max_batch=2, token_chunk_size=8, precision=rt.Precision.Fp16)
    Bn = rt.ModelBuilder(st).build(max_batch=2, token_chunk_size=8, precision=rt.Precision.Fp16)   # never scores
    V = A.info.num_vocab
    doc = prompt(V, 80, 21)
    pieces = [prompt(V, 81 + i, n) for i, n in enumerate((5, 1, 9, 1))]
    inp = rt.RnnInput([rt.RnnInputBatch(list(doc), rt.RnnOption.Full), rt.RnnInputBatch()])
    targets = [doc[1:] + [SKIP], None]
    for piece in pieces:
        if inp.num_token():
            inp, targets, _ = A.infer_score(inp, targets)
        rows = []
        for eng in (A, Bn):
            last = rt.RnnInput([rt.RnnInputBatch(), rt.RnnInputBatch(list(piece), rt.RnnOption.Last)])
            emitted = []
            while last.num_token():                                  # the 9-token piece straddles two calls at chunk 8
                last, outs = eng.infer(last)
                emitted.extend(list(outs[1]))
            assert len(emitted) == 1 and emitted[0].shape == (V,)    # `Last`: one row, when the piece is exhausted
            rows.append(emitted[0])
        np.testing.assert_array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32))
    np.testing.assert_array_equal(A.state.back(1).view(np.uint32), Bn.state.back(1).view(np.uint32))
    A.close()
    Bn.close()


def test_tokens_through_infer_score_disarm_a_generation_slot():
    eng = rt.ModelBuilder(R.st_serialize(R.synth_named("v6-tiny"))).build(max_batch=2, token_chunk_size=8, precision=rt.Precision.Fp16)
    V = eng.info.num_vocab
    for b in range(2):
        eng.gen_arm(b, 5 + b, 16, H.NucleusSampler(), seed=3)
    inp = rt.RnnInput([rt.RnnInputBatch([7, 8, 9], rt.RnnOption.Full), rt.RnnInputBatch()])
    _, _, scores = eng.infer_score(inp, [[8, 9, SKIP], None])
    assert len(scores[0]) == 3 and np.isfinite(scores[0][:2]).all()
    toks, probs, n_emitted, finish = eng.gen_run(3)
    assert (toks[:, 0] == 0xFFFFFFFF).all() and np.isnan(probs[:, 0]).all() and n_emitted[0] == 0    # nothing in the scored slot's column
    assert n_emitted[1] >= 1 and (toks[:n_emitted[1], 1] < V).all()                                  # the other slot generates
    eng.close()

"""GPU (-m gpu): the engine's graph caches under churn (csrc/graph_cache.h; the policy itself is pinned on the CPU by
tests/test_graph_cache_cpp.py).  The smallest two-layer row of tests/dims_table.py in Precision.Fp32, max_batch 4, token_chunk_size 128.

Step shapes: one slot, option Last, steps of 1..70 tokens, each length twice in a row.  A step's graph key holds its row count, so these are
70 distinct keys: every length runs directly the first time and is captured the second, 70 captures into 64 places, 6 evictions (lengths
1..6, the least recently replayed).  Then lengths 1..6 again (captured again, evicting 7..12) and 65..70 again (replayed from the cache).
The slot's state carries on from call to call, so the logits of every call are checked against the oracle following the same token stream,
within the tolerance tests/test_gpu_dims.py applies to this row: 2e-5 x max(1, |ref|_inf).  Equality with the oracle, not bit-equality between
replays.

Greedy: rwkv_decode_greedy at slot counts 1..4 (one cached graph per count, captured on first sight), twice each from the same loaded
state: the second call's tokens equal the first call's."""
import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import dims_table as D

pytestmark = pytest.mark.gpu
ROW = min((i for i in D.RUN), key=lambda i: (D.TABLE[i].C, D.TABLE[i].F, D.TABLE[i].V, i))     # the smallest row that runs
FP32_TOL = 2e-5                                                   # tests/test_gpu_dims.py
LENGTHS = [n for n in range(1, 71) for _ in range(2)] + list(range(1, 7)) + list(range(65, 71))
GREEDY_STEPS = 8

_REF = {}


def reference():
    """Checkpoint bytes, the token stream, and the oracle's last-row logits of every call; computed once."""
    if not _REF:
        tens = D.tensors(ROW)
        ref = R.RwkvRef(tens)
        V = ref.info.num_vocab
        stream = [t % V for t in R.synth_prompt(7700, sum(LENGTHS))]
        state, want, pos = ref.init_state(), [], 0
        for n in LENGTHS:
            want.append(ref.forward(stream[pos:pos + n], state)[-1])
            pos += n
        _REF.update(st=R.st_serialize(tens), stream=stream, want=want)
    return _REF


def build(st):
    return rt.ModelBuilder(st).build(max_batch=4, token_chunk_size=128, precision=rt.Precision.Fp32)


def test_step_graphs_survive_capture_eviction_recapture_and_replay():
    assert D.TABLE[ROW].C == 64 and D.LAYERS == 2 and len(set(LENGTHS)) == 70 and len(LENGTHS) == 152
    ref = reference()
    eng = build(ref["st"])
    pos, worst, over = 0, 0.0, []
    for call, n in enumerate(LENGTHS):
        inp = rt.RnnInput([rt.RnnInputBatch(list(ref["stream"][pos:pos + n]), rt.RnnOption.Last)] + [rt.RnnInputBatch() for _ in range(3)])
        inp, outs = eng.infer(inp)
        assert inp.num_token() == 0 and len(outs[0]) == 1, (call, n, inp.num_token(), len(outs[0]))
        want = ref["want"][call]
        ratio = float(np.abs(outs[0][-1] - want).max()) / (FP32_TOL * max(1.0, float(np.abs(want).max())))
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            over.append((call, n, ratio))
        pos += n
    eng.close()
    print(f"\n[graph cache] {D.row_id(ROW)} fp32: {len(LENGTHS)} calls, worst logits error / tolerance {worst:.3f}")
    assert not over, f"(call, length, error / tolerance) above 1: {over[:10]} ({len(over)} of {len(LENGTHS)} calls)"


def test_greedy_graphs_replay_what_they_captured():
    ref = reference()
    eng = build(ref["st"])
    V = D.TABLE[ROW].V
    # a state worth decoding from: every slot prefilled with its own prompt, read back once and loaded before every call
    prompts = [[t % V for t in R.synth_prompt(7710 + b, 9 + b)] for b in range(4)]
    inp = rt.RnnInput([rt.RnnInputBatch(p, rt.RnnOption.Last) for p in prompts])
    inp, outs = eng.infer(inp)
    assert inp.num_token() == 0
    first = [int(np.argmax(outs[b][-1])) for b in range(4)]
    states = [eng.state.back(b) for b in range(4)]
    for n in (1, 2, 3, 4):
        got = []
        for _ in range(2):
            for b in range(4):
                eng.state.load(states[b], b)
            toks, _ = eng.decode_greedy(first[:n], GREEDY_STEPS)
            got.append(np.array(toks, copy=True))
        assert got[0].shape == (GREEDY_STEPS, n) and int(got[0].max()) < V
        assert np.array_equal(got[0], got[1]), (n, got[0].T.tolist(), got[1].T.tolist())
    eng.close()

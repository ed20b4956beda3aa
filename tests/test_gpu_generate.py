"""MI355X: device-resident sampled generation (rwkv_gen_arm / rwkv_gen_run, ABI 8) against the per-token path it completes.

Engine A is armed and generates on the device; engine B runs the existing `infer_sample` loop with the host samplers of
`ai00_server_amd.harness` and the uniforms `gen_uniform` restates.  Both run the same kernels on the same logits with the same
rows in every step, so token ids, `out_probs` and states are compared with no tolerance at all.  (The per-token sampler is itself
held to the restated reference samplers in test_gpu_parity.py.)"""
import copy
import os

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF
MODELS = [("v6-small", (3, 1)), ("v7-small", (3, 2))]          # Int8 / NF4 on every layer, default precision
SEED = 20251024


class BiasedMirostat(H.MirostatSampler):
    """Mirostat with `GenerateRequest::bias` (run.rs:681-683 applies it to every sampler): the per-token side passes it as adjustments."""

    def __init__(self, bias=None, **kw):
        super().__init__(**kw)
        self.bias = dict(bias or {})

    def adjustments(self):
        return {t: np.float32(b) for t, b in self.bias.items()}


def build_pair(name, quant, B=3):
    st = R.st_serialize(R.synth_named(name))
    mk = lambda: rt.ModelBuilder(st).quant(quant[0], rt.Quant(quant[1])).build(max_batch=B, token_chunk_size=8, precision=rt.Precision.Fp16)
    return mk(), mk()


def prompt(V, slot, n):
    return [t % V for t in R.synth_prompt(slot, n)]


def prefill(eng, prompts):
    """consume the prompts (slots with an empty list stay untouched); returns the arg-max of each prompt's row as the first token"""
    inp = rt.RnnInput([rt.RnnInputBatch(list(p)) for p in prompts])
    first = [None] * len(prompts)
    while inp.num_token() > 0:
        inp, outs = eng.infer(inp)
        for b, o in enumerate(outs):
            if len(o):
                first[b] = int(np.argmax(o[-1]))
    return first


def samplers(kind, V):
    """slot 0: presence_penalty 0 and a bias that makes repeats certain; slot 1: defaults + bias; slot 2: defaults"""
    bias = {17 % V: 8.0, 401 % V: 7.5}
    if kind == "nucleus":
        return [H.NucleusSampler(top_p=0.8, top_k=32, temperature=1.2, presence_penalty=0.0, frequency_penalty=0.4, bias=bias),
                H.NucleusSampler(bias={5: 3.0, 900 % V: -2.0}), H.NucleusSampler()]
    if kind == "typical":
        return [H.TypicalSampler(tau=0.9, top_k=32, temperature=1.2, presence_penalty=0.0, frequency_penalty=0.4, bias=bias),
                H.TypicalSampler(bias={5: 3.0, 900 % V: -2.0}), H.TypicalSampler()]
    return [BiasedMirostat(bias=bias), BiasedMirostat(bias={5: 3.0, 900 % V: -2.0}, tau=2.0, rate=0.3), BiasedMirostat()]


def per_token(eng, smp, cur, slots, steps, draws, states=None):
    """The existing loop: `steps` calls of infer_sample for `slots`, host samplers updated per token.  `cur[b]` is the token slot b
    consumes next, `draws[b]` its draw counter (both advanced in place).  Returns {slot: [(token, prob)]}; with `states` (a dict)
    the slab of every slot after every step is kept as states[(slot, draw index)]."""
    B = eng.max_batch
    out = {b: [] for b in slots}
    for _ in range(steps):
        us = [rt.gen_uniform(SEED, b, draws[b]) if b in slots else 0.0 for b in range(B)]
        inp = rt.RnnInput([rt.RnnInputBatch([cur[b]] if b in slots else []) for b in range(B)])
        _, res = eng.infer_sample(inp, [smp[b] if b in slots else None for b in range(B)], us)
        for b in slots:
            tok, prob = res[b]
            smp[b].update(prob if getattr(smp[b], "kind", 0) == 2 else tok)
            out[b].append((tok, prob))
            cur[b] = tok
            if states is not None:
                states[(b, draws[b])] = eng.state.back(b)
            draws[b] += 1
    return out


def setup(name, quant, kind, B=3, n_slots=3):
    A, Bn = build_pair(name, quant, B)
    V = A.info.num_vocab
    prompts = [prompt(V, 60 + b, 6 + 3 * b) if b < n_slots else [] for b in range(B)]
    first = prefill(A, prompts)
    assert prefill(Bn, prompts) == first
    smp = samplers(kind, V)
    for b in range(n_slots):
        smp[b].init(prompts[b])
        if kind != "mirostat":
            smp[b].update(first[b])                                  # the prompt's token went through `sample` (nucleus.rs:104-119)
    return A, Bn, V, prompts, first, smp


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", ["nucleus", "typical", "mirostat"])
@pytest.mark.parametrize("name,quant", MODELS)
def test_resident_generation_equals_the_per_token_loop_bit_for_bit(name, quant, kind):
    A, Bn, V, prompts, first, smp = setup(name, quant, kind)
    n = 24
    for b in range(3):
        A.gen_arm(b, first[b], n, copy.deepcopy(smp[b]), seed=SEED)
    toks, probs = [], []
    for steps in (1, 5, 18):                                          # the draw counter and the held token carry over between runs
        t, p, ne, fin = A.gen_run(steps)
        toks.append(t)
        probs.append(p)
        assert list(ne) == [steps] * 3
    toks, probs = np.concatenate(toks), np.concatenate(probs)
    assert list(fin) == [rt.GenFinish.Length] * 3
    want = per_token(Bn, smp, list(first), [0, 1, 2], n, [0, 0, 0])
    for b in range(3):
        wt = [t for t, _ in want[b]]
        assert 0 not in wt, "token 0 would stop the resident side: pick another prompt"
        print(name, kind, "slot", b, wt)
        np.testing.assert_array_equal(toks[:, b], np.array(wt, np.uint32))
        np.testing.assert_array_equal(bits(probs[:, b]), bits([p for _, p in want[b]]))
    t0 = [t for t, _ in want[0]]
    assert len(set(t0)) < len(t0), "slot 0 must repeat a token (presence_penalty = 0: membership, not value)"
    A.close()
    Bn.close()


@pytest.mark.parametrize("name,quant", MODELS)
def test_stops_lengths_padding_and_the_state_rule(name, quant):
    """Ragged max_tokens (3, 7, 24), a stop token on slot 2, two runs (4 + 20 steps).  After each run every slot's state equals the
    per-token engine's after it consumed the same tokens except the last one emitted — running, stopped or out of tokens."""
    A, Bn, V, prompts, first, smp = setup(name, quant, "nucleus")
    # engine B first (it tells which token slot 2 emits at step 5): the rows of each step are the rows engine A will run
    cur, draws, states = list(first), [0, 0, 0], {}
    smp_b = copy.deepcopy(smp)
    w1 = per_token(Bn, smp_b, cur, [0, 1, 2], 4, draws, states)
    w2 = per_token(Bn, smp_b, cur, [1, 2], 20, draws, states)          # slot 0 finished inside the first run
    want = {0: w1[0], 1: w1[1] + w2[1], 2: w1[2] + w2[2]}
    t2 = [t for t, _ in want[2]]
    stop = t2[5]
    limits = [3, 7, t2.index(stop) + 1]
    assert limits[2] > 4, "slot 2 must still run after the first 4 steps (engine B ran it there): pick another prompt"
    for b in range(3):
        assert 0 not in [t for t, _ in want[b]][:limits[b]]
    maxes = [3, 7, 24]
    for b in range(3):
        A.gen_arm(b, first[b], maxes[b], copy.deepcopy(smp[b]), seed=SEED, stop_tokens=[stop] if b == 2 else [])
    t, p, ne, fin = A.gen_run(4)
    e1 = [min(4, limits[b]) for b in range(3)]
    assert list(ne) == e1
    assert list(fin) == [rt.GenFinish.Length, 0, rt.GenFinish.Stop if limits[2] <= 4 else 0]
    for b in range(3):
        np.testing.assert_array_equal(t[:e1[b], b], np.array([x for x, _ in want[b]][:e1[b]], np.uint32))
        assert (t[e1[b]:, b] == PAD).all() and np.isnan(p[e1[b]:, b]).all() and not np.isnan(p[:e1[b], b]).any()
        np.testing.assert_array_equal(A.state.back(b), states[(b, e1[b] - 1)])
    t, p, ne, fin = A.gen_run(20)
    e2 = [0, 3, limits[2] - e1[2]]
    assert list(ne) == e2
    assert list(fin) == [rt.GenFinish.Length, rt.GenFinish.Length, rt.GenFinish.Stop]
    for b in range(3):
        got = t[:, b][t[:, b] != PAD]
        np.testing.assert_array_equal(got, np.array([x for x, _ in want[b]][e1[b]:limits[b]], np.uint32))
        np.testing.assert_array_equal(bits(p[:e2[b], b]), bits([x for _, x in want[b]][e1[b]:limits[b]]))
        assert (t[e2[b]:, b] == PAD).all() and np.isnan(p[e2[b]:, b]).all()
        np.testing.assert_array_equal(A.state.back(b), states[(b, limits[b] - 1)])
    assert int(t[e2[2] - 1, 2]) == stop and limits[2] < 24             # the stop token is the slot's last token
    t, p, ne, fin = A.gen_run(3)                                       # everything finished: nothing moves
    assert (t == PAD).all() and list(ne) == [0, 0, 0] and list(fin) == [2, 2, 1]
    A.close()
    Bn.close()


def test_continuous_batching_a_slot_joins_between_two_runs():
    name, quant = MODELS[0]
    A, Bn, V, prompts, first, smp = setup(name, quant, "nucleus", B=4)
    p3 = prompt(V, 77, 11)
    for b in range(3):
        A.gen_arm(b, first[b], 64, copy.deepcopy(smp[b]), seed=SEED)
    ta, _, _, _ = A.gen_run(4)
    f3 = prefill(A, [[], [], [], p3])[3]                               # rwkv_infer on another slot between two runs
    s3 = H.NucleusSampler()
    s3.init(p3)
    s3.update(f3)
    A.gen_arm(3, f3, 64, copy.deepcopy(s3), seed=SEED)
    tb, _, ne, fin = A.gen_run(8)
    assert list(ne) == [8] * 4 and list(fin) == [0] * 4
    got = np.concatenate([ta, tb])
    want = per_token(Bn, smp, list(first), [0, 1, 2], 12, [0, 0, 0])    # uninterrupted
    for b in range(3):
        np.testing.assert_array_equal(got[:, b], np.array([t for t, _ in want[b]], np.uint32))
    assert (ta[:, 3] == PAD).all()
    assert prefill(Bn, [[], [], [], p3])[3] == f3
    cur = [0, 0, 0, f3]
    w3 = per_token(Bn, {3: s3}, cur, [3], 8, [0, 0, 0, 0])
    np.testing.assert_array_equal(tb[:, 3], np.array([t for t, _ in w3[3]], np.uint32))
    A.close()
    Bn.close()


def test_disarm_rules_and_refusals():
    name, quant = MODELS[0]
    A, Bn, V, prompts, first, smp = setup(name, quant, "nucleus")
    Bn.close()
    t, p, ne, fin = A.gen_run(2)                                        # nothing armed: RWKV_OK, nothing emitted
    assert (t == PAD).all() and np.isnan(p).all() and list(ne) == [0, 0, 0] and list(fin) == [0, 0, 0]
    A.gen_arm(0, first[0], 5, smp[0], seed=SEED)
    A.gen_arm(1, first[1], 5, smp[1], seed=SEED)
    prefill(A, [[3, 4], [], []])                                        # rwkv_infer on an armed slot disarms it
    A.state.load(A.state.back(1), 1)                                    # ... and so does rwkv_state_load
    t, _, ne, _ = A.gen_run(2)
    assert (t == PAD).all() and list(ne) == [0, 0, 0]
    A.gen_arm(2, first[2], 5, smp[2], seed=SEED)
    A.gen_disarm(2)
    assert (A.gen_run(1)[0] == PAD).all()
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm(0, first[0], 5, smp[0], allow=np.ones(V, np.uint8))   # the formatter mask stays with rwkv_infer_sample
    assert e.value.code == -3
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm(0, first[0], 5, H.NucleusSampler(top_k=300))
    assert e.value.code == -3
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm(0, first[0], 5, smp[0], stop_tokens=list(range(1, 10)))
    assert e.value.code == -3
    for bad in (dict(max_tokens=0), dict(first_token=V)):
        with pytest.raises(rt.RwkvError) as e:
            A.gen_arm(0, **{**dict(first_token=first[0], max_tokens=5, sampler=smp[0]), **bad})
        assert e.value.code == -1
    assert (A.gen_run(1)[0] == PAD).all()                               # a refused arm arms nothing
    A.close()


@pytest.mark.parametrize("mode", ["nucleus", "mirostat"])
def test_cpp_decode_loop_resident_prints_the_same_ids(tmp_path, mode):
    """harness/decode_loop.cpp: RWKV_DECODE_RESIDENT=4 (gen_params_for -> Runtime::gen_arm / gen_run) against the same loop per token
    with the same seeded draws."""
    import subprocess
    from ai00_server_amd import build as B
    exe = B.build_harness(verbose=False) if not os.path.exists(B.HARNESS_BIN) else B.HARNESS_BIN
    t = R.synth_named("v6-small")
    path = tmp_path / "m.st"
    path.write_bytes(R.st_serialize(t))
    V = R.RwkvRef(t).info.num_vocab
    p0, p1 = prompt(V, 52, 9), prompt(V, 53, 14)
    args = [exe, str(path), "2", "1", "3", "8", "11"] + [str(x) for x in p0] + ["/"] + [str(x) for x in p1]
    env = dict(os.environ, RWKV_DECODE_SAMPLER=mode, RWKV_DECODE_SEED="7")
    a = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
    b = subprocess.run(args, capture_output=True, text=True, timeout=300, env=dict(env, RWKV_DECODE_RESIDENT="4"))
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    ids = [[int(x) for x in ln.split()] for ln in a.stdout.strip().splitlines()]
    assert len(ids) == 2 and all(len(r) == 11 and 0 not in r for r in ids)
    assert a.stdout == b.stdout

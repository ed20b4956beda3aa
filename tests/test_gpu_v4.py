"""MI355X: RWKV-4 through the C ABI against tests/v4_ref.py (a float64 numpy evaluation of the V4 formulas) and tests/v4_literal.py.

Bounds are the project's (tests/test_gpu_parity.py): logits and state within 1e-3 * max(1, |ref|_inf) in Precision::Fp16 and
2e-5 * max(1, |ref|_inf) in Precision::Fp32; token ids, bytes and everything that is moved rather than computed are exact."""
import copy
import os
import sys

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import v4_ref
from tests.v4_literal import LiteralV4

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_converted_v4 as MC4  # noqa: E402

pytestmark = pytest.mark.gpu
GREEDY_PROMPT_SLOT, GREEDY_PROMPT_LEN, GREEDY_STEPS = v4_ref.GREEDY_RUN

FP16_TOL, FP32_TOL = 1e-3, 2e-5
FP32, FP16 = rt.Precision.Fp32, rt.Precision.Fp16


def tol(prec, want):
    return (FP32_TOL if prec == FP32 else FP16_TOL) * max(1.0, float(np.abs(want).max()))


def err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max())


def build(tensors, prec=FP32, quant=(0, 0), B=2, chunk=16, lora=None):
    b = rt.ModelBuilder(R.st_serialize(tensors)).quant(quant[0], rt.Quant(quant[1]))
    if lora:
        b = b.lora(*lora)
    return b.build(max_batch=B, token_chunk_size=chunk, precision=prec)


def run_prompts(eng, prompts, option=rt.RnnOption.Last):
    """prompts[b] for slot b (an empty list leaves the slot alone); the rows every slot emitted"""
    B = eng.max_batch
    inp = rt.RnnInput([rt.RnnInputBatch(list(prompts[b]) if b < len(prompts) else [], option) for b in range(B)])
    rows = [[] for _ in range(B)]
    while inp.num_token() > 0:
        inp, outs = eng.infer(inp)
        for b, o in enumerate(outs):
            rows[b].extend(list(o))
    return [np.stack(r) if r else np.zeros((0, eng.info.num_vocab), np.float32) for r in rows]


def slab(eng, b):
    """slot b's state as [5L][C]"""
    back = eng.state.back(b)
    assert back.shape == (1, 5 * eng.info.num_layer, eng.info.num_emb)
    return back[0]


def check_slot(eng, b, got_row, ref, p, prec, what=""):
    s = ref.init_state()
    want = ref.forward(p, s)[-1]
    e_l, e_s = err(got_row, want), err(slab(eng, b), s)
    print(f"{what} slot {b}: logits err {e_l:.3e} (bound {tol(prec, want):.3e}), state err {e_s:.3e} (bound {tol(prec, s):.3e})")
    assert np.isfinite(got_row).all() and e_l <= tol(prec, want)
    assert e_s <= tol(prec, s)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v4-tiny", "v4-small"])
@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "fp16"])
def test_prefill_logits_and_full_state_match_v4_ref(name, prec):
    """B = 3, chunk 16, prompts of 11, 18 and 25 tokens: sequences of several rows that straddle steps, ragged, and a last step with one slot"""
    t = v4_ref.synth_v4(name)
    eng = build(t, prec, B=3, chunk=16)
    ref = v4_ref.V4Ref(t)
    assert int(eng.info.version) == 4 and eng.state.shape == (ref.info.num_emb, 5 * ref.info.num_layer, 1, 1)
    ps = [v4_ref.prompt(ref.info.num_vocab, s, 11 + 7 * s) for s in range(3)]
    got = run_prompts(eng, ps)
    for b in range(3):
        assert got[b].shape == (1, ref.info.num_vocab)
        check_slot(eng, b, got[b][0], ref, ps[b], prec, f"{name} {prec.name}")
    eng.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
def test_greedy_ids_identical_over_many_steps():
    """96 greedy steps through InferLoop in Precision::Fp16, then 40 through rwkv_decode_greedy: the ids of v4_ref.greedy (tests/test_v4_cpu.py
    shows that no step of this run hangs on a margin fp32 cannot resolve)"""
    t = v4_ref.synth_v4("v4-tiny")
    ref = v4_ref.V4Ref(t)
    p = v4_ref.prompt(ref.info.num_vocab, GREEDY_PROMPT_SLOT, GREEDY_PROMPT_LEN)
    want, _ = ref.greedy(p, GREEDY_STEPS)
    eng = build(t, FP16, B=2, chunk=16)
    loop = H.InferLoop(eng)
    toks, got = list(p), []
    for _ in range(GREEDY_STEPS):
        req = loop.submit(H.InferRequest(0, toks, rt.RnnOption.Last))
        loop.run_pending()
        got.append(int(np.argmax(req.outputs[-1][-1])))
        toks = [got[-1]]
    print("greedy ids", got)
    assert got == want
    # device-resident: slot 0 of a fresh state takes the prompt, its first id starts the loop
    eng.state.load(eng.state.init(), 0)
    row = run_prompts(eng, [p])[0][-1]
    assert int(np.argmax(row)) == want[0]
    ids, _ = eng.decode_greedy([want[0]], 40)
    assert [int(x) for x in ids[:, 0]] == want[1:41]
    eng.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
def test_step_form_does_not_matter():
    """One 23-token prompt three ways: chunk 1 (wkv4_kernel only), chunk 8 (wkv4_chunk_kernel, three steps), chunk 32 with both neighbour slots busy
    (one step, three sequences).  Each meets the Fp32 bound against the oracle, and a second run of the same steps gives the same bits."""
    t = v4_ref.synth_v4("v4-tiny")
    ref = v4_ref.V4Ref(t)
    V = ref.info.num_vocab
    p = v4_ref.prompt(V, 7, 23)
    for chunk, B, others in [(1, 1, False), (8, 1, False), (32, 3, True)]:
        eng = build(t, FP32, B=B, chunk=chunk)
        b = 1 if others else 0
        ps = [v4_ref.prompt(V, 8, 4), p, v4_ref.prompt(V, 9, 5)] if others else [p]
        runs = []
        for _ in range(2):
            for s in range(B):
                eng.state.load(eng.state.init(), s)
            row = run_prompts(eng, ps)[b][-1]
            runs.append((row.copy(), slab(eng, b).copy()))
        check_slot(eng, b, runs[1][0], ref, p, FP32, f"chunk {chunk}")
        np.testing.assert_array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
        np.testing.assert_array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32))
        eng.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quant", [(3, 1), (2, 2)], ids=["int8-all", "nf4-first-two"])
def test_quantised_layers_match_v4_ref_with_the_same_quantisation(quant):
    t = v4_ref.synth_v4("v4-small")
    eng = build(t, FP32, quant=quant, B=2, chunk=16)
    ref = v4_ref.V4Ref(t, quant_layers=quant[0], quant_type=quant[1])
    p = v4_ref.prompt(ref.info.num_vocab, 11, 21)
    got = run_prompts(eng, [p])[0][-1]
    check_slot(eng, 0, got, ref, p, FP32, f"quant {quant}")
    plain = v4_ref.V4Ref(t).forward(p, v4_ref.V4Ref(t).init_state())[-1]
    assert err(got, plain) > 1e-4                                   # the quantisation was applied
    eng.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_state_plumbing_is_exact():
    t = v4_ref.synth_v4("v4-tiny")
    eng = build(t, FP32, B=3, chunk=16)
    L, C = eng.info.num_layer, eng.info.num_emb
    init = eng.state.init()
    assert init.shape == (1, 5 * L, C)
    want = np.zeros((5 * L, C), np.float32)
    want[3::5] = np.float32(-1e30)
    np.testing.assert_array_equal(init[0].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(slab(eng, 2).view(np.uint32), want.view(np.uint32))    # a slot nobody touched holds the initial state
    rng = np.random.default_rng(3)
    s = rng.standard_normal((1, 5 * L, C)).astype(np.float32)
    s[0, 3::5] = rng.uniform(-40, 40, size=(L, C)).astype(np.float32)
    eng.state.load(s, 1)
    np.testing.assert_array_equal(eng.state.back(1).view(np.uint32), s.view(np.uint32))
    snap = eng.state.read(1)
    eng.state.write(snap, 2)
    np.testing.assert_array_equal(eng.state.back(2).view(np.uint32), s.view(np.uint32))
    for l in range(L):
        rows = eng.state.embed(l, 1)
        assert rows.shape == (3, C)
        np.testing.assert_array_equal(rows.view(np.uint32), s[0, 5 * l + 1:5 * l + 4].view(np.uint32))
    with pytest.raises(rt.RwkvError) as e:
        eng.read_state(R.st_serialize({"blocks.0.att.time_state": np.zeros((1, 64, 64), np.float16)}))
    assert e.value.code == -3
    # pp = -FLT_MAX is the same initial state as pp = -1e30
    p = v4_ref.prompt(eng.info.num_vocab, 12, 9)
    a = run_prompts(eng, [p])[0][-1]
    fm = init.copy()
    fm[0, 3::5] = -np.finfo(np.float32).max
    eng.state.load(fm, 0)
    b = run_prompts(eng, [p])[0][-1]
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    eng.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------
def range_variant():
    """v4-tiny with keys of magnitude up to about 60 (exp(k) alone overflows fp32 at 88.7 and the sums of it much earlier: a WKV-4 without the
    running maximum fails), decays from exp(-8) to exp(5) per token and bonuses u in [-5, 5]"""
    t = v4_ref.synth_v4("v4-tiny")
    rng = np.random.default_rng(17)
    C = t["emb.weight"].shape[1]
    for l in range(2):
        p = f"blocks.{l}.att."
        t[p + "key.weight"] = (t[p + "key.weight"].astype(np.float32) * np.float32(36.0)).astype(np.float16)
        t[p + "time_decay"] = rng.uniform(-8, 5, size=C).astype(np.float16)
        t[p + "time_first"] = rng.uniform(-5, 5, size=C).astype(np.float16)
    return t


def test_range_large_keys_and_wide_decays():
    t = range_variant()
    ref = v4_ref.V4Ref(t)
    p = v4_ref.prompt(ref.info.num_vocab, 13, 40)
    eng = build(t, FP32, B=1, chunk=16)
    got = run_prompts(eng, [p], rt.RnnOption.Full)[0]
    s = ref.init_state()
    want = ref.forward(p, s, full=True)
    print(f"range: max |k| {ref.k_absmax:.1f}, logits err {err(got, want):.3e} (bound {tol(FP32, want):.3e}), "
          f"state err {err(slab(eng, 0), s):.3e} (bound {tol(FP32, s):.3e})")
    assert 50.0 <= ref.k_absmax <= 88.0                            # the case is the one it claims to be
    assert np.isfinite(got).all() and np.isfinite(slab(eng, 0)).all()
    assert err(got, want) <= tol(FP32, want)
    assert err(slab(eng, 0), s) <= tol(FP32, s)
    eng.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------
def test_prefab_round_trip_is_bit_exact(tmp_path):
    t = v4_ref.synth_v4("v4-small")
    eng = build(t, FP16, quant=(3, 1), B=2, chunk=16)
    p = v4_ref.prompt(eng.info.num_vocab, 14, 19)
    a, sa = run_prompts(eng, [p])[0], eng.state.back(0)
    path = str(tmp_path / "v4.prefab")
    eng.save_prefab(path)
    info, wb = eng.info, eng.weight_bytes
    eng.close()
    image = open(path, "rb").read()
    assert image[:7] == b"RWKVHIP" and rt.Loader.info(image) == info and int(info.version) == 4
    eng2 = rt.ModelBuilder(image).build(max_batch=2, token_chunk_size=16, precision=FP16)
    assert eng2.info == info and eng2.weight_bytes == wb
    np.testing.assert_array_equal(a.view(np.uint32), run_prompts(eng2, [p])[0].view(np.uint32))
    np.testing.assert_array_equal(sa.view(np.uint32), eng2.state.back(0).view(np.uint32))
    eng2.close()
    lora = R.st_serialize({"blocks.0.att.key.lora.0": np.zeros((256, 4), np.float16), "blocks.0.att.key.lora.1": np.zeros((256, 4), np.float16)})
    with pytest.raises(rt.RwkvError) as e:
        rt.ModelBuilder(image).lora(lora, 0.5).build(max_batch=1)
    assert e.value.code == -3


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------
def test_lora_blend_at_load():
    t = v4_ref.synth_v4("v4-tiny")
    _, L, C, F, V = v4_ref.CONFIGS["v4-tiny"]
    rng = np.random.default_rng(8)
    f16 = lambda *shape: (rng.standard_normal(shape) * 0.05).astype(np.float16)
    lora = {"blocks.0.att.key.lora.0": f16(C, 8), "blocks.0.att.key.lora.1": f16(C, 8),             # [in, r], [out, r]
            "blocks.1.ffn.value.lora.0": f16(F, 8), "blocks.1.ffn.value.lora.1": f16(C, 8)}
    eng = build(t, FP32, B=1, chunk=16, lora=(R.st_serialize(lora), 0.7))
    ref = v4_ref.V4Ref(v4_ref.blend_lora(t, lora, 0.7))
    p = v4_ref.prompt(V, 15, 17)
    got = run_prompts(eng, [p])[0][-1]
    check_slot(eng, 0, got, ref, p, FP32, "lora")
    plain = v4_ref.V4Ref(t)
    assert err(got, plain.forward(p, plain.init_state())[-1]) > 1e-3   # the adapters did something
    eng.close()


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------
def test_scoring_on_the_device_matches_the_oracles_log_softmax():
    t = v4_ref.synth_v4("v4-tiny")
    ref = v4_ref.V4Ref(t)
    V = ref.info.num_vocab
    p, tg = v4_ref.prompt(V, 16, 9), v4_ref.prompt(V, 17, 9)
    eng = build(t, FP32, B=2, chunk=16)
    inp = rt.RnnInput([rt.RnnInputBatch(list(p), rt.RnnOption.Full), rt.RnnInputBatch()])
    _, _, scores = eng.infer_score(inp, [list(tg), None])
    rows = ref.forward(p, ref.init_state(), full=True)
    m = rows.max(axis=1, keepdims=True)
    logp = rows - m - np.log(np.exp(rows - m).sum(axis=1, keepdims=True))
    want = logp[np.arange(9), tg]
    got = np.asarray(scores[0], np.float64)
    print("score err", np.abs(got - want).max())
    assert got.shape == (9,) and np.all(np.abs(got - want) <= 2e-5 * np.maximum(1.0, np.abs(want)))
    eng.close()


def test_resident_generation_equals_the_per_token_loop_bit_for_bit():
    """rwkv_gen_arm + rwkv_gen_run (Nucleus, 16 steps, seeded) against a loop of rwkv_infer_sample fed by rwkv_gen_uniform: tokens and probability bits"""
    t = v4_ref.synth_v4("v4-tiny")
    V = v4_ref.CONFIGS["v4-tiny"][4]
    seed, n = 20251024, 16
    p = v4_ref.prompt(V, 18, 10)
    A, Bn = build(t, FP16, B=2, chunk=8), build(t, FP16, B=2, chunk=8)
    first = int(np.argmax(run_prompts(A, [p])[0][-1]))
    assert int(np.argmax(run_prompts(Bn, [p])[0][-1])) == first
    smp = H.NucleusSampler(top_p=0.8, top_k=32, temperature=1.2)
    smp.init(p)
    smp.update(first)
    A.gen_arm(0, first, n, copy.deepcopy(smp), seed=seed)
    toks, probs, ne, fin = A.gen_run(n)
    cur, want = first, []
    for i in range(n):
        inp = rt.RnnInput([rt.RnnInputBatch([cur]), rt.RnnInputBatch()])
        _, res = Bn.infer_sample(inp, [smp, None], [rt.gen_uniform(seed, 0, i), 0.0])
        cur, prob = res[0]
        smp.update(cur)
        want.append((cur, prob))
        if cur == 0:
            break
    k = len(want)                                                   # token 0 stops the resident side too (run.rs:855)
    print("sampled", [tk for tk, _ in want])
    assert int(ne[0]) == k
    np.testing.assert_array_equal(toks[:k, 0], np.array([tk for tk, _ in want], np.uint32))
    np.testing.assert_array_equal(probs[:k, 0].view(np.uint32), np.array([pr for _, pr in want], np.float32).view(np.uint32))
    np.testing.assert_array_equal(A.state.back(0).view(np.uint32), Bn.state.back(0).view(np.uint32))
    A.close()
    Bn.close()


# ---- 10 ---------------------------------------------------------------------------------------------------------------------------
def test_engine_loads_the_reference_converters_v4_file():
    with open(MC4.FIXTURE, "rb") as f:
        eng = rt.ModelBuilder(f.read()).build(max_batch=2, token_chunk_size=8, precision=FP32)
    lit = LiteralV4(MC4.source())
    toks = v4_ref.prompt(eng.info.num_vocab, 22, 19)
    ls = lit.new_state()
    want = np.stack([lit.forward(tk, ls) for tk in toks])
    got = run_prompts(eng, [toks], rt.RnnOption.Full)[0]
    s = lit.to_slab_order(ls)
    print(f"converted: logits err {err(got, want):.3e}, state err {err(slab(eng, 0), s):.3e}")
    assert got.shape == want.shape and err(got, want) <= tol(FP32, want)
    assert err(slab(eng, 0), s) <= tol(FP32, s)
    eng.close()

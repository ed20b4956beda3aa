"""GPU (-m gpu): `rwkv_infer_score_fused` (head_score_kernel: target tokens scored inside the head GEMM, no logits array) against the float64
log-softmax of the ORACLE's logits for the same prompt, in units of max(1, |want|).  Bounds (profiles/r19_score_fused_errors.jsonl):
PLAIN[prec] is the largest error of the plain path, `rwkv_infer_score`, measured against this very reference on the cases of test 1; the fused path,
the same arithmetic class in another reduction tree, is allowed twice that, under Fp32 never less than the plain path's documented 2e-5.
C = 64 is one K chunk of the kernel, C = 192 three: the chunk index and the parity of the double buffer part ways."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import v4_ref

pytestmark = pytest.mark.gpu
SKIP, FP32, FP16 = rt.SCORE_SKIP, rt.Precision.Fp32, rt.Precision.Fp16
T = 64                                              # head_score_kernel's row-tile height (HEAD_SCORE_ROWS); steps above it run 128-row tiles
SPLIT = 256                                         # columns of a block's split range at V = 65536 (two 128-column strip groups); a strip is 16
PLAIN = {FP32: 1.65e-7, FP16: 8.14e-5}              # measured maxima of rwkv_infer_score over the 24 cases of each precision (MI355X)
BOUND = {FP32: max(2e-5, 2 * PLAIN[FP32]), FP16: 2 * PLAIN[FP16]}


@functools.lru_cache(maxsize=None)
def model(version, V, emb=192, row=None, scale=256):
    """(safetensors bytes, oracle) of the small synthetic model; `row`: that head row times `scale`.  256 takes its logit past 88 (to ~340) and no
    further: the factor also multiplies the fp32 error the operand arrives with, in both paths alike (at 2048 rwkv_infer_score itself is 2.0e-5 off)"""
    if version == 4:                                                 # RWKV-4 has its own synthetic checkpoint and float64 reference
        t = v4_ref.synth_checkpoint_v4(1, emb, 256, V, seed=1904)
    else:
        t = R.synth_checkpoint(version, 1, emb, 256, V, seed=1900 + version, lora_dims=(32, 32, 32, 32) if version == 7 else None)
    if row is not None:
        t["head.weight"][row] *= np.float16(scale)
    return R.st_serialize(t), (v4_ref.V4Ref(t) if version == 4 else R.RwkvRef(t))


@functools.lru_cache(maxsize=None)
def reference(version, V, slot, n, emb=192, row=None):
    """(prompt, float64 log-softmax rows [n][V]) of the oracle from the initial state; read-only"""
    ref = model(version, V, emb, row)[1]
    p = [t % V for t in R.synth_prompt(slot, n)]
    x = ref.forward(p, ref.init_state(), full=True).astype(np.float64)
    x -= x.max(axis=1, keepdims=True)
    lp = x - np.log(np.exp(x).sum(axis=1, keepdims=True))
    lp.setflags(write=False)
    return p, lp


def run(eng, prompts, targets, fused=True, options=None):
    """from the initial state, the prompts through infer_score[_fused] until they are consumed: (scores per slot, calls made)"""
    for b in range(len(prompts)):
        eng.state.load(eng.state.init(), b)
    options = options or [rt.RnnOption.Full] * len(prompts)
    inp = rt.RnnInput([rt.RnnInputBatch(list(p), o) for p, o in zip(prompts, options)])
    targets = [None if t is None else list(t) for t in targets]
    scores, calls = [[] for _ in prompts], 0
    while inp.num_token() > 0:
        inp, targets, out = (eng.infer_score_fused if fused else eng.infer_score)(inp, targets)
        calls += 1
        for b, o in enumerate(out):
            scores[b].extend(list(o))
    return [np.array(s, np.float32) for s in scores], calls


def worst_error(got, lp, targets):
    """largest |got - want| / max(1, |want|) over the scored rows; skipped rows must be NaN, scored ones finite"""
    for i, t in enumerate(targets):
        assert np.isnan(got[i]) if t == SKIP else np.isfinite(got[i]), (i, t, got[i])
    return max([abs(float(got[i]) - lp[i, t]) / max(1.0, abs(lp[i, t])) for i, t in enumerate(targets) if t != SKIP], default=0.0)


@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "default"])
@pytest.mark.parametrize("V,emb", [(16, 64), (272, 64), (65520, 64), (65536, 64), (272, 192), (65536, 192)])
@pytest.mark.parametrize("version", [4, 5, 6, 7])
def test_against_float64_of_the_oracle(version, V, emb, prec):
    eng = rt.ModelBuilder(model(version, V, emb)[0]).build(max_batch=1, token_chunk_size=16, precision=prec)
    p, lp = reference(version, V, 30 + version, 21, emb)             # two calls at chunk 16
    # next tokens; then 0, V - 1 and the edges of a strip, of a strip group and of a block's split range; the skip value on the last row
    edges = [0, V - 1, 15, 16, 127, 128, SPLIT - 1, SPLIT, V - SPLIT, V - SPLIT - 1, V - 16, V - 17]
    tg = p[1:5] + [e % V for e in edges] + p[5 + len(edges):] + [SKIP]
    plain, _ = run(eng, [p], [tg], fused=False)
    fused, calls = run(eng, [p], [tg])
    again, _ = run(eng, [p], [tg])                                   # both step shapes replayed from their captured graphs
    eng.close()
    assert calls == 2 and len(fused[0]) == len(p) == len(tg)
    np.testing.assert_array_equal(again[0].view(np.uint32), fused[0].view(np.uint32))
    e_plain, e_fused = worst_error(plain[0], lp, tg), worst_error(fused[0], lp, tg)
    print(json.dumps({"test": "against_float64", "version": version, "V": V, "C": emb, "precision": prec.name, "plain": e_plain, "fused": e_fused,
                      "ratio_to_bound": e_fused / BOUND[prec]}))
    assert e_fused <= BOUND[prec]


@pytest.mark.parametrize("lengths", [(1,), (T - 1,), (T,), (T + 1,), (2 * T + 3,), (5, T - 24, T + 6), (2 * T + 30,)],
                         ids=["1", "T-1", "T", "T+1", "2T+3", "three-slots", "longer-than-chunk"])
def test_row_tile_and_split_edges(lengths):
    V = 272                                                          # 17 strips: two whole groups and one strip of a third, three splits
    eng = rt.ModelBuilder(model(6, V)[0]).build(max_batch=3, token_chunk_size=2 * T + 8, precision=FP32)
    refs = [reference(6, V, 50 + b, n) for b, n in enumerate(lengths)] + [([], None)] * (3 - len(lengths))
    targets = [(p[1:] + [SKIP]) if p else None for p, _ in refs]
    got, calls = run(eng, [p for p, _ in refs], targets)
    eng.close()
    assert calls == (2 if sum(lengths) > 2 * T + 8 else 1)
    worst = max(worst_error(got[b], lp, targets[b]) for b, (p, lp) in enumerate(refs) if p)
    print(f"row tiles {lengths}: max error {worst:.3e} of the bound's scale (bound {BOUND[FP32]:.1e}, ratio {worst / BOUND[FP32]:.3f})")
    assert worst <= BOUND[FP32]


@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "default"])
def test_a_rows_bits_do_not_depend_on_its_company(prec):
    V = 65520
    eng = rt.ModelBuilder(model(7, V)[0]).build(max_batch=3, token_chunk_size=3 * T, precision=prec)
    (p0, _), (p1, _), (p2, _) = (reference(7, V, 60 + b, n) for b, n in enumerate((T + 9, 17, 23)))
    tg = [p[1:] + [SKIP] for p in (p0, p1, p2)]
    none, full = rt.RnnOption.NoOutput, rt.RnnOption.Full
    # the subject rides in slot 1: alone (rows 0 .., 64-row tile), beside two scored slots (rows T + 9 .., 128-row tiles), beside a state-only slot
    arrangements = [([[], p1, []], [None, tg[1], None], [full] * 3), ([p0, p1, p2], tg, [full] * 3), ([p0, p1, []], [None, tg[1], None], [none, full, full])]
    results, states = [], {}
    for fused in (True, False):
        for k, (prompts, targets, options) in enumerate(arrangements):
            got, calls = run(eng, prompts, targets, fused=fused, options=options)
            assert calls == 1
            states[fused, k] = [eng.state.back(b) for b in range(3)]
            if fused:
                results.append(got[1])
    eng.close()
    assert np.isfinite(results[0][:-1]).all()
    for other in results[1:]:
        np.testing.assert_array_equal(other.view(np.uint32), results[0].view(np.uint32))
    for k in range(3):                                               # every slot's state: what rwkv_infer_score leaves, bit for bit
        np.testing.assert_array_equal(np.stack(states[True, k]).view(np.uint32), np.stack(states[False, k]).view(np.uint32))


def test_an_out_of_range_target_is_refused_with_the_outputs_untouched():
    V = 272
    eng = rt.ModelBuilder(model(5, V)[0]).build(max_batch=2, token_chunk_size=16)
    toks, out, before = np.array([1, 2, 3], np.uint32), np.full(3, 7.0, np.float32), eng.state.back(0)
    ins, tp, op = (rt._SlotInC * 2)(), (C.POINTER(C.c_uint32) * 2)(), (C.POINTER(C.c_float) * 2)()
    ins[0] = rt._SlotInC(toks.ctypes.data_as(C.POINTER(C.c_uint32)), 3, int(rt.RnnOption.Full), 0)
    op[0] = out.ctypes.data_as(C.POINTER(C.c_float))
    for bad in (V, V + 5, 0xFFFFFFFE):
        tg = np.array([0, bad, SKIP], np.uint32)
        tp[0] = tg.ctypes.data_as(C.POINTER(C.c_uint32))
        consumed = (C.c_size_t * 2)(9, 9)
        assert rt.lib().rwkv_infer_score_fused(eng._h, ins, tp, op, consumed) == -1
        assert (out == 7.0).all() and consumed[0] == 0
    np.testing.assert_array_equal(eng.state.back(0).view(np.uint32), before.view(np.uint32))
    eng.close()


@pytest.mark.parametrize("version,scale", [(5, 256), (7, 256), (6, np.nan), (6, np.inf)])
def test_logits_beyond_88_score_finitely_and_inf_or_nan_logits_as_nan(version, scale):
    V, k = 272, 100
    eng = rt.ModelBuilder(model(version, V, row=k, scale=scale)[0]).build(max_batch=1, token_chunk_size=T + 16, precision=FP32)
    p, lp = reference(version, V, 70, T + 6, row=k if np.isfinite(scale) else None)   # a 128-row tile step; the poisoned models need the prompt only
    on, off = [k] * len(p), [(k + 1 + i) % V for i in range(len(p))]
    got = [run(eng, [p], [tg])[0][0] for tg in (on, off)]
    eng.close()
    if not np.isfinite(scale):                                       # the head row is NaN, or +inf against channels of both signs: NaN on and off the token
        assert np.isnan(got[0]).all() and np.isnan(got[1]).all()
        return
    gap = -np.sort(lp, axis=1)[:, -2].min()                          # how far the scaled logit stands above the rest of its row, at most
    assert gap > 88, "the scaled head row must take a logit past 88"
    worst = max(worst_error(got[0], lp, on), worst_error(got[1], lp, off))
    print(f"large logits v{version}: logit gap {gap:.1f}, max error {worst:.3e} of the bound's scale (bound {BOUND[FP32]:.1e}, ratio {worst / BOUND[FP32]:.3f})")
    assert worst <= BOUND[FP32]

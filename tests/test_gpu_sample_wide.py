"""MI355X: on-device sampling over the whole vocabulary — `sample_wide_kernel`, the rows `nucleus_kernel` cannot hold: Nucleus / Typical
with top_k > 256 (nucleus.rs:71-101, typical.rs:70-120 `take(top_k)` for any top_k) and Mirostat whose max_surprise admits 8192
candidates or more (mirostat.rs:55-74).

Everything is held to oracle/rwkv_ref.py's `nucleus_ref` / `typical_ref` / `mirostat_ref` ON THE DEVICE'S OWN LOGITS: the row is read
with rwkv_infer, the state is put back, then the device samples (as test_gpu_parity.py does).  Models, smallest that reach the code:
  M65536  synth_checkpoint(6, 1, 128, 448, 65536, seed=5), head.weight x 8 / x 4 / x 1 (powers of two: exact in f16).  On the oracle's
          row: x 8 reaches mass 0.9 with 351 tokens; x 4 with 15 619 (two windows) and has 10 541 tokens at p >= 2^-16; x 1 is nearly
          flat, 26 465 tokens at p >= 2^-16.
  M20000  synth_checkpoint(6, 1, 128, 448, 20000): the bounded instantiation, a partial last window.
  v6-tiny V = 512: one partial window, V < 8192.
Rules: an id must equal the oracle's when the oracle's margin (distance of the decisive CDF comparison) exceeds 1e-4 (Mirostat: 1e-5, as
in test_gpu_parity.py), and at most a third of a setting's draws may fall under the margin.  Where the CDF steps are ~1e-5 (deep picks)
the margin rule would skip everything; there the token must sit at a position i of the oracle's kept set with
c[i-1] - 1e-4 <= u <= c[i] + 1e-4 (c: the oracle's fp32 cumulative), nothing skipped, and out_prob within 1e-3 relative.
Resident generation is compared with the per-token loop bit for bit, as test_gpu_generate.py does."""
import copy

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF
SEED = 20251201
B = 4
_CTX = {}


class Ctx:
    """one engine per model, the prompt, the device's logits row of the prompt and its softmax (computed once, never changed)"""

    def __init__(self, tens):
        self.V = int(tens["head.weight"].shape[0])
        self.p = [int(t) % self.V for t in R.synth_prompt(90, 5)]
        self.eng = rt.ModelBuilder(R.st_serialize(tens)).build(max_batch=B, token_chunk_size=32, precision=rt.Precision.Fp32)
        _, outs = self.eng.infer(rt.RnnInput([rt.RnnInputBatch(list(self.p))] + [rt.RnnInputBatch() for _ in range(B - 1)]))
        self.row = np.array(outs[0][-1], np.float32)
        self.probs = R.softmax_ref(self.row[None])[0]
        self.probs.setflags(write=False)

    def sample(self, smps, us):
        """smps[b] (or None) samples the prompt's row in slot b, every slot from the initial state: the rows are the row read above"""
        for b in range(B):
            self.eng.state.load(self.eng.state.init(), b)
        inp = rt.RnnInput([rt.RnnInputBatch(list(self.p) if smps[b] is not None else []) for b in range(B)])
        _, out = self.eng.infer_sample(inp, list(smps), list(us))
        return out

    def one(self, smp, u):
        return self.sample([smp, None, None, None], [u, 0.0, 0.0, 0.0])[0]


def m65536(scale):
    t = R.synth_checkpoint(6, 1, 128, 448, 65536, seed=5)
    t["head.weight"] = t["head.weight"] * np.asarray(scale, t["head.weight"].dtype)
    return t


def ctx(name):
    if name not in _CTX:
        _CTX[name] = Ctx({"x8": lambda: m65536(8), "x4": lambda: m65536(4), "x1": lambda: m65536(1),
                          "m20000": lambda: R.synth_checkpoint(6, 1, 128, 448, 20000), "v512": lambda: R.synth_named("v6-tiny")}[name]())
    return _CTX[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for c in _CTX.values():
        c.eng.close()
    _CTX.clear()


def nucleus(top_k, top_p, temp):
    return H.NucleusSampler(top_p=top_p, top_k=top_k, temperature=temp, presence_penalty=0.0, frequency_penalty=0.0)


def typical(top_k, tau, temp):
    return H.TypicalSampler(tau=tau, top_k=top_k, temperature=temp, presence_penalty=0.0, frequency_penalty=0.0)


def mirostat(max_surprise):
    s = H.MirostatSampler()
    s.max_surprise = np.float32(max_surprise)
    return s


# ---- 1. exact ids (M65536 x 8): the draws land in the head of the distribution, where the CDF steps are far above the margin ----------
NUCLEUS = [(1024, 0.95, 1.0), (4096, 0.99, 0.8), (20000, 0.9, 1.0), (65536, 2.0, 1.3)]   # the last walks the whole vocabulary, both passes
TYPICAL = [(1024, 0.9, 1.0), (20000, 0.95, 0.8), (65536, 2.0, 1.2)]
N_NUC, N_TYP = 8, 6
U_NUC = np.random.default_rng(11).random((len(NUCLEUS), N_NUC))     # drawn in the order the settings are listed
U_TYP = np.random.default_rng(12).random((len(TYPICAL), N_TYP))


@pytest.mark.parametrize("i", range(len(NUCLEUS)), ids=[str(s) for s in NUCLEUS])
def test_nucleus_top_k_above_256_exact_ids(i):
    c = ctx("x8")
    top_k, top_p, temp = NUCLEUS[i]
    checked = skipped = 0
    for u in U_NUC[i]:
        want, margin = R.nucleus_ref(c.probs, top_p, top_k, temp, float(u))
        got = c.one(nucleus(top_k, top_p, temp), float(u))
        print(NUCLEUS[i], "u", float(u), "got", got, "want", want, "margin", margin)
        if margin > 1e-4:
            assert got[0] == want, (NUCLEUS[i], float(u), got, want, margin)
            assert abs(got[1] - float(c.probs[want])) <= 1e-3 * float(c.probs[want])
            checked += 1
        else:
            skipped += 1
    assert 3 * skipped <= N_NUC, (checked, skipped)


@pytest.mark.parametrize("i", range(len(TYPICAL)), ids=[str(s) for s in TYPICAL])
def test_typical_top_k_above_256_exact_ids(i):
    c = ctx("x8")
    top_k, tau, temp = TYPICAL[i]
    checked = skipped = 0
    for u in U_TYP[i]:
        alts = [R.typical_ref(c.probs, tau, top_k, temp, float(u), h_shift=d) for d in (0.0, 1e-5, -1e-5, 4e-5, -4e-5)]   # H: a 65k-term fp32 sum
        want, margin = {a[0] for a in alts}, min(a[1] for a in alts)
        got = c.one(typical(top_k, tau, temp), float(u))
        print(TYPICAL[i], "u", float(u), "got", got, "want", want, "margin", margin)
        if margin > 1e-4:
            assert got[0] in want, (TYPICAL[i], float(u), got, want, margin)
            checked += 1
        else:
            skipped += 1
    assert 3 * skipped <= N_TYP, (checked, skipped)


# ---- 2. deep picks: the interval rule ----------------------------------------------------------------------------------------------
def nucleus_kept(probs, top_p, top_k, temp):
    """the kept set of `nucleus_ref` in rank order and its fp32 cumulative c (the same operations; np.cumsum adds in sequence)"""
    p = probs.astype(np.float32)
    order = np.lexsort((np.arange(p.size), -p))[:top_k]
    before = np.concatenate([[np.float32(0)], np.cumsum(p[order], dtype=np.float32)[:-1]])
    stop = np.nonzero(before > np.float32(top_p))[0]
    kept = order[:int(stop[0])] if stop.size else order
    q = np.power(p[kept], np.float32(1.0 / temp), dtype=np.float32)
    s = np.cumsum(q, dtype=np.float32)[-1]
    return kept, np.cumsum((q / s).astype(np.float32), dtype=np.float32)


@pytest.mark.parametrize("model", ["x4", "x1", "m20000", "v512"])
def test_deep_picks_sit_in_the_oracles_cdf_interval(model):
    c = ctx(model)
    rng = np.random.default_rng(13)
    for top_k, top_p in [(20000, 0.9), (c.V, 2.0)]:
        kept, cdf = nucleus_kept(c.probs, top_p, top_k, 1.0)
        pos = {int(t): i for i, t in enumerate(kept)}
        us = [float(u) for u in rng.random(4) * 0.98]
        for u in us[:1]:                                           # the helper above IS nucleus_ref where the margin decides
            want, margin = R.nucleus_ref(c.probs, top_p, top_k, 1.0, u)
            assert margin <= 1e-6 or int(kept[np.searchsorted(cdf, np.float32(u), side="left")]) == want
        for u in us:
            tok, prob = c.one(nucleus(top_k, top_p, 1.0), u)
            assert tok in pos, (model, top_k, top_p, u, tok)
            i = pos[tok]
            lo = float(cdf[i - 1]) if i else 0.0
            print(model, (top_k, top_p), "u", u, "token", tok, "position", i, "of", len(kept), "interval", lo, float(cdf[i]), "prob", prob)
            assert lo - 1e-4 <= u <= float(cdf[i]) + 1e-4, (model, top_k, top_p, u, tok, i, lo, float(cdf[i]))
            assert abs(prob - float(c.probs[tok])) <= 1e-3 * float(c.probs[tok]), (prob, float(c.probs[tok]))


# ---- 3. Mirostat beyond 8192 candidates ---------------------------------------------------------------------------------------------
def mirostat_kept(probs, max_surprise):
    """`mirostat_ref`'s candidates in rank order, their fp32 running sum (the same operations; np.cumsum adds in sequence)"""
    p = probs.astype(np.float32)
    order = np.lexsort((np.arange(p.size), -p))
    with np.errstate(divide="ignore"):
        over = np.nonzero(-np.log2(p[order]) > np.float32(max_surprise))[0]
    order = order[:int(over[0]) + 1] if over.size else order
    return order, np.cumsum(p[order], dtype=np.float32)


@pytest.mark.parametrize("model,max_surprise,flat", [("x4", 16.0, False), ("x4", 17.5, False), ("x1", 16.5, True), ("m20000", 15.0, True)])
def test_mirostat_beyond_8192_candidates(model, max_surprise, flat):
    """The margin rule: id equal when the oracle's margin exceeds 1e-5, surprise within 1e-3 * max(1, |s|), at most a third skipped.
    On M65536 x 4 the draws are uniform over [0, 1) (the oracle alone, on its own logits, keeps 7/8 and 7/8 of these with margin at 16.0
    and 17.5, and 8/8 at 12.5).  The rule needs CDF steps well above the margin: on the FLAT rows (x 1: every step <= 1.2e-4, most
    ~3e-5; M20000 alike) a draw spread over [0, 1) lands within 1e-5 of a boundary more often than the cap allows, whatever the seed.
    There the draws are spread over the HEAD of the row, the tokens of probability >= 5e-5 (a step of five margins): u in [0, mass of
    the head).  `u * sum` and the surprise still go through the sum over ALL candidates, which is what nucleus_kernel's 8192-entry cut
    gets wrong (x 4 at 16: 4 % of the mass).  On every row the interval rule follows, draws over [0, 0.98), nothing skipped: the token
    sits where the oracle's running sum brackets u * sum within the same 1e-5, and its surprise is the oracle's for that token."""
    c = ctx(model)
    rng = np.random.default_rng(17 if flat else 29)
    n = 8
    head = float(c.probs[c.probs >= np.float32(5e-5)].sum(dtype=np.float64)) if flat else 1.0
    order, cum = mirostat_kept(c.probs, max_surprise)
    print(model, max_surprise, "candidates", len(order), "mass", float(cum[-1]), "head", head)
    assert len(order) > 8192
    for ms in (max_surprise, 12.5):                                # 12.5: the same row through the narrow kernel, unchanged
        checked = skipped = 0
        for u in rng.random(n) * head:
            tok, surprise, margin = R.mirostat_ref(c.probs, ms, float(u))
            got = c.one(mirostat(ms), float(u))
            print(model, ms, "u", float(u), "got", got, "want", (tok, surprise), "margin", margin)
            if margin > 1e-5:
                assert got[0] == tok, (model, ms, float(u), got, tok, surprise, margin)
                assert abs(got[1] - surprise) < 1e-3 * max(1.0, abs(surprise)), (got, surprise)
                checked += 1
            else:
                skipped += 1
        assert 3 * skipped <= n, (ms, checked, skipped)
    pos = {int(t): i for i, t in enumerate(order)}
    total = cum[-1]
    for u in rng.random(4) * 0.98:
        tok, s = c.one(mirostat(max_surprise), float(u))
        r = float(np.float32(np.float32(u) * total))
        assert tok in pos, (model, max_surprise, float(u), tok)
        i = pos[tok]
        lo = float(cum[i - 1]) if i else 0.0
        want = float(np.log2(total) - np.log2(c.probs[tok]))
        print(model, max_surprise, "u", float(u), "token", tok, "position", i, "interval", lo, float(cum[i]), "r", r, "surprise", s, want)
        assert lo - 1e-5 <= r <= float(cum[i]) + 1e-5, (model, float(u), tok, i, lo, float(cum[i]), r)
        assert abs(s - want) < 1e-3 * max(1.0, abs(want)), (s, want)


# ---- 4. one call, three launches: every row is written by exactly one kernel ---------------------------------------------------------
def test_narrow_and_wide_rows_in_one_call():
    c = ctx("x4")
    smps = [nucleus(40, 0.9, 1.0), nucleus(5000, 0.95, 0.9), mirostat(16.0), mirostat(6.0)]
    us = [0.31, 0.62, 0.47, 0.83]
    us2 = [0.62, 0.1, 0.47, 0.2]
    greedy = nucleus(1, 0.0, 1.0)                                   # the other rows of an "alone" call: the same step, the same logits bits
    alone = []
    for b in range(B):
        out = c.sample([smps[i] if i == b else greedy for i in range(B)], us)
        assert all(out[i][0] == int(np.argmax(c.row)) for i in range(B) if i != b)
        alone.append(out[b])
    both = c.sample(smps, us)
    print("alone", alone, "together", both)
    for b in range(B):
        assert both[b][0] == alone[b][0] and np.float32(both[b][1]).view(np.uint32) == np.float32(alone[b][1]).view(np.uint32), (b, both[b], alone[b])
    assert alone[1][0] == R.nucleus_ref(c.probs, 0.95, 5000, 0.9, us[1])[0] or R.nucleus_ref(c.probs, 0.95, 5000, 0.9, us[1])[1] <= 1e-4
    # `.take(0)` keeps nothing -> token 0 (nucleus.rs:78-101).  top_k = 0 is never routed wide (wide needs top_k > 256), so this is
    # nucleus_kernel's answer in a call whose other rows are wide; sample_wide_kernel's own `top_k < 1` branch cannot be reached
    # through the engine and is not covered here.
    out = c.sample([nucleus(5000, 0.95, 0.9), nucleus(0, 0.95, 0.9), mirostat(16.0), typical(0, 0.9, 1.0)], us2)
    ref0 = c.sample([nucleus(5000, 0.95, 0.9), greedy, greedy, greedy], us2)[0]
    assert out[1][0] == 0 and out[3][0] == 0 and out[0] == ref0 and out[2] == both[2]
    # top_k above num_vocab is num_vocab
    assert c.one(nucleus(10 ** 9, 0.9, 1.0), 0.4) == c.one(nucleus(c.V, 0.9, 1.0), 0.4)


# ---- 5. resident generation ----------------------------------------------------------------------------------------------------------
def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def build_pair(n_slots):
    st = R.st_serialize(m65536(4))
    mk = lambda: rt.ModelBuilder(st).build(max_batch=n_slots, token_chunk_size=8, precision=rt.Precision.Fp16)
    return mk(), mk()


def prefill(eng, prompts):
    inp = rt.RnnInput([rt.RnnInputBatch(list(p)) for p in prompts])
    first = [None] * len(prompts)
    while inp.num_token() > 0:
        inp, outs = eng.infer(inp)
        for b, o in enumerate(outs):
            if len(o):
                first[b] = int(np.argmax(o[-1]))
    return first


def is_miro(s):
    return getattr(s, "kind", 0) == 2


def test_resident_generation_with_wide_slots_equals_the_per_token_loop():
    """Slot 0: Mirostat with target 4.5 — armed at max_surprise 9, which 4 * target = 18 may exceed, so the slot takes the wide kernel
    in every resident step, while the per-token loop takes the narrow one as long as max_surprise < 13: the bit rule.  Slot 1: Nucleus
    top_k = 4096, armed with wide_top_k.  Slot 2: the default Nucleus sampler (narrow)."""
    A, Bn = build_pair(3)
    V = A.info.num_vocab
    prompts = [[t % V for t in R.synth_prompt(60 + b, 6 + 3 * b)] for b in range(3)]
    first = prefill(A, prompts)
    assert prefill(Bn, prompts) == first
    smp = [H.MirostatSampler(tau=4.5, rate=0.1), H.NucleusSampler(top_p=0.9, top_k=4096, temperature=1.1), H.NucleusSampler()]
    for b in (1, 2):
        smp[b].init(prompts[b])
        smp[b].update(first[b])
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm(1, first[1], 5, H.NucleusSampler(top_k=300))         # without the flag: refused, as before
    assert e.value.code == -3
    n = 12
    for b in range(3):
        A.gen_arm(b, first[b], n, copy.deepcopy(smp[b]), seed=SEED, wide_top_k=(b == 1))
    toks, probs = [], []
    for steps in (1, 11):
        t, p, ne, fin = A.gen_run(steps)
        toks.append(t)
        probs.append(p)
        assert list(ne) == [steps] * 3
    toks, probs = np.concatenate(toks), np.concatenate(probs)
    cur, seen = list(first), []
    want = {b: [] for b in range(3)}
    for d in range(n):                                              # the per-token loop (test_gpu_generate.py `per_token`)
        seen.append(float(smp[0].max_surprise))
        us = [rt.gen_uniform(SEED, b, d) for b in range(3)]
        _, res = Bn.infer_sample(rt.RnnInput([rt.RnnInputBatch([cur[b]]) for b in range(3)]), smp, us)
        for b in range(3):
            tok, prob = res[b]
            smp[b].update(prob if is_miro(smp[b]) else tok)
            want[b].append((tok, prob))
            cur[b] = tok
    print("max_surprise per step", seen)
    assert max(seen) < 13.0, "slot 0 must stay narrow on the per-token side: that is what the bit rule is shown on"
    for b in range(3):
        wt = [t for t, _ in want[b]]
        assert 0 not in wt, "token 0 would stop the resident side: pick another prompt"
        print("slot", b, "want", wt, "got", toks[:, b].tolist())
        np.testing.assert_array_equal(toks[:, b], np.array(wt, np.uint32))
        np.testing.assert_array_equal(bits(probs[:, b]), bits([p for _, p in want[b]]))
    A.close()
    Bn.close()


def test_resident_admission_of_a_prompt_with_a_wide_top_k():
    """rwkv_gen_arm_prompt with wide_top_k: the first draw comes from the prompt's last row in a mixed step, the rest from decode steps"""
    A, Bn = build_pair(2)
    V = A.info.num_vocab
    toks = [t % V for t in R.synth_prompt(31, 13)]                     # two steps of the chunk: 8 + 5
    smp = H.NucleusSampler(top_p=0.9, top_k=4096, temperature=1.1)
    smp.init(toks)
    with pytest.raises(rt.RwkvError) as e:
        A.gen_arm_prompt(0, toks, 5, copy.deepcopy(smp))
    assert e.value.code == -3
    n = 8
    A.gen_arm_prompt(0, toks, n, copy.deepcopy(smp), seed=SEED, wide_top_k=True)
    t, p, ne, fin = A.gen_run(12)
    assert list(ne) == [n, 0] and list(fin) == [rt.GenFinish.Length, 0]
    want = []
    inp = rt.RnnInput([rt.RnnInputBatch(list(toks)), rt.RnnInputBatch()])
    for d in range(n):                                              # test_gpu_gen_prompt.py `reference`
        u, res = rt.gen_uniform(SEED, 0, d), None
        while inp.num_token() > 0:
            inp, r = Bn.infer_sample(inp, [smp, None], [u, 0.0])
            res = r[0] if r[0] is not None else res
        smp.update(res[0])
        want.append(res)
        inp = rt.RnnInput([rt.RnnInputBatch([res[0]]), rt.RnnInputBatch()])
    rows = np.nonzero(t[:, 0] != PAD)[0]
    wt = [x for x, _ in want]
    assert 0 not in wt[:-1]
    print("want", wt, "got", t[rows, 0].tolist())
    np.testing.assert_array_equal(t[rows, 0], np.array(wt, np.uint32))
    np.testing.assert_array_equal(bits(p[rows, 0]), bits([x for _, x in want]))
    A.close()
    Bn.close()

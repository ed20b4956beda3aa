"""The model-dimension sweep shared by tests/test_gpu_dims.py (GPU parity) and tests/test_dims_cpu.py (oracle cross-check, sampler margins,
planner invariants): one table of points of the loader's lattice (rwkv_engine.cpp: C % 64, F % 32, V % 16, head size 64, K % 32 and
rows % 16 per matrix, quantisation C % 256 and F % 256, V6 decay LoRA Dd % 32 and Dd <= 128) that the rest of the suite does not visit,
the step recipes both files run, and the GEMM launches the engine makes of them (what the planner sees).  A plain module, no fixtures.

Two layers everywhere.  `refuse`: the loader must answer RWKV_ERR_UNSUPPORTED (-3) with a message that holds this text; such a row is
never run (the kernels cannot take it: DESIGN.md, "Dimensions the loader accepts")."""
from collections import namedtuple

from oracle import rwkv_ref as R

Row = namedtuple("Row", "ver C F V lora note refuse", defaults=(None,))

TABLE = [
    Row(5, 64, 224, 16, None, "one head, V < 256, TAIL"),
    Row(5, 192, 672, 272, None, "K % 128 = 64, F = 32 x odd"),
    Row(5, 320, 1120, 1008, None, "K % 128 = 64, wider"),
    Row(6, 64, 224, 48, (32, 4), "smallest dims the loader's first contract named", "time_decay LoRA dim"),
    Row(6, 192, 672, 272, (32, 36), "decay dim 36", "time_decay LoRA dim"),
    Row(6, 320, 1120, 1008, (64, 100), "decay dim 100", "time_decay LoRA dim"),
    Row(6, 64, 224, 48, (32, 32), "smallest accepted everything"),
    Row(6, 192, 672, 272, (32, 96), "unfused mix, generic WKV decay dims"),
    Row(6, 320, 1120, 1008, (64, 32), "unfused mix with Dm = 64"),
    Row(6, 512, 1824, 2064, (96, 128), "C % 256 == 0 but Dm unsupported by the fused mix"),
    Row(6, 768, 2816, 4112, (64, 64), "fused mix at 3 x 256; quantisable"),
    Row(7, 64, 256, 16, (32, 32, 32, 32), "smallest V7"),
    Row(7, 192, 768, 272, (32, 64, 96, 160), "mixed small-K lengths"),
    Row(7, 320, 1280, 1008, (96, 96, 64, 352), "Dg > SK_KMAX: small-K must be declined"),
    Row(7, 768, 3072, 4112, (64, 64, 32, 128), "real 0.1B dims; quantisable"),
    Row(7, 2048, 8192, 1024, (96, 96, 64, 256), "real 1.5B dims"),
]
RUN = [i for i, r in enumerate(TABLE) if not r.refuse]
REFUSED = [i for i, r in enumerate(TABLE) if r.refuse]
LAYERS = 2
SK_KMAX = 320                                                   # gemm_plan.h


def row_id(i):
    r = TABLE[i]
    return f"v{r.ver}-C{r.C}-F{r.F}-V{r.V}" + ("" if r.lora is None else "-" + "x".join(str(d) for d in r.lora))


def quantisable(r):
    return r.C % 256 == 0 and r.F % 256 == 0


def tensors(i):
    r = TABLE[i]
    return R.synth_checkpoint(r.ver, LAYERS, r.C, r.F, r.V, seed=9100 + i, lora_dims=r.lora)


# ------------------------------------------------------------------------------------------------
# step recipes: a single step of exactly N rows = slot b feeds the first step_lengths(N)[b] tokens of ITS base sequence, so one lock-step
# run of the reference over the base sequences serves every step size, the Full request and both precisions
# ------------------------------------------------------------------------------------------------
STEP_SIZES = (1, 3, 16, 17, 32, 33, 64, 65, 192, 193, 250)      # both sides of every path boundary of the planner: 16|17, 32|33, 64|65, 192|193
NSLOT = 12
FULL_ROWS = 65                                                  # the RnnOption.Full request: base sequence 0, every row an output row
GREEDY_STEPS = 24


def step_lengths(N):
    """Ragged prompt lengths of a step of exactly N rows: min(N, NSLOT) slots, pairs of slots (base + d, base - d), the remainder on slot 0."""
    B = min(N, NSLOT)
    base = N // B
    lens = [base] * B
    for i in range(B // 2):
        d = min(i + 1, base - 1)
        lens[2 * i] += d
        lens[2 * i + 1] -= d
    lens[0] += N - sum(lens)
    assert sum(lens) == N and min(lens) >= 1
    return lens


def base_len(b):
    """Tokens of base sequence b that any recipe reads."""
    return max([step_lengths(N)[b] for N in STEP_SIZES if b < min(N, NSLOT)] + ([FULL_ROWS] if b == 0 else []))


def base_tokens(i, b):
    V = TABLE[i].V
    return [t % V for t in R.synth_prompt(500 + 20 * i + b, base_len(b))]


def needed_prefixes():
    """{(base sequence, prefix length)}: where a test reads the reference's state."""
    return {(b, n) for N in STEP_SIZES for b, n in enumerate(step_lengths(N))}


# ------------------------------------------------------------------------------------------------
# sampler cases (V = 16 and V = 272): the draws of the on-device sampling test.  The CPU file proves from the oracle's logits that at most
# 1 draw in 16 lies within 1e-4 of a CDF boundary, so the GPU file's cap of 1 in 8 survives device rounding.
# ------------------------------------------------------------------------------------------------
SAMPLER_ROWS = [i for i in RUN if TABLE[i].V in (16, 272)]
SAMPLER_STEPS = 16
SAMPLER_SEED = 4242


SAMPLER_MARGIN = {"nucleus": 1e-4, "typical": 1e-4, "mirostat": 1e-5}   # the rules of tests/test_gpu_parity.py's three sampler tests


def sampler_configs(V):
    """(kind, settings) per slot: nucleus with top_k = 128 (> V at V = 16), top_k = V (the device's cap of 256 at most) and top_k = 1,
    typical, mirostat.  No penalties, no bias: the samplers are under test at a vocabulary, not their state machines."""
    return [("nucleus", dict(top_p=0.9, top_k=128, temperature=1.0)), ("nucleus", dict(top_p=0.7, top_k=min(V, 256), temperature=0.8)),
            ("nucleus", dict(top_p=0.5, top_k=1, temperature=1.0)), ("typical", dict(tau=0.8, top_k=128, temperature=1.0)),
            ("mirostat", dict(tau=3.0, rate=0.1))]


def sampler_tokens(i):
    """[SAMPLER_STEPS][slots] token ids every slot consumes, fixed in advance (the draws are checked, not fed back: the logits the device
    samplers see are then the oracle's up to the engine's rounding, whatever was drawn before)."""
    V = TABLE[i].V
    n = len(sampler_configs(V))
    seqs = [[t % V for t in R.synth_prompt(900 + 10 * i + b, SAMPLER_STEPS)] for b in range(n)]
    return [[seqs[b][s] for b in range(n)] for s in range(SAMPLER_STEPS)]


def sampler_uniforms(i):
    import numpy as np
    return np.random.default_rng(SAMPLER_SEED + i).random((SAMPLER_STEPS, len(sampler_configs(TABLE[i].V)))).astype(np.float32)


def sampler_want(kind, cfg, logits, u, max_surprise):
    """(acceptable ids, margin of the decisive comparison, token surprise or None) of one draw on one logits row."""
    pr = R.softmax_ref(logits[None])[0]
    if kind == "nucleus":
        tok, mg = R.nucleus_ref(pr, cfg["top_p"], cfg["top_k"], cfg["temperature"], u)
        return {tok}, mg, None
    if kind == "typical":                                        # H is a many-term fp32 sum whose last bits depend on the summation order
        alts = [R.typical_ref(pr, cfg["tau"], cfg["top_k"], cfg["temperature"], u, h_shift=d) for d in (0.0, 1e-5, -1e-5, 4e-5, -4e-5)]
        return {a[0] for a in alts}, min(a[1] for a in alts), None
    tok, surprise, mg = R.mirostat_ref(pr, max_surprise, u)
    return {tok}, mg, surprise


def mirostat_update(max_surprise, surprise, cfg):
    """mirostat.rs:85-87 in fp32 (the state machine of harness.MirostatSampler)."""
    import numpy as np
    f = np.float32
    return f(min(f(max_surprise - f(cfg["rate"]) * f(f(surprise) - f(cfg["tau"]))), f(4.0 * cfg["tau"])))


def sampler_walk(i, step, states):
    """The reference side of the sampler test on the logits `step(tokens, states)` returns: yields (kind, margin) per draw."""
    import numpy as np
    cfgs = sampler_configs(TABLE[i].V)
    ms = [np.float32(2.0 * c["tau"]) if k == "mirostat" else None for k, c in cfgs]
    us = sampler_uniforms(i)
    for s, toks in enumerate(sampler_tokens(i)):
        lg = step(toks, states)
        for b, (kind, cfg) in enumerate(cfgs):
            _, margin, surprise = sampler_want(kind, cfg, lg[b], float(us[s, b]), None if ms[b] is None else float(ms[b]))
            if kind == "mirostat":
                ms[b] = mirostat_update(ms[b], surprise, cfg)
            yield kind, margin


# ------------------------------------------------------------------------------------------------
# the GEMM launches of one step as the planner sees them (rwkv_engine.cpp run_layers; gemm_plan.h ProbShape)
# ------------------------------------------------------------------------------------------------
FMT = {0: 0, 1: 1, 2: 2}
CLS_ATT, CLS_LORA2, CLS_WO, CLS_FFN1, CLS_FV, CLS_HEAD, CLS_NONE = 0, 1, 2, 3, 4, 5, 31


def launches(i, quant, fp32, T, n_out):
    """[(name, T, hilo, commit, [(rows, K, fmt, partial, kcopies, smallk), ...])] of a T-row step with n_out output rows, layers 0 and 1.
    `quant`: 0 / 1 (Int8) / 2 (NF4) on both layers; `fp32`: Precision.Fp32 (hi + lo operands everywhere), else Precision.Fp16 (promoted classes)."""
    r = TABLE[i]
    C, F, V, q = r.C, r.F, r.V, quant
    mask = 63 if fp32 else (7 if r.ver == 7 else 1)
    wide = lambda cls: bool(fp32 or (cls < 31 and (mask >> cls) & 1))
    out = []
    for layer in range(LAYERS):
        if r.ver == 5:
            out.append(("att", T, wide(CLS_ATT), 0, [(C, C, q, 0, 1, 1)] * 3 + [(C, C, q, 0, 0, 1)]))
        elif r.ver == 6:
            Dm, Dd = r.lora
            fusable = C % 256 == 0 and Dm in (32, 64)
            if not fusable:
                out.append(("mix1", T, wide(CLS_NONE), 0, [(5 * Dm, C, 0, 0, 0, 0)]))
                out.append(("mix2", T, wide(CLS_NONE), 0, [(C, Dm, 0, 0, 0, 0)] * 5))
            commit = int(fusable and T == 1 and not fp32)
            out.append(("att", T, wide(CLS_ATT), commit, [(C, C, q, 0, 1, 1)] * 3 + [(C, C, q, 0, 0, 1), (Dd, C, 0, 0, 0, 1)]))
        else:
            Dw, Da, Dv, Dg = r.lora
            first = [(C, C, q, 0, 1, 1)] * 3 + [(Dw, C, 0, 0, 0, 0), (Da, C, 0, 0, 0, 0), (Dg, C, 0, 0, 0, 0)]
            second = [(C, Dw, 0, 0, 0, 1), (C, Da, 0, 0, 0, 1), (C, Dg, 0, 0, 1, 1)]
            if layer > 0:
                first.append((Dv, C, 0, 0, 0, 0))
                second.append((C, Dv, 0, 0, 0, 1))
            out.append(("att", T, wide(CLS_ATT), 0, first))
            out.append(("lora2", T, wide(CLS_LORA2), 0, second))
        out.append(("wo", T, wide(CLS_WO), 0, [(C, C, q, 1, 1, 1)]))
        out.append(("ffn1", T, wide(CLS_FFN1), 0, [(F, C, q, 0, 0, 0)] + ([(C, C, q, 0, 0, 1)] if r.ver != 7 else [])))
        out.append(("fv", T, wide(CLS_FV), 0, [(C, F, q, 1, 1, int(r.ver == 7))]))
    if n_out:
        out.append(("head", n_out, wide(CLS_HEAD), 0, [(V, C, 0, 0, 1, 1)]))
    return out


def sweep_launches():
    """Every launch the GPU sweep makes: each run row x precision x quantisation it runs x step size (all slots emit their last row), the Full
    request, and the decode steps of the greedy run."""
    for i in RUN:
        for quant in (0, 1, 2) if quantisable(TABLE[i]) else (0,):
            for fp32 in (False, True):
                steps = [(N, min(N, NSLOT)) for N in STEP_SIZES] + [(FULL_ROWS, FULL_ROWS), (NSLOT, NSLOT)]
                for T, n_out in steps:
                    for name, t, hilo, commit, probs in launches(i, quant, fp32, T, n_out):
                        yield dict(row=i, quant=quant, fp32=fp32, name=name, T=t, hilo=int(hilo), commit=commit, probs=probs)

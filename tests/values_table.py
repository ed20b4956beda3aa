"""The value sweep shared by tests/test_gpu_values.py (GPU parity) and tests/test_values_cpu.py (the checker pinned first): named STRESSORS,
deterministic edits of a benign synthetic checkpoint that put weights where `oracle.rwkv_ref.synth_checkpoint` never does, the recipes both
files run, and a BITE predicate per stressor, evaluated on the oracle's own intermediates over exactly the rows the GPU test runs.
A plain module, no fixtures.

Shapes.  L = 2, F = 512, V = 512, the default LoRA ranks.  Unquantised runs are 128 wide (two heads).  The loader quantises only models whose
width and hidden size are multiples of 256 (rwkv_engine.cpp; tests/test_gpu_dims.py proves the refusal), so the Int8 / NF4 runs are 256 wide
(four heads): the smallest width the quantised kernels take.

Decay ends.  exp(-exp(d)) is exactly 1.0f only for d < -17.3 (exp(d) below half an ulp of 1) and exactly 0 for d > 4.64; V7's
exp(-0.606531 sigmoid(d)) is exactly 1.0f for d < -16.8 and never below exp(-0.606531), which it reaches when the sigmoid is exactly 1.0f
(d > 16.7).  The uniform ranges of `decay_ends` are the stated ones (-12 .. 5, V7 -12 .. 8) with pins at their ends; on top of those a few channels
are pinned at -18 and (V7) -20 / +20, because without them `w == 1.0f` never happens in V5 / V7 and the predicate could not hold."""
import numpy as np

from oracle import rwkv_ref as R

VERSIONS = (5, 6, 7)
STRESSORS = ("decay_ends", "bonus_large", "ln_spread", "emb_outliers", "dead_heads", "ffn_large", "ffn_saturating", "faint_heads")
ALL = "all"                                                     # ALL_PARTS at once
# `ffn_saturating` is the same edit as `ffn_large` at another scale; `faint_heads` (att.value.weight x 0.003: every head's WKV output has a
# variance near or below the GroupNorm's eps 64e-5, so the eps decides the result — an all-zero head is blind to it) would undo `dead_heads`
ALL_PARTS = tuple(s for s in STRESSORS if s not in ("ffn_saturating", "faint_heads"))
FAINT_VARIANCE = 1e-3
QUANT_BLOCKS = "quant_blocks"                                   # Int8 / NF4 runs only
LAYERS, F, V = 2, 512, 512
CONST_ROW, CONST_VALUE = 7, 0.25                                # emb_outliers: this embedding row is constant; slot 0 starts with it
OUTLIER_CHANNELS = (5, 64, 127)
F16_MAX = 65504.0


def width(quant):
    return 256 if quant else 128


def base(ver, quant=0):
    return R.synth_checkpoint(ver, LAYERS, width(quant), F, V, seed=7700 + ver)


# ffn.key.weight x s.  Chosen by running the oracle on the CPU over the rows of the recipes below (tests/test_values_cpu.py holds the predicates):
# `ffn_large` / `all`: the largest relu^2 operand lies in [1e4, 6e4]; `ffn_saturating`: 1-5 % of the operand elements exceed 65504.
FFN_SCALE = {
    (5, "ffn_large"): 72.0, (6, "ffn_large"): 72.0, (7, "ffn_large"): 72.0,
    (5, "ffn_saturating"): 300.0, (6, "ffn_saturating"): 300.0, (7, "ffn_saturating"): 300.0,
    (5, "all"): 22.0, (6, "all"): 28.0, (7, "all"): 28.0,
}


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


# The noise of the planted quantisation blocks is drawn with a salt chosen on the CPU alone, by one criterion: the oracle's own two fp32
# restatements (numpy, C) agree within their 1e-5 / 2e-5 bounds over every row of the decode recipe.  With the planted rows 0..15 the output
# matrices let a few channels dominate the residual stream, and some draws pass an ill-conditioned LayerNorm: over salts 0..9 the
# disagreement reaches 25 x the bound (V5 Int8, blocks alone) and V5 NF4 with everything at once sits at 1.2 .. 2.5 x for all but this
# one (0.77) — there the reference does not resolve the device.  tests/test_values_cpu.py holds the criterion for every quantised case.
QUANT_SALT = 8


def _rng(ver, name, C):
    return np.random.default_rng([ver, C, sum(name.encode()) * 131 + len(name)] + ([QUANT_SALT] if name == QUANT_BLOCKS else []))


def _decay_ends(t, ver, C, rng):
    for l in range(LAYERS):
        a = f"blocks.{l}.att."
        if ver == 7:
            d = rng.uniform(-12, 8, C)
            d[[1, 70]], d[[2, 71]], d[[3, 72]], d[[4, 73]] = -12, 8, -20, 20
            t[a + "w0"] = _f16(d).reshape(1, 1, C)
            continue
        d = rng.uniform(-12, 5, C)
        d[[1, 70]], d[[2, 71]], d[[3, 72]] = -12, 5, -18
        t[a + "time_decay"] = _f16(d).reshape(t[a + "time_decay"].shape)
        if ver == 6:
            for n, sd in (("time_decay_w1", 0.3), ("time_decay_w2", 0.5)):
                t[a + n] = _f16(rng.standard_normal(t[a + n].shape) * sd)


def _bonus_large(t, ver, C, rng):
    for l in range(LAYERS):
        n = f"blocks.{l}.att." + ("r_k" if ver == 7 else "time_first")
        t[n] = _f16(rng.standard_normal(t[n].shape) * 2.0)


def _ln_spread(t, ver, C, rng):
    for l in range(LAYERS):
        for ln in ("ln1", "ln2", "att.ln_x"):
            n = f"blocks.{l}.{ln}."
            t[n + "weight"] = _f16(np.exp(rng.uniform(np.log(0.05), np.log(8.0), C)))
            t[n + "bias"] = _f16(rng.standard_normal(C))


def _emb_outliers(t, ver, C, rng):
    e = t["emb.weight"].copy()
    for c in OUTLIER_CHANNELS:
        e[:, c] = _f16(rng.standard_normal(V) * 150.0)
    e[CONST_ROW, :] = np.float16(CONST_VALUE)
    t["emb.weight"] = e


def _dead_heads(t, ver, C, rng):
    for l in range(LAYERS):
        a = f"blocks.{l}.att."
        w = t[a + "value.weight"].copy()
        w[0:64, :] = 0
        t[a + "value.weight"] = w
        if ver == 7:
            w = t[a + "key.weight"].copy()
            w[64:128, :] = 0
            t[a + "key.weight"] = w


def _faint_heads(t, ver, C, rng):
    for l in range(LAYERS):
        n = f"blocks.{l}.att.value.weight"
        t[n] = _f16(t[n].astype(np.float32) * np.float32(0.003))


def _ffn_scale(t, s):
    for l in range(LAYERS):
        n = f"blocks.{l}.ffn.key.weight"
        t[n] = _f16(t[n].astype(np.float32) * np.float32(s))


def nf4_midpoint_neighbours():
    """For each of the 15 NF4 midpoints: the largest f16 below it and the smallest f16 above it (block absmax 1, so x / absmax = x)."""
    out = []
    for m in R.NF4_MID:
        h = np.float16(m)
        lo = h if np.float32(h) < m else np.nextafter(h, np.float16(-np.inf))
        hi = h if np.float32(h) > m else np.nextafter(h, np.float16(np.inf))
        assert np.float32(lo) < m < np.float32(hi)
        out += [lo, hi]
    return np.array(out, np.float16)


QUANT_KINDS = ("zero", "constant", "noise_one_large", "subnormal_scale", "scale_rounds_to_zero", "f16_max", "nf4_midpoints")
SUBNORMAL = 2.0 ** -24                                          # the f16 subnormal quantum


def quant_block(kind, n, rng):
    """One planted block of n elements (fp16)."""
    if kind == "zero":
        return np.zeros(n, np.float16)
    if kind == "constant":
        return np.full(n, 0.37, np.float16)
    if kind == "noise_one_large":
        b = _f16(rng.standard_normal(n) * 1e-3)
        b[n // 3] = 8.0
        return b
    if kind == "subnormal_scale":                               # Int8: (max - min) / 255 is an f16 subnormal; NF4: absmax is one
        return _f16(rng.uniform(0.0, 0.01, n)) if n == R.INT8_BLOCK else _f16(rng.integers(-80, 81, n) * SUBNORMAL)
    if kind == "scale_rounds_to_zero":                          # not constant, but (max - min) / 255 < 2^-25 rounds to f16 zero
        b = _f16(rng.integers(0, 50, n) * SUBNORMAL)
        b[0], b[1] = 0.0, 49 * SUBNORMAL
        return b
    if kind == "f16_max":                                       # see F16_MAX_IN
        top = F16_MAX if n == R.NF4_BLOCK else 32768.0
        b = _f16(rng.standard_normal(n) * 0.05)
        b[1::8] = top
        b[5::8] = -top
        return b
    nb = nf4_midpoint_neighbours()                              # nf4_midpoints
    b = np.zeros(n, np.float16)
    b[0] = 1.0
    b[1:1 + nb.size] = nb
    return b


# The block at the top of f16's range is planted in one matrix only, and at +-32768 for Int8.  (1) Weights of 65504 in a matrix whose output
# feeds the residual stream unnormalised (output, ffn.value, ffn.key) drive the stream past 1e19, where the variance of a LayerNorm
# overflows fp32 in the oracle itself: no finite reference exists.  The receptance output only meets the head's GroupNorm (V5 / V6) or the
# bonus term (V7, ~1e6), so the model stays finite.  (2) Int8 as the format is defined — a = f16((max - min) / 255) rounds to nearest —
# dequantises the top code of a block whose max is 65504 to a * 255 + b >= 65520 = +inf in f16, in rwkv_ref.dequant_int8 and on the device
# alike ("Value sweep"); 32768 is the largest power of two whose top code stays finite.  (3) V7 has no such matrix: its bonus term
# carries r and k to the residual stream unnormalised, and with the block in place the oracle's two fp32 restatements (numpy, C) disagree
# by 2e-5 x |ref|_inf on the logits (tests/test_values_cpu.py measured 3.7e-5 at |ref| 1.75) — the whole Fp32 bound, so no reference
# resolves the device there.  V7 gets every other kind.
F16_MAX_IN = "att.receptance.weight"


def planted_blocks(name, shape, quant, ver=6):
    """[(row, first column, kind)] of the blocks `quant_blocks` plants in a [rows, K] matrix: rows 0..15, every block of the format."""
    n = R.INT8_BLOCK if quant == R.QUANT_INT8 else R.NF4_BLOCK
    kinds = [k for k in QUANT_KINDS if (k != "f16_max" or (name == F16_MAX_IN and ver != 7)) and (k != "nf4_midpoints" or quant == R.QUANT_NF4)]
    nb = shape[1] // n
    return [(r, j * n, kinds[(r * nb + j) % len(kinds)]) for r in range(16) for j in range(nb)]


def _quant_blocks(t, ver, C, rng, quant):
    n = R.INT8_BLOCK if quant == R.QUANT_INT8 else R.NF4_BLOCK
    for l in range(LAYERS):
        for name in R.quantised_matrix_names(ver):
            k = f"blocks.{l}.{name}"
            w = t[k].copy()
            for r, c0, kind in planted_blocks(name, w.shape, quant, ver):
                w[r, c0:c0 + n] = quant_block(kind, n, rng)
            t[k] = w


_EDIT = {"decay_ends": _decay_ends, "bonus_large": _bonus_large, "ln_spread": _ln_spread, "emb_outliers": _emb_outliers, "dead_heads": _dead_heads,
         "faint_heads": _faint_heads}
_TENSORS = {}


def tensors(ver, stressor, quant=0, ffn_scale=None):
    """The base checkpoint of (ver, width(quant)) with one stressor (or ALL) applied; with `quant`, QUANT_BLOCKS alone or ALL + QUANT_BLOCKS.
    `ffn_scale` overrides FFN_SCALE (the search that filled the table)."""
    key = (ver, stressor, quant, ffn_scale)
    if key in _TENSORS:
        return _TENSORS[key]
    C = width(quant)
    t = dict(base(ver, quant))
    names = ALL_PARTS if stressor == ALL else () if stressor == QUANT_BLOCKS else (stressor,)
    for n in names:
        if n in _EDIT:
            _EDIT[n](t, ver, C, _rng(ver, n, C))
    if stressor in (ALL, "ffn_large", "ffn_saturating"):
        _ffn_scale(t, FFN_SCALE[(ver, stressor)] if ffn_scale is None else ffn_scale)
    if quant:
        assert stressor in (ALL, QUANT_BLOCKS)
        _quant_blocks(t, ver, C, _rng(ver, QUANT_BLOCKS, C), quant)
    _TENSORS[key] = t
    return t


def clipped(stressor, quant=0):
    """Whether the reference of this run is the oracle with `clip_operands` (the engine's saturation contract).  Everywhere else nothing
    saturates and the two are bit-identical (tests/test_values_cpu.py); the planted +-65504 weights of QUANT_BLOCKS do saturate operands."""
    return stressor == "ffn_saturating" or bool(quant)


# ------------------------------------------------------------------------------------------------
# recipes: four base sequences; slot 0's is long.  One lock-step run of the oracle serves every recipe and both precisions.
# ------------------------------------------------------------------------------------------------
NSLOT = 4
PROMPT, DECODE_STEPS = 3, 48                                    # decode: a 3-token prompt, then 48 single-token steps on 4 slots
CHUNK8_ROWS, CHUNK8_CALLS = 8, 6                                # chunk8: 4 slots x 8 rows per call
CHUNK32_ROWS = 70                                               # chunk32: slot 0, one Full call (two chunks of 32 and a ragged tail of 6)
TILE_ROWS = 250                                                 # tile: slot 0, one Last call (>= 193 rows: the tile GEMMs)
LONG_ROWS, LONG_CALL, LONG_GREEDY = 600, 100, 16                # long: slot 0, 600 tokens by 100-row calls, then 16 greedy steps
SHORT = PROMPT + DECODE_STEPS                                   # tokens of base sequences 1..3 (and of slot 0 in the lock-step part)
STATE_AT = {(b, SHORT) for b in range(NSLOT)} | {(b, CHUNK8_ROWS * CHUNK8_CALLS) for b in range(NSLOT)} | \
           {(0, CHUNK32_ROWS), (0, TILE_ROWS), (0, LONG_ROWS)}


def base_tokens(ver, b):
    toks = [x % V for x in R.synth_prompt(700 + 10 * ver + b, LONG_ROWS if b == 0 else SHORT)]
    if b == 0:
        toks[0] = CONST_ROW
    return toks


class Probe:
    """Collects what the bite predicates read from `RwkvRef.probe` over a run."""

    def __init__(self):
        self.w_one = self.w_zero = self.w_floor7 = 0
        self.relu2_max, self.relu2_over, self.relu2_n = 0.0, 0, 0
        self.head0_out_max = 0.0
        self.kappa_ss_min = np.inf
        self.const_row_var = None
        self.t = 0                                              # the token index of the lock-step run (set by Reference)
        self.faint, self.heads_seen = 0, 0                      # slot 0, rows of the chunk32 / tile recipes: (layer, head) outputs of variance <= FAINT_VARIANCE

    def __call__(self, name, layer, a):
        a = np.asarray(a)
        if name == "wdec":
            self.w_one += int((a == np.float32(1.0)).sum())
            self.w_zero += int((a == 0).sum())
            self.w_floor7 += int((a == np.exp(np.float32(-0.606531))).sum())
        elif name == "relu2":
            self.relu2_max = max(self.relu2_max, float(a.max()))
            self.relu2_over += int((a > np.float32(F16_MAX)).sum())
            self.relu2_n += a.size
        elif name == "wkv_out":
            self.head0_out_max = max(self.head0_out_max, float(np.abs(a.reshape(-1, a.shape[-1])[:, :64]).max()))
            if self.t < TILE_ROWS:
                var = a.reshape(-1, a.shape[-1])[0].reshape(-1, 64).astype(np.float32).var(axis=1)
                self.faint += int((var <= FAINT_VARIANCE).sum())
                self.heads_seen += var.size
        elif name == "kappa_ss":
            self.kappa_ss_min = min(self.kappa_ss_min, float(a.min()))
        elif name == "emb_row" and self.const_row_var is None:   # the first token of slot 0: the variance as `_ln` computes it
            x = a.reshape(-1, a.shape[-1])[0].astype(np.float32)
            self.const_row_var = float(((x - x.mean(dtype=np.float32)) ** 2).mean(dtype=np.float32))


class Reference:
    """One lock-step run of RwkvRefBatch over the base sequences: logits[b][t], the state after the prefixes of STATE_AT, the greedy
    continuation of the long recipe (ids, per-step logits) and the probe's counts."""

    def __init__(self, ver, stressor, quant=0, ffn_scale=None, greedy=True):
        self.tens = tensors(ver, stressor, quant, ffn_scale)
        self.rb = rb = R.RwkvRefBatch(self.tens, LAYERS if quant else 0, quant, clip_operands=clipped(stressor, quant))
        self.probe = rb.probe = Probe()
        self.base = [base_tokens(ver, b) for b in range(NSLOT)]
        self.logits = [np.zeros((len(p), V), np.float32) for p in self.base]
        self.state = {}
        states = rb.init_states(NSLOT)
        for t in range(LONG_ROWS):
            self.probe.t = t
            act = [b for b in range(NSLOT) if t < len(self.base[b])]
            sub = np.ascontiguousarray(states[act])
            lg = rb.step([self.base[b][t] for b in act], sub)
            states[act] = sub
            for j, b in enumerate(act):
                self.logits[b][t] = lg[j]
                if (b, t + 1) in STATE_AT:
                    self.state[(b, t + 1)] = sub[j].copy()
        rb.probe = None
        self.greedy_ids, self.greedy_logits = [], []
        if greedy:
            st = self.state[(0, LONG_ROWS)][None].copy()
            cur = int(np.argmax(self.logits[0][-1]))
            self.greedy_first = cur
            for _ in range(LONG_GREEDY):
                lg = rb.step([cur], st)[0]
                cur = int(np.argmax(lg))
                self.greedy_ids.append(cur)
                self.greedy_logits.append(lg)
            self.greedy_state = st[0]


_REF = {}


def reference(ver, stressor, quant=0):
    if (ver, stressor, quant) not in _REF:
        _REF[(ver, stressor, quant)] = Reference(ver, stressor, quant)
    return _REF[(ver, stressor, quant)]


def bites(ver, stressor, p):
    """{predicate: (holds, figure)} of one stressor (or of every component of ALL) on a Probe."""
    names = ALL_PARTS if stressor == ALL else (stressor,)
    out = {}
    if "decay_ends" in names:
        out["w == 1.0f somewhere"] = (p.w_one > 0, p.w_one)
        if ver == 7:
            out["w at V7's floor exp(-0.606531) somewhere"] = (p.w_floor7 > 0, p.w_floor7)
        else:
            out["w == 0 somewhere"] = (p.w_zero > 0, p.w_zero)
    if "dead_heads" in names:
        out["head 0 output exactly 0"] = (p.head0_out_max == 0.0, p.head0_out_max)
        if ver == 7:
            out["a kappa norm of exactly 0 (the floor)"] = (p.kappa_ss_min == 0.0, p.kappa_ss_min)
    if "ffn_saturating" in names:
        share = p.relu2_over / max(1, p.relu2_n)
        out["1-5 % of the relu^2 operand above 65504"] = (0.01 <= share <= 0.05, share)
    if "ffn_large" in names:
        out["relu^2 peak in [1e4, 6e4]"] = (1e4 <= p.relu2_max <= 6e4, p.relu2_max)
    if "faint_heads" in names:
        share = p.faint / max(1, p.heads_seen)
        out[f"most head outputs of the chunk32 / tile rows have variance <= {FAINT_VARIANCE}"] = (share >= 0.5, share)
    if "emb_outliers" in names:
        out["variance of the constant row exactly 0"] = (p.const_row_var == 0.0, p.const_row_var)
    return out


def state_blocks(slab):
    """The pieces a state slab [L, N+2, C] is compared by: the two token-shift rows and every (layer, head) 64 x 64 WKV block, each against
    its own max-abs — one head of V5 reaches 1e3 while its neighbour stays below 1, and a slab-wide bound would let the small one be wrong
    by the large one's tolerance."""
    L, rows, C = slab.shape
    N = rows - 2
    for l in range(L):
        yield (l, "att_shift"), slab[l, 0]
        yield (l, "ffn_shift"), slab[l, N + 1]
        for h in range(C // N):
            yield (l, h), slab[l, 1:1 + N, h * N:(h + 1) * N]


# ------------------------------------------------------------------------------------------------
# Fp16 bounds derived from a simulation ("Value sweep").  Five quantised runs exceed 1e-3 in Precision.Fp16 (Fp32 holds 2e-5
# everywhere).  `simulate_fp16` runs the compiled oracle with the operands of the launch classes that Fp16 leaves in plain f16 rounded on the
# way in against the same oracle unrounded, on the recipe's own rows; the figures are in units of the 1e-3 tolerance (logits per row, state
# per block) and the GPU bound of such a run is 2 x its figure (the near-tie convention).  tests/test_values_cpu.py recomputes every figure.
# ------------------------------------------------------------------------------------------------
FP16_PLAIN_CLASSES = {5: ("wo", "ffn1", "fv", "mix1", "mix2", "decay2", "head"), 6: ("wo", "ffn1", "fv", "mix1", "mix2", "decay2", "head"),
                      7: ("ffn1", "fv", "head")}
FP16_DERIVED = {                                                 # (version, stressor, quantisation) -> {(recipe, "logits" | "state"): simulated}
    (5, QUANT_BLOCKS, 1): {("decode", "logits"): 1.030, ("decode", "state"): 3.262, ("tile", "logits"): 7.247, ("tile", "state"): 7.751},
    (5, ALL, 2): {("decode", "logits"): 2.525},
    (6, QUANT_BLOCKS, 2): {("decode", "logits"): 1.391},
    (6, ALL, 2): {("decode", "logits"): 2.783, ("decode", "state"): 1.683},
    (7, QUANT_BLOCKS, 2): {("decode", "logits"): 1.214},
}


def simulate_fp16(ver, stressor, quant):
    """{(recipe, "logits" | "state"): error / 1e-3 tolerance} of the decode and tile recipes, rounded-operand oracle against the plain one."""
    from oracle.cpu_backend import CpuBackend
    cb = CpuBackend(tensors(ver, stressor, quant), LAYERS if quant else 0, quant)
    mask = sum(1 << CpuBackend.OPERAND_CLASSES.index(n) for n in FP16_PLAIN_CLASSES[ver])

    def run(toks, m):
        cb.set_operand_rounding(m)
        cb.set_operand_clip(True)
        try:
            st = cb.init_states(len(toks))
            return np.stack([cb.step([p[t] for p in toks], st) for t in range(len(toks[0]))]), st
        finally:
            cb.set_operand_rounding(0)
            cb.set_operand_clip(False)

    out = {}
    for name, toks in (("decode", [base_tokens(ver, b)[:SHORT] for b in range(NSLOT)]), ("tile", [base_tokens(ver, 0)[:TILE_ROWS]])):
        (b, sb), (a, sa) = run(toks, 0), run(toks, mask)
        if name == "tile":                                      # a Last request: one row
            a, b = a[-1:], b[-1:]
        out[(name, "logits")] = max(float(np.abs(a[t, i] - b[t, i]).max()) / (1e-3 * max(1.0, float(np.abs(b[t, i]).max())))
                                    for t in range(a.shape[0]) for i in range(a.shape[1]))
        out[(name, "state")] = max(float(np.abs(g - w).max()) / (1e-3 * max(1.0, float(np.abs(w).max())))
                                   for i in range(sa.shape[0]) for (_, g), (_, w) in zip(state_blocks(sa[i]), state_blocks(sb[i])))
    return out

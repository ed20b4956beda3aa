"""The RWKV-4 value sweep shared by tests/test_gpu_v4_values.py (GPU parity) and tests/test_v4_values_cpu.py (the checker pinned first):
named STRESSORS, deterministic edits of a benign synthetic V4 checkpoint, the five recipes of tests/values_table.py (constants imported, not
restated), a BITE predicate per stressor evaluated on V4Ref's probe over exactly the rows the GPU test runs, and the bounds of every run.
A plain module, no fixtures.

Shapes.  L = 2, F = 512, V = 512; 128 wide unquantised, 256 wide for Int8 / NF4 (values_table.width).

Units.  A run is compared unit by unit: per recipe the logits (each row against its own |ref|_inf) and the state per row kind (att shift, aa,
bb, pp, ffn shift; each layer's row against its own |ref|_inf).  A unit's figure is the worst error / tolerance over its rows.

Bounds.  A unit is held to the plain bound (1.0 in units of 2e-5 / 1e-3) unless a table below names it:
  FP32_DERIVED  units where the float32 restatement of the checker itself sits more than 0.5 x the Fp32 bound from the float64 one (fp32
                `exp` at arguments of tens: no device kernel can do better).  The Fp32 GPU bound of such a unit is 2 x that figure.
  FP16_DERIVED  units where the rounded-operand simulation (V4Ref with the operands of the classes Precision.Fp16 leaves in plain f16
                rounded on the way in, against itself unrounded, both clamped) exceeds 1.0.  The Fp16 GPU bound is 2 x that figure.
tests/test_v4_values_cpu.py recomputes every figure and proves that no other unit needs one."""
import numpy as np

from oracle import rwkv_ref as R
from tests import v4_ref
from tests.v4_sweep_table import ROW_KINDS, state_units, unit_ratio
from tests.values_table import (CHUNK8_CALLS, CHUNK8_ROWS, CHUNK32_ROWS, CONST_ROW, CONST_VALUE, DECODE_STEPS, F, F16_MAX, LAYERS, LONG_CALL,  # noqa: F401
                                LONG_GREEDY, LONG_ROWS, NSLOT, OUTLIER_CHANNELS, PROMPT, SHORT, STATE_AT, TILE_ROWS, V, planted_blocks, quant_block, width)

STRESSORS = ("decay_ends", "keys_large", "bonus_large", "ln_spread", "emb_outliers", "dead_channels", "ffn_large", "ffn_saturating")
ALL = "all"
ALL_PARTS = tuple(s for s in STRESSORS if s != "ffn_saturating")
QUANT_BLOCKS = "quant_blocks"                                   # Int8 / NF4 runs only, alone and with ALL
RECIPES = ("decode", "chunk8", "chunk32", "tile", "long")
QUANT_RECIPES = ("decode", "tile")                              # what the quantised runs go through (as tests/test_gpu_values.py)
UNITS = ("logits",) + ROW_KINDS
FP16_TOL, FP32_TOL = 1e-3, 2e-5
KEY_SCALE = 36.0                                                # keys_large: the edit of tests/test_gpu_v4.py's range test
# ALL has a key scale of its own, like its ffn scale: with `ln_spread` in place (LayerNorm weights up to 8) x 36 puts max |k| at 200, outside
# the 50 .. 88 the predicate of `keys_large` asks of every run it is part of (and where fp32 exp still resolves the 2e-5 bound).
KEY_SCALE_ALL = 12.0

# ffn.key.weight x s, found on the CPU by the search that filled values_table.FFN_SCALE (doubling, then bisection on the predicate over the
# rows of the recipes); tests/test_v4_values_cpu.py holds the predicates, so a wrong scale fails there.
FFN_SCALE = {"ffn_large": 72.0, "ffn_saturating": 300.0, "all": 12.0}

# The salt of the planted blocks' noise, chosen on the CPU alone by the criterion of values_table.QUANT_SALT: V4Ref(float32) and V4Ref(float64)
# agree within the Fp32 bound on every unit of the decode recipe, for all four quantised cases.  Salts tried: see tests/test_v4_values_cpu.py.
QUANT_SALT = 0


def base(quant=0):
    return v4_ref.synth_checkpoint_v4(LAYERS, width(quant), F, V, seed=7704)


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def _rng(name, C, salt=None):
    return np.random.default_rng([4, C, sum(name.encode()) * 131 + len(name)] + ([QUANT_SALT if salt is None else salt] if name == QUANT_BLOCKS else []))


def _decay_ends(t, C, rng):
    for l in range(LAYERS):
        d = rng.uniform(-12, 5, C)
        d[[1, 70]], d[[2, 71]], d[[3, 72]] = -12, 5, -18
        t[f"blocks.{l}.att.time_decay"] = _f16(d)


def _keys_large(t, C, rng, scale=KEY_SCALE):
    for l in range(LAYERS):
        n = f"blocks.{l}.att.key.weight"
        t[n] = _f16(t[n].astype(np.float32) * np.float32(scale))


def _bonus_large(t, C, rng):
    for l in range(LAYERS):
        t[f"blocks.{l}.att.time_first"] = _f16(rng.standard_normal(C) * 2.0)


def _ln_spread(t, C, rng):
    for l in range(LAYERS):
        for ln in ("ln1", "ln2"):
            t[f"blocks.{l}.{ln}.weight"] = _f16(np.exp(rng.uniform(np.log(0.05), np.log(8.0), C)))
            t[f"blocks.{l}.{ln}.bias"] = _f16(rng.standard_normal(C))


def _emb_outliers(t, C, rng):
    e = t["emb.weight"].copy()
    for c in OUTLIER_CHANNELS:
        e[:, c] = _f16(rng.standard_normal(V) * 150.0)
    e[CONST_ROW, :] = np.float16(CONST_VALUE)
    t["emb.weight"] = e


def _dead_channels(t, C, rng):
    for l in range(LAYERS):
        for n, rows in (("value", slice(0, 64)), ("key", slice(64, 128))):
            w = t[f"blocks.{l}.att.{n}.weight"].copy()
            w[rows, :] = 0
            t[f"blocks.{l}.att.{n}.weight"] = w


def _ffn_scale(t, s):
    for l in range(LAYERS):
        n = f"blocks.{l}.ffn.key.weight"
        t[n] = _f16(t[n].astype(np.float32) * np.float32(s))


def _quant_blocks(t, C, rng, quant):
    n = R.INT8_BLOCK if quant == R.QUANT_INT8 else R.NF4_BLOCK
    for l in range(LAYERS):
        for name in v4_ref.QUANT_NAMES:
            k = f"blocks.{l}.{name}"
            w = t[k].copy()
            for r, c0, kind in planted_blocks(name, w.shape, quant):   # the top-of-range block in att.receptance.weight only (values_table.F16_MAX_IN)
                w[r, c0:c0 + n] = quant_block(kind, n, rng)
            t[k] = w


_EDIT = {"decay_ends": _decay_ends, "keys_large": _keys_large, "bonus_large": _bonus_large, "ln_spread": _ln_spread,
         "emb_outliers": _emb_outliers, "dead_channels": _dead_channels}
_TENSORS = {}


def tensors(stressor, quant=0, ffn_scale=None, salt=None, key_scale=None):
    """The base checkpoint of width(quant) with one stressor (or ALL) applied; with `quant`, QUANT_BLOCKS alone or ALL + QUANT_BLOCKS.
    `ffn_scale` / `salt` / `key_scale` override FFN_SCALE / QUANT_SALT / KEY_SCALE_ALL (the searches that filled them)."""
    key = (stressor, quant, ffn_scale, salt, key_scale)
    if key in _TENSORS:
        return _TENSORS[key]
    C = width(quant)
    t = dict(base(quant))
    names = ALL_PARTS if stressor == ALL else () if stressor == QUANT_BLOCKS else (stressor,)
    for n in names:
        if n == "keys_large" and stressor == ALL:
            _keys_large(t, C, None, KEY_SCALE_ALL if key_scale is None else key_scale)
        elif n in _EDIT:
            _EDIT[n](t, C, _rng(n, C))
    if stressor in FFN_SCALE:
        _ffn_scale(t, FFN_SCALE[stressor] if ffn_scale is None else ffn_scale)
    if quant:
        assert stressor in (ALL, QUANT_BLOCKS)
        _quant_blocks(t, C, _rng(QUANT_BLOCKS, C, salt), quant)
    _TENSORS[key] = t
    return t


def clipped(stressor, quant=0):
    """Whether the reference of this run is the checker with `clip_operands` (the engine's saturation contract): where operands saturate."""
    return stressor == "ffn_saturating" or bool(quant)


CASES = [(s, 0) for s in STRESSORS + (ALL,)] + [(s, q) for s in (QUANT_BLOCKS, ALL) for q in (R.QUANT_INT8, R.QUANT_NF4)]


def case_id(stressor, quant):
    return f"{stressor}-{('f16', 'int8', 'nf4')[quant]}"


def recipes_of(quant):
    return QUANT_RECIPES if quant else RECIPES


def base_tokens(b):
    toks = v4_ref.prompt(V, 740 + b, LONG_ROWS if b == 0 else SHORT)
    if b == 0:
        toks[0] = CONST_ROW                                       # slot 0 starts with the constant embedding row
    return toks


class Probe:
    """Collects what the bite predicates read from `V4Ref.probe` over a run (fp32 questions are asked of the values cast to fp32)."""

    def __init__(self):
        self.decay_noop = self.state_forgotten = 0
        self.k_max = 0.0
        self.relu2_max, self.relu2_over, self.relu2_n = 0.0, 0, 0
        self.dead_out_max = self.dead_k_max = 0.0
        self.const_row_var = None

    def __call__(self, name, layer, a):
        a = np.asarray(a)
        if name == "pp_step":                                   # a live pp (not the initial -1e30) that the decay leaves where it was, in fp32
            pp, ww = a[0].astype(np.float32), a[1].astype(np.float32)
            self.live = pp > np.float32(-1e29)
            self.decay_noop += int(((ww == pp) & self.live).sum())
        elif name == "e_state":                                  # a live state whose share e1 of the update is exactly 0 in fp32 (follows pp_step)
            self.state_forgotten += int(((a[1].astype(np.float32) == 0) & self.live).sum())
        elif name == "k":
            self.k_max = max(self.k_max, float(np.abs(a).max()))
            self.dead_k_max = max(self.dead_k_max, float(np.abs(a[64:128]).max()))
        elif name == "wkv_out":
            self.dead_out_max = max(self.dead_out_max, float(np.abs(a[:64]).max()))
        elif name == "relu2":
            self.relu2_max = max(self.relu2_max, float(a.max()))
            self.relu2_over += int((a > F16_MAX).sum())
            self.relu2_n += a.size
        elif name == "emb_row" and self.const_row_var is None:   # the first token of slot 0: the variance as an fp32 LayerNorm computes it
            x = a.astype(np.float32)
            self.const_row_var = float(((x - x.mean(dtype=np.float32)) ** 2).mean(dtype=np.float32))


class Reference:
    """One run of `model` per base sequence: logits[b][t], the state after the prefixes of values_table.STATE_AT, the greedy continuation of
    the long recipe (ids, per-step logits, final state; `follow` replays given ids instead of the model's own arg-max) and the probe's counts."""

    def __init__(self, model, greedy=True, follow=None, probe=True):
        self.model = model
        self.probe = model.probe = Probe() if probe else None
        self.base = [base_tokens(b) for b in range(NSLOT)]
        self.logits, self.state = [], {}
        for b in (0, 1, 2, 3):                                    # slot 0 first: the probe's emb_row is its first token
            s = model.init_state()
            rows = []
            for t, tok in enumerate(self.base[b]):
                rows.append(model.forward([tok], s)[-1])
                if (b, t + 1) in STATE_AT:
                    self.state[(b, t + 1)] = s.copy()
            self.logits.append(np.stack(rows))
        model.probe = None
        self.greedy_ids, self.greedy_logits = [], []
        if greedy:
            s = self.state[(0, LONG_ROWS)].copy()
            self.greedy_first = cur = int(np.argmax(self.logits[0][-1])) if follow is None else follow[0]
            for i in range(LONG_GREEDY):
                lg = model.forward([cur], s)[-1]
                cur = int(np.argmax(lg)) if follow is None else follow[1][i]
                self.greedy_ids.append(cur)
                self.greedy_logits.append(lg)
            self.greedy_state = s


def make_model(stressor, quant=0, dtype=np.float64, clip=None, round_operands=(), pairwise_sums=False, **kw):
    return v4_ref.V4Ref(tensors(stressor, quant, **kw), LAYERS if quant else 0, quant, dtype=dtype,
                        clip_operands=clipped(stressor, quant) if clip is None else clip, round_operands=round_operands, pairwise_sums=pairwise_sums)


_REF = {}


def reference(stressor, quant=0):
    if (stressor, quant) not in _REF:
        _REF[(stressor, quant)] = Reference(make_model(stressor, quant))
    return _REF[(stressor, quant)]


def bites(stressor, p, tens):
    """{predicate: (holds, figure)} of one stressor (or of every component of ALL) on a Probe and the tensors it ran on."""
    names = ALL_PARTS if stressor == ALL else (stressor,)
    out = {}
    if "decay_ends" in names:
        out["pp + w == pp in fp32 somewhere (a decay that does nothing)"] = (p.decay_noop > 0, p.decay_noop)
        out["state-side e1 exactly 0 in fp32 somewhere (the state forgotten in one token)"] = (p.state_forgotten > 0, p.state_forgotten)
    if "keys_large" in names:
        out["50 <= max |k| <= 88"] = (50.0 <= p.k_max <= 88.0, p.k_max)
    if "bonus_large" in names:
        u = max(float(np.abs(tens[f"blocks.{l}.att.time_first"].astype(np.float32)).max()) for l in range(LAYERS))
        out["max |u| >= 4"] = (u >= 4.0, u)
    if "dead_channels" in names:
        out["wkv_out of channels 0..63 exactly 0"] = (p.dead_out_max == 0.0, p.dead_out_max)
        out["k of channels 64..127 exactly 0"] = (p.dead_k_max == 0.0, p.dead_k_max)
    if "ffn_saturating" in names:
        share = p.relu2_over / max(1, p.relu2_n)
        out["1-5 % of the relu^2 operand above 65504"] = (0.01 <= share <= 0.05, share)
    if "ffn_large" in names:
        out["relu^2 peak in [1e4, 6e4]"] = (1e4 <= p.relu2_max <= 6e4, p.relu2_max)
    if "emb_outliers" in names:
        out["variance of the constant row exactly 0"] = (p.const_row_var == 0.0, p.const_row_var)
    return out


class Tally:
    """Worst error / tolerance of one recipe per unit, and whether anything was not finite."""

    def __init__(self, factor):
        self.f, self.worst, self.finite, self.near_tie = factor, dict.fromkeys(UNITS, 0.0), True, 0

    def row(self, got, want):
        self.finite &= bool(np.isfinite(got).all())
        self.worst["logits"] = max(self.worst["logits"], unit_ratio(got, want, self.f))

    def slab(self, got, want):
        self.finite &= bool(np.isfinite(got).all())
        for ((_, kind), g), (_, w) in zip(state_units(got), state_units(want)):
            self.worst[kind] = max(self.worst[kind], unit_ratio(g, w, self.f))


def recipe_units(ref, other, factor, recipes=RECIPES):
    """{(recipe, unit): error / tolerance} of `other` against `ref` (two References over the same tokens) on the rows each recipe compares on
    the GPU (tests/test_gpu_v4_values.py run_recipe): what the conditioning figures and the Fp16 simulation are measured on."""
    out = {}
    for name in recipes:
        t = Tally(factor)
        if name == "decode":
            for b in range(NSLOT):
                for s in range(PROMPT - 1, SHORT):
                    t.row(other.logits[b][s], ref.logits[b][s])
                t.slab(other.state[(b, SHORT)], ref.state[(b, SHORT)])
        elif name == "chunk8":
            n = CHUNK8_ROWS * CHUNK8_CALLS
            for b in range(NSLOT):
                for hi in range(CHUNK8_ROWS, n + 1, CHUNK8_ROWS):
                    t.row(other.logits[b][hi - 1], ref.logits[b][hi - 1])
                t.slab(other.state[(b, n)], ref.state[(b, n)])
        elif name == "chunk32":
            for r in range(CHUNK32_ROWS):
                t.row(other.logits[0][r], ref.logits[0][r])
            t.slab(other.state[(0, CHUNK32_ROWS)], ref.state[(0, CHUNK32_ROWS)])
        elif name == "tile":
            t.row(other.logits[0][TILE_ROWS - 1], ref.logits[0][TILE_ROWS - 1])
            t.slab(other.state[(0, TILE_ROWS)], ref.state[(0, TILE_ROWS)])
        else:
            for hi in range(LONG_CALL, LONG_ROWS + 1, LONG_CALL):
                t.row(other.logits[0][hi - 1], ref.logits[0][hi - 1])
            t.slab(other.state[(0, LONG_ROWS)], ref.state[(0, LONG_ROWS)])
            for g, w in zip(other.greedy_logits, ref.greedy_logits):
                t.row(g, w)
            t.slab(other.greedy_state, ref.greedy_state)
        for u in UNITS:
            out[(name, u)] = t.worst[u]
    return out


def conditioning(stressor, quant, **kw):
    """{(recipe, unit): distance of the float32 checker from the float64 one / Fp32 bound} on the recipes' own rows (the float32 run replays the
    float64 run's greedy ids: the question is the arithmetic's, not the arg-max's; it sums rows pairwise, V4Ref's `pairwise_sums`, so that the
    figures do not depend on the BLAS kernel of the CPU at hand)."""
    ref = Reference(make_model(stressor, quant, **kw), probe=False) if kw else reference(stressor, quant)
    f32 = Reference(make_model(stressor, quant, np.float32, pairwise_sums=True, **kw), follow=(ref.greedy_first, ref.greedy_ids), probe=False)
    return recipe_units(ref, f32, FP32_TOL, recipes_of(quant))


def simulate_fp16(stressor, quant):
    """{(recipe, unit): error / 1e-3 tolerance}: V4Ref(round_operands=FP16_PLAIN, clip_operands=True) against the same checker unrounded."""
    plain = Reference(make_model(stressor, quant, clip=True), probe=False)
    rounded = Reference(make_model(stressor, quant, clip=True, round_operands=v4_ref.V4Ref.FP16_PLAIN),
                        follow=(plain.greedy_first, plain.greedy_ids), probe=False)
    return recipe_units(plain, rounded, FP16_TOL, recipes_of(quant))


# (stressor, quantisation) -> {(recipe, unit): figure}; see the module docstring.  Filled from the CPU file's own printout.  FP32_DERIVED lists
# every unit whose figure exceeds 0.45 (a unit below 0.5 keeps the plain bound: cap() is max(1, 2 x figure)); the large ones are `keys_large`'s
# aa / bb rows, fp32 `exp` at |k| of 50 .. 66 summed over hundreds of tokens, which is why the slab-wide bound of tests/test_gpu_v4.py passes.
FP32_DERIVED = {
    ("decay_ends", 0): {("tile", "pp"): 0.454, ("long", "aa"): 0.544, ("long", "bb"): 0.695, ("long", "pp"): 1.107},
    ("keys_large", 0): {("decode", "aa"): 1.031, ("decode", "bb"): 0.521, ("chunk8", "aa"): 1.031, ("chunk8", "bb"): 0.458, ("chunk32", "aa"): 0.675,
                        ("chunk32", "bb"): 0.551, ("tile", "aa"): 3.136, ("tile", "bb"): 3.373, ("long", "aa"): 6.368, ("long", "bb"): 13.895,
                        ("long", "pp"): 1.013},
    ("ln_spread", 0): {("long", "bb"): 0.501},
    ("dead_channels", 0): {("tile", "bb"): 0.516, ("long", "aa"): 0.480, ("long", "bb"): 0.984},
    (ALL, 0): {("tile", "bb"): 0.514, ("long", "aa"): 0.702, ("long", "bb"): 1.178, ("long", "pp"): 1.361},
    (QUANT_BLOCKS, 1): {("tile", "aa"): 0.666},
    (ALL, 1): {("decode", "aa"): 0.662, ("tile", "aa"): 1.678, ("tile", "bb"): 0.475, ("tile", "pp"): 0.455},
    (ALL, 2): {("tile", "aa"): 0.629, ("tile", "bb"): 0.475},
}
FP16_DERIVED = {
    (ALL, 2): {("decode", "logits"): 1.636},
}


def cap(stressor, quant, fp32, recipe, unit):
    """The GPU bound of one unit of one run in units of its tolerance."""
    table = FP32_DERIVED if fp32 else FP16_DERIVED
    return max(1.0, 2.0 * table.get((stressor, quant), {}).get((recipe, unit), 0.0))

"""The RWKV-4 rows of the dimension sweep, shared by tests/test_gpu_v4_dims.py (GPU parity) and tests/test_v4_sweep_cpu.py (the checker
pinned first).  The step recipes are those of tests/dims_table.py, imported, not restated; the reference is tests/v4_ref.py's V4Ref in
float64, one run per (row, quantisation) over the twelve base sequences.  A plain module, no fixtures.

State rule.  The V4 slab [5L][C] is compared per layer and per row kind (att shift, aa, bb, pp, ffn shift), each against its own
|ref|_inf: the pp rows reach tens while the shift rows stay O(1), and a slab-wide bound would let a shift row be wrong by the pp rows'
tolerance."""
from collections import namedtuple

import numpy as np

from tests import v4_ref
from tests.dims_table import FULL_ROWS, GREEDY_STEPS, NSLOT, STEP_SIZES, needed_prefixes, step_lengths  # noqa: F401  (the recipes)

Row = namedtuple("Row", "C F V note")
TABLE = [
    Row(64, 224, 16, "one wave per row in wkv4_kernel, V < 256, TAIL"),
    Row(192, 672, 272, "K % 128 = 64, F = 32 x odd"),
    Row(320, 1120, 1008, "the same, wider; two wkv4_kernel blocks, the second a quarter full"),
    Row(768, 3072, 4112, "real 169M dims; quantisable"),
]
LAYERS = 2
RUN = list(range(len(TABLE)))
# shapes the loader must refuse (rwkv_engine.cpp: C % 64, F % 32, V % 16): (C, F, V, layers)
REFUSED = [(96, 384, 16, 2), (64, 224, 50277, 1)]
REFUSAL = "C%64==0, F%32==0, V%16==0"
ROW_KINDS = ("att_shift", "aa", "bb", "pp", "ffn_shift")
FP16_TOL, FP32_TOL = 1e-3, 2e-5


def row_id(i):
    r = TABLE[i]
    return f"v4-C{r.C}-F{r.F}-V{r.V}"


def quantisable(r):
    return r.C % 256 == 0 and r.F % 256 == 0


def tensors(i):
    r = TABLE[i]
    return v4_ref.synth_checkpoint_v4(LAYERS, r.C, r.F, r.V, seed=9200 + i)


def refused_tensors(j):
    C, F, V, L = REFUSED[j]
    return v4_ref.synth_checkpoint_v4(L, C, F, V, seed=9300 + j)


def base_len(b):
    """Tokens of base sequence b that any recipe reads."""
    return max([step_lengths(N)[b] for N in STEP_SIZES if b < min(N, NSLOT)] + ([FULL_ROWS] if b == 0 else []))


def base_tokens(i, b):
    return v4_ref.prompt(TABLE[i].V, 500 + 20 * i + b, base_len(b))


def state_units(slab):
    """((layer, row kind), row [C]) of a slab [5L][C] (or [1][5L][C]): the pieces a V4 state is compared by."""
    s = np.asarray(slab)
    s = s.reshape(-1, s.shape[-1])
    for l in range(s.shape[0] // 5):
        for j, kind in enumerate(ROW_KINDS):
            yield (l, kind), s[5 * l + j]


def unit_ratio(got, want, factor):
    """|got - want|_inf / (factor * max(1, |want|_inf)) of one compared unit (a logits row, a state row)."""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / (factor * max(1.0, float(np.abs(want).max())))


def state_ratio(got, want, factor):
    return max(unit_ratio(g, w, factor) for (_, g), (_, w) in zip(state_units(got), state_units(want)))


class Reference:
    """logits[b][t] and the state after n tokens of base sequence b at the prefixes the recipes read (dims_table.needed_prefixes), from one
    run of `model` (a V4Ref, or anything with its `init_state` / `forward`) per base sequence."""

    def __init__(self, i, model):
        self.model = model
        self.base = [base_tokens(i, b) for b in range(NSLOT)]
        need = needed_prefixes()
        self.logits, self.state = [], {}
        for b, toks in enumerate(self.base):
            s = model.init_state()
            rows = []
            for t, tok in enumerate(toks):
                rows.append(model.forward([tok], s)[-1])
                if (b, t + 1) in need:
                    self.state[(b, t + 1)] = s.copy()
            self.logits.append(np.stack(rows))

    def greedy(self, n=GREEDY_STEPS):
        """The greedy run that goes on from the 3-row step: per slot (first id, [n] ids, [n] logits rows, final state)."""
        out = []
        for b, ln in enumerate(step_lengths(3)):
            s = self.state[(b, ln)].copy()
            first = cur = int(np.argmax(self.logits[b][ln - 1]))
            ids, lgs = [], []
            for _ in range(n):
                lg = self.model.forward([cur], s)[-1]
                cur = int(np.argmax(lg))
                ids.append(cur)
                lgs.append(lg)
            out.append((first, ids, np.stack(lgs), s))
        return out


_REF = {}


def reference(i, quant=0, dtype=np.float64):
    key = (i, quant, np.dtype(dtype).name)
    if key not in _REF:
        _REF[key] = Reference(i, v4_ref.V4Ref(tensors(i), LAYERS if quant else 0, quant, dtype=dtype))
    return _REF[key]


def compared_units(ref, other, factor):
    """{unit name: error / tolerance} of `other` against `ref` (two References of one row) over everything the GPU file compares: the last
    row of every slot of every step size, the state per (layer, row kind) there, and every row of the Full request."""
    out = {}
    for N in STEP_SIZES:
        for b, ln in enumerate(step_lengths(N)):
            out[f"step{N}.slot{b}.logits"] = unit_ratio(other.logits[b][ln - 1], ref.logits[b][ln - 1], factor)
            for ((l, kind), g), (_, w) in zip(state_units(other.state[(b, ln)]), state_units(ref.state[(b, ln)])):
                out[f"step{N}.slot{b}.state.{l}.{kind}"] = unit_ratio(g, w, factor)
    for t in range(FULL_ROWS):
        out[f"full.row{t}"] = unit_ratio(other.logits[0][t], ref.logits[0][t], factor)
    return out

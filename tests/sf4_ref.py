"""The checker of Quant::SF4: the code book, its derivation, and the quantiser arithmetic, written as oracle/rwkv_ref.py writes NF4's.

SF4 is the "Student Float" of Dotzel et al. 2024 ("Learning from Students: Applying t-Distributions to Explore Accurate and Efficient
Formats for LLMs"): the NF4 construction of QLoRA (Dettmers et al. 2023, Appendix E) with the standard normal replaced by Student's t with
5 degrees of freedom:

    eight positive points  ppf(linspace(delta, 0.5, 9)[:-1]),  zero,  seven negative points  -ppf(linspace(delta, 0.5, 8)[:-1]),
    delta = 0.9677083, sorted, divided by the largest magnitude.

With the normal ppf this reproduces oracle.rwkv_ref.NF4_TABLE to float32 (tests/test_sf4_cpu.py).  The t5 quantile is taken from the closed
form of its CDF,  F(x) = 1/2 + (th + sin th cos th (1 + (2/3) cos^2 th)) / pi,  th = atan(x / sqrt 5),  inverted by bisection in float64;
scipy.stats.t.ppf agrees to 1e-9 where scipy is installed.  The float32 table and its fp16 rounding are pinned in
tests/golden/sf4_table.json.  [EXT] Whether web-rwkv's SF4 table has these digits cannot be checked offline: the format is build-defined, as
Int8 and NF4 are.

Everything else is NF4's, expression for expression: 64-element blocks, absmax stored as fp16, idx = #(x / absmax > mid_i) with the fp32
midpoints (Q[i+1] + Q[i]) * 0.5f of the float32 table, dequantisation fp16(absmax * fp16(Q[idx])) rounded once.  A plain module, no fixtures;
no file of oracle/ knows SF4: the oracle evaluates an SF4 model as an unquantised model on `prequantise`d weights, which are fp16 values."""
import json
import math
import os

import numpy as np

from oracle import rwkv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sf4_table.json")
QUANT_SF4 = 3
SF4_BLOCK = R.NF4_BLOCK
DELTA = 0.9677083
T_DOF = 5


def t5_cdf(x):
    th = math.atan(x / math.sqrt(5.0))
    c = math.cos(th)
    return 0.5 + (th + math.sin(th) * c * (1.0 + (2.0 / 3.0) * c * c)) / math.pi


def normal_cdf(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def ppf_by_bisection(cdf):
    """The quantile function of a continuous, strictly increasing `cdf`, for p in [0.5, 1): float64 bisection to the last bit."""
    def ppf(p):
        assert 0.5 <= p < 1.0
        lo, hi = 0.0, 1.0
        while cdf(hi) < p:
            hi *= 2.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if cdf(mid) < p:
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)
    return ppf


def construct(ppf, delta=DELTA):
    """The 16 code points of the NF4 construction over the distribution whose quantile function is `ppf`, float64."""
    pos = [ppf(float(p)) for p in np.linspace(delta, 0.5, 9)[:-1]]
    neg = [-ppf(float(p)) for p in np.linspace(delta, 0.5, 8)[:-1]]
    v = np.sort(np.array(pos + [0.0] + neg, np.float64))
    return v / np.abs(v).max()


SF4_TABLE_F64 = construct(ppf_by_bisection(t5_cdf))
SF4_TABLE = SF4_TABLE_F64.astype(np.float32)
SF4_MID = ((SF4_TABLE[1:] + SF4_TABLE[:-1]) * np.float32(0.5)).astype(np.float32)
SF4_TABLE_F16 = SF4_TABLE.astype(np.float16)


def golden():
    """(float32 table, fp16 bit patterns) as tests/golden/sf4_table.json pins them."""
    with open(GOLDEN) as f:
        g = json.load(f)
    return np.array(g["table_f32"], np.float64).astype(np.float32), np.array([int(h, 16) for h in g["table_f16_bits"]], np.uint16)


def quant_sf4(w16):
    """Per 64-element block: absmax fp16, idx = #(x/absmax > mid_i). Returns (idx u8, absmax f16)."""
    out_dim, in_dim = w16.shape
    assert in_dim % SF4_BLOCK == 0
    x = w16.astype(np.float32).reshape(out_dim, in_dim // SF4_BLOCK, SF4_BLOCK)
    am = np.abs(x).max(axis=2).astype(np.float16)
    am32 = am.astype(np.float32)
    safe = np.where(am32 > 0, am32, np.float32(1.0))
    xn = x / safe[..., None]
    idx = (xn[..., None] > SF4_MID).sum(axis=-1).astype(np.uint8)
    return idx.reshape(out_dim, in_dim), am


def dequant_sf4(idx, am):
    """x^ = fp16(absmax * fp16(Q[idx])) with one rounding (v_pk_mul_f16)."""
    out_dim, in_dim = idx.shape
    t = SF4_TABLE_F16.astype(np.float64)[idx.reshape(out_dim, in_dim // SF4_BLOCK, SF4_BLOCK)]
    v = am.astype(np.float64)[..., None] * t
    return v.astype(np.float16).reshape(out_dim, in_dim)


def fake_quant_sf4(w16):
    return dequant_sf4(*quant_sf4(np.asarray(w16, np.float16)))


def prequantise(tensors, quant_layers, names=None):
    """The checkpoint with every matrix the loader quantises in layers 0 .. quant_layers - 1 replaced by its SF4 fake-quantisation.  Those
    values are fp16, so an unquantised evaluation of the result evaluates exactly the SF4 model.  `names`: the per-layer matrix names
    (default: oracle.rwkv_ref.quantised_matrix_names of the checkpoint's version; tests/v4_ref.py QUANT_NAMES for a V4 checkpoint)."""
    if names is None:
        names = R.quantised_matrix_names(int(R.model_info(tensors).version))
    L = sum(1 for k in tensors if k.endswith(".ln1.weight"))
    out = dict(tensors)
    for l in range(min(quant_layers, L)):
        for n in names:
            k = f"blocks.{l}.{n}"
            out[k] = fake_quant_sf4(tensors[k])
    return out

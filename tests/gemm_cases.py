"""The GEMM probe's case table, shared by tests/test_gpu_gemm_exact.py (runs tests/cpp/gemm_probe.hip on the GPU) and
tests/test_gemm_cases_cpu.py (proves the table without one): one launch per case, inputs from grids on which every product and every partial
sum is exactly representable, so the fp64 reference must be met in every bit whatever the order of summation (DESIGN.md "GEMM probe").

  lattice   weights on which quantise -> dequantise is the identity (fp16: small integers; Int8: b + q/16 with q = 0 and q = 255 in every
            128-block, so a = 1/16; NF4: {-am, 0, +am}, am a power of two per 64-block), integer X hi, X lo in quarters, integer bias / m0 / m1
  onehot    ARBITRARY fp16 weights; token t is one power of two at column perm[t]: the output row is fake_quant(W)[:, perm[t]] * x exactly
  act       lattice inputs, a transcendental activation: exact accumulator, fp64 function at 2e-5 * max(1, |ref|)

A plain module, no fixtures.  The layouts (operand B-fragment order, tiled payloads, scales) are restated here from the comments of
rwkv_kernels.hip / rwkv_kernels.h, independently of the kernels' index arithmetic."""
import json
import os
import subprocess
import zlib
from dataclasses import dataclass, field

import numpy as np

from oracle import rwkv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, INT8, NF4 = 0, 1, 2
FMT_NAME = {F16: "f16", INT8: "int8", NF4: "nf4"}
ACT_NONE, ACT_TANH, ACT_SIGMOID, ACT_RELU2, ACT_SILU, ACT_DECAY7 = range(6)
POST_NONE, POST_MUL, POST_MIX = range(3)
EXACT_ACTS = (ACT_NONE, ACT_RELU2)
GUARD = 256
SENT32, SENT16 = 0x7FC0DEAD, 0x7EAD
SK_KMAX, TILE_MIN_T, MAXP = 320, 193, 8
FP32_TOL = 2e-5                                                   # the project's Fp32 tolerance (tests/test_gpu_dims.py), for the `act` family only
HEADROOM = 1 << 20                                                # sum |w||x| / quantum of every output stays below: four bits under fp32's 24
TILE_KIND = {s: (0 if s <= 5 else 1 if s <= 9 else 2 if s <= 11 else 3) for s in range(13)}   # gemm_plan.h kTileShapes
TILE_ROWS = {0: 256, 1: 128, 2: 64, 3: 64, 4: 64, 5: 128, 6: 64, 7: 128, 8: 128, 9: 256, 10: 128, 11: 128, 12: 128}


@dataclass
class Prob:
    rows: int
    K: int
    fmt: int = F16
    xoff: int = 0
    act: int = ACT_NONE
    post: int = POST_NONE
    partial: bool = False
    bias: object = False            # False, True (small integers) or "big" (beyond the fp16 range: the operand output saturates)
    f32: bool = True                # writes fp32 output
    opd: bool = False               # writes operand output (hi, and lo unless no_lo)
    no_lo: bool = False
    # filled by layout():
    ocol: int = -1
    hcol: int = -1
    mcol: int = 0


@dataclass
class Case:
    name: str
    group: str                      # which GPU test runs it
    T: int
    probs: list
    hilo: bool = False
    mode: int = -1                  # -1 plan_gemm decides, 2 plan_decode(force_spb), 1 tile_geometry(tile_shape, ksplit)
    force_spb: int = 0
    tile_shape: int = -1
    ksplit: int = 0
    xcd: int = -1
    family: str = "lattice"
    xpad: int = 0                   # ldx = max(xoff + K) + xpad
    lo_mode: str = "both"           # onehot: where the token's power of two sits: "hi", "lo", "both"
    perm_base: int = 0              # onehot: token t reads column ((perm_base + t) * 7) % K
    single: bool = False
    ldx: int = 0
    ldo: int = 0
    ldh: int = 0
    ldm: int = 0
    nslab: int = 1
    tags: tuple = ()

    def layout(self):
        """Column offsets of the problems' outputs in the shared buffers: gaps between and beyond them stay sentinels."""
        o = h = 0
        for i, p in enumerate(self.probs):
            if p.f32:
                p.ocol = o + (4 if i else 0)
                o = p.ocol + p.rows
            if p.opd:
                p.hcol = h + (32 if i else 0)
                h = (p.hcol + p.rows + 31) // 32 * 32
            p.mcol = max(p.ocol, 0)
        self.ldo = o + 8 if o else 0
        self.ldh = h + 32 if h else 0
        self.ldm = self.ldo if any(p.post != POST_NONE for p in self.probs) else 0
        self.ldx = max(p.xoff + p.K for p in self.probs) + self.xpad
        self.nslab = 9 if any(p.partial for p in self.probs) else 2
        if self.single:
            self.ldo, self.nslab = 16, 1
        return self


def seed_of(case):
    return zlib.crc32(case.name.encode())


# ------------------------------------------------------------------------------------------------
# the operand layout (rwkv_kernels.hip "Activation operands ... in MFMA B-FRAGMENT order"): 1 KiB tiles of 16 tokens x 32 k, tile (t / 16, k / 32)
# of a [ceil16(T)][ld] operand at tile index (t / 16) * (ld / 32) + k / 32; inside a tile lane ((k / 8) % 4) * 16 + t % 16 owns 8 consecutive k
# ------------------------------------------------------------------------------------------------
def pack_opd(x):
    """[T16][ld] -> flat operand (T16 % 16 == 0, ld % 32 == 0)."""
    T16, ld = x.shape
    return np.ascontiguousarray(x.reshape(T16 // 16, 16, ld // 32, 4, 8).transpose(0, 2, 3, 1, 4)).reshape(-1)


def unpack_opd(flat, T16, ld):
    return np.ascontiguousarray(flat.reshape(T16 // 16, ld // 32, 4, 16, 8).transpose(0, 3, 1, 2, 4)).reshape(T16, ld)


def opd_off(t, k, ld):
    """Direct transcription of the kernels' own index function, for the element-by-element cross-check of the two above."""
    return ((t >> 4) * (ld >> 5) + (k >> 5)) * 512 + ((((k >> 3) & 3) << 4) + (t & 15)) * 8 + (k & 7)


# ------------------------------------------------------------------------------------------------
# tiled weights (rwkv_kernels.h DMat, rwkv_kernels.hip "Load-time layout kernels"): strips of 16 rows, 1 KiB tiles contiguous along K
# ------------------------------------------------------------------------------------------------
def tiled_f16(W):
    """fp16: tile = 16 rows x 32 k, lane l holds row l % 16, k = (l / 16) * 8 + [0, 8)."""
    rows, K = W.shape
    return np.ascontiguousarray(W.reshape(rows // 16, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4)).reshape(-1)


def tiled_int8(q, a, b):
    """Int8: tile = 16 rows x 64 k, lane (row % 16) + 16 * ((k % 32) / 8), byte (k % 64 >= 32 ? 8 : 0) + k % 8; scales half2{a, b} as
    [strip][K / 256][16 rows][128-block of the pair]."""
    rows, K = q.shape
    pay = np.ascontiguousarray(q.reshape(rows // 16, 16, K // 64, 2, 4, 8).transpose(0, 2, 4, 1, 3, 5)).reshape(-1)
    ab = np.stack([a, b], axis=-1).reshape(rows // 16, 16, K // 256, 2, 2)
    return pay, np.ascontiguousarray(ab.transpose(0, 2, 1, 3, 4)).reshape(-1)


def tiled_nf4(idx, am):
    """NF4: tile = 16 rows x 128 k, lane (row % 16) + 16 * ((k % 32) / 8), byte (k % 128) / 32 * 4 + (k % 8) % 4, low nibble for k % 8 < 4;
    scales half as [strip][K / 256][16 rows][64-block of the four]."""
    rows, K = idx.shape
    n = idx.reshape(rows // 16, 16, K // 128, 4, 4, 2, 4)          # strip, row, tile, k-step, k / 8 % 4, nibble, byte
    byte = (n[:, :, :, :, :, 0, :] | (n[:, :, :, :, :, 1, :] << 4)).astype(np.uint8)
    pay = np.ascontiguousarray(byte.transpose(0, 2, 4, 1, 3, 5)).reshape(-1)
    sc = am.reshape(rows // 16, 16, K // 256, 4)
    return pay, np.ascontiguousarray(sc.transpose(0, 2, 1, 3)).reshape(-1)


def payload_sizes(p):
    n = p.rows * p.K
    return {F16: (n * 2, 0), INT8: (n, p.rows * (p.K // 128) * 4), NF4: (n // 2, p.rows * (p.K // 64) * 2)}[p.fmt]


def expected_payload(p, W):
    """(payload bytes, scale bytes) the load-time kernel must write for raw weights W, from the oracle's quantisers."""
    if p.fmt == F16:
        return tiled_f16(W).view(np.uint8), np.zeros(0, np.uint8)
    if p.fmt == INT8:
        pay, sc = tiled_int8(*R.quant_int8(W))
    else:
        pay, sc = tiled_nf4(*R.quant_nf4(W))
    return pay.view(np.uint8), sc.view(np.uint8)


QUANT_OF = {F16: 0, INT8: R.QUANT_INT8, NF4: R.QUANT_NF4}


def fake_quant(p, W):
    return R.fake_quant(W, QUANT_OF[p.fmt])


# ------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------
def lattice_weights(rng, p, small=False):
    rows, K = p.rows, p.K
    if p.fmt == F16:
        w = rng.integers(-2 if small else -3, (2 if small else 3) + 1, (rows, K))
        return w.astype(np.float16)
    if p.fmt == INT8:
        nb = K // 128
        b = rng.integers(-10, -5, (rows, nb, 1))
        q = -16 * b + rng.integers(-24, 25, (rows, nb, 128))          # |w| <= 1.5 around zero ...
        pos = np.argsort(rng.random((rows, nb, 128)), axis=2)[:, :, :2]
        np.put_along_axis(q, pos[:, :, :1], 0, axis=2)                 # ... and both ends of the code range in every block
        np.put_along_axis(q, pos[:, :, 1:], 255, axis=2)
        return (b + q / 16.0).reshape(rows, K).astype(np.float16)
    nb = K // 64
    am = 2.0 ** rng.integers(-2, 2, (rows, nb, 1))
    s = rng.choice([-1.0, 0.0, 1.0], (rows, nb, 64), p=[0.4, 0.2, 0.4])
    pos = np.argsort(rng.random((rows, nb, 64)), axis=2)[:, :, :2]
    np.put_along_axis(s, pos[:, :, :1], -1.0, axis=2)
    np.put_along_axis(s, pos[:, :, 1:], 1.0, axis=2)
    return (s * am).reshape(rows, K).astype(np.float16)


W_QUANTUM = {F16: 1.0, INT8: 1.0 / 16, NF4: 0.25}


def onehot_weights(rng, p):
    """Arbitrary fp16 values: scales that are no powers of two, a block offset, some constant blocks (Int8 a = 0, NF4 absmax = 0)."""
    rows, K = p.rows, p.K
    blk = 128 if p.fmt == INT8 else 64
    nb = K // blk
    scale = rng.uniform(0.01, 3.0, (rows, nb, 1))
    shift = rng.uniform(-1.0, 1.0, (rows, nb, 1)) * (p.fmt == INT8)
    w = rng.standard_normal((rows, nb, blk)) * scale + shift
    w[rng.random((rows, nb)) < 0.04] = 0.37
    w[rng.random((rows, nb)) < 0.03] = 0.0
    return w.reshape(rows, K).astype(np.float16)


def make(case):
    """Inputs of a case: dict(xhi, xlo [T][ldx] f16, m0, m1 [T][ldm] f32, W [list of f16 rows x K], bias [list of f32 | None], perm)."""
    rng = np.random.default_rng(seed_of(case))
    T, ldx = case.T, case.ldx
    d = {"perm": None}
    if case.family == "onehot":
        K = case.probs[0].K
        perm = ((case.perm_base + np.arange(T)) * 7) % K              # 7 is coprime to K: T <= K distinct columns, K consecutive indices reach every one
        d["perm"] = perm
        xhi = np.zeros((T, ldx), np.float16)
        xlo = np.zeros((T, ldx), np.float16)
        e = rng.integers(-2, 3, T).astype(np.float64)
        col = case.probs[0].xoff + perm
        if case.lo_mode in ("hi", "both"):
            xhi[np.arange(T), col] = 2.0 ** e
        if case.lo_mode == "lo":
            xlo[np.arange(T), col] = 2.0 ** e
        if case.lo_mode == "both":
            xlo[np.arange(T), col] = 2.0 ** (e - 3)
        d["W"] = [onehot_weights(rng, p) for p in case.probs]
    else:
        act = case.family == "act"
        if act:
            xhi = (rng.integers(-1, 2, (T, ldx)) / 8.0).astype(np.float16)
            xlo = (rng.integers(-1, 2, (T, ldx)) / 32.0).astype(np.float16)
        else:
            xhi = rng.integers(-2, 3, (T, ldx)).astype(np.float16)
            xlo = (rng.integers(-3, 4, (T, ldx)) / 4.0).astype(np.float16)    # to the kernel lo is just a second operand: deliberately not tiny
        d["W"] = [lattice_weights(rng, p, small=act) for p in case.probs]
    d["xhi"], d["xlo"] = xhi, (xlo if case.hilo else None)
    d["m0"] = rng.integers(-3, 4, (T, case.ldm)).astype(np.float32) if case.ldm else None
    d["m1"] = rng.integers(-2, 3, (T, case.ldm)).astype(np.float32) if case.ldm else None
    d["bias"] = []
    for p in case.probs:
        if p.bias == "big":                                            # beyond +-65504, just inside, and values whose lo part is not zero
            b = rng.choice([70000.0, -70000.0, 65504.0, 40001.0, -33333.0, 3.0], p.rows)
        elif p.bias:
            b = rng.integers(-4, 5, p.rows).astype(np.float64)
        else:
            b = None
        d["bias"].append(None if b is None else b.astype(np.float32))
    return d


# ------------------------------------------------------------------------------------------------
# the reference, fp64
# ------------------------------------------------------------------------------------------------
def x_of(case, d, p):
    x = d["xhi"].astype(np.float64)
    if case.hilo:
        x = x + d["xlo"].astype(np.float64)
    return x[:, p.xoff:p.xoff + p.K]


def act64(act, v):
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    if act == ACT_TANH:
        return np.tanh(v)
    if act == ACT_SIGMOID:
        return sig(v)
    if act == ACT_RELU2:
        return np.maximum(v, 0.0) ** 2
    if act == ACT_SILU:
        return v * sig(v)
    if act == ACT_DECAY7:
        return np.exp(-0.606531 * sig(v))
    return v


def epilogue(case, d, i, acc, stages=None):
    """v = act(acc + bias[row]); POST_MUL: v *= m0; POST_MIX: v = m0 + m1 * v.  `stages` collects every intermediate (exactness proof)."""
    p = case.probs[i]
    v = acc if d["bias"][i] is None else acc + d["bias"][i].astype(np.float64)[None, :]
    s = [v]
    v = act64(p.act, v)
    s.append(v)
    if p.post != POST_NONE:
        m0 = d["m0"][:, p.mcol:p.mcol + p.rows].astype(np.float64)
        if p.post == POST_MUL:
            v = v * m0
        else:
            prod = d["m1"][:, p.mcol:p.mcol + p.rows].astype(np.float64) * v
            s.append(prod)
            v = m0 + prod
        s.append(v)
    if stages is not None:
        stages.extend(s)
    return v


def reference(case, d, i, k0=0, k1=None, stages=None):
    """[T][rows] of problem i, K restricted to [k0, k1) (a partial slab of a decode K split)."""
    p = case.probs[i]
    Wq = fake_quant(p, d["W"][i]).astype(np.float64)
    x = x_of(case, d, p)
    k1 = p.K if k1 is None else k1
    acc = x[:, k0:k1] @ Wq[:, k0:k1].T
    if stages is not None:
        stages.append(acc)
    return epilogue(case, d, i, acc, stages)


def split_hilo(v):
    """hi = rn(clamp(v)), lo = rn(clamp(v) - hi) of an fp32 value (rwkv_kernels.hip split_hilo)."""
    c = np.clip(v.astype(np.float32), np.float32(-65504.0), np.float32(65504.0))
    hi = c.astype(np.float16)
    lo = (c - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def kstep_sums(case, d, i):
    """[T][rows][K / 32]: the partial sum of every 32-k step."""
    p = case.probs[i]
    Wq = fake_quant(p, d["W"][i]).astype(np.float64)
    x = x_of(case, d, p)
    return np.einsum("tjk,rjk->trj", x.reshape(case.T, p.K // 32, 32), Wq.reshape(p.rows, p.K // 32, 32))


def headroom(case, d, i):
    """max over outputs of sum |w||x| / quantum."""
    p = case.probs[i]
    Wq = np.abs(fake_quant(p, d["W"][i]).astype(np.float64))
    xq = {"lattice": (1.0, 0.25), "act": (1.0 / 8, 1.0 / 32)}[case.family][int(case.hilo)]
    return float((np.abs(d["xhi"].astype(np.float64))[:, p.xoff:p.xoff + p.K] @ Wq.T
                  + (np.abs(d["xlo"].astype(np.float64))[:, p.xoff:p.xoff + p.K] @ Wq.T if case.hilo else 0.0)).max() / (W_QUANTUM[p.fmt] * xq))


# ------------------------------------------------------------------------------------------------
# the probe's files
# ------------------------------------------------------------------------------------------------
def padded_x(case, x):
    """rows T .. ceil16(T) - 1 hold NaN halfs: nothing of them may reach a valid output."""
    T16 = (case.T + 15) // 16 * 16
    full = np.full((T16, case.ldx), SENT16, np.uint16)
    full[:case.T] = x.view(np.uint16)
    return pack_opd(full)


def write_cases(path, cases, datas):
    with open(path, "wb") as f:
        f.write(np.array([0x42525047, len(cases)], np.int32).tobytes())
        for c, d in zip(cases, datas):
            f.write(np.array([c.T, int(c.hilo), c.mode, c.force_spb, c.tile_shape, c.ksplit, c.xcd, len(c.probs), c.ldx, c.ldo, c.ldh, c.ldm,
                              c.nslab, int(c.single)], np.int32).tobytes())
            f.write(padded_x(c, d["xhi"]).tobytes())
            if c.hilo:
                f.write(padded_x(c, d["xlo"]).tobytes())
            if c.ldm:
                f.write(d["m0"].tobytes())
                f.write(d["m1"].tobytes())
            for p, W, b in zip(c.probs, d["W"], d["bias"]):
                f.write(np.array([p.rows, p.K, p.fmt, p.xoff, p.act, p.post, int(p.partial), int(b is not None), p.mcol,
                                  p.ocol, p.hcol, int(not p.no_lo)], np.int32).tobytes())
                f.write(np.ascontiguousarray(W).tobytes())
                if b is not None:
                    f.write(b.tobytes())


def read_results(path, cases):
    """Per case None (unsupported) or dict(out u32 [nslab * T * ldo + GUARD], ohi / olo u16, payload / scales per problem)."""
    buf = np.fromfile(path, np.uint8)
    pos, res = 0, []

    def take(nbytes, dtype):
        nonlocal pos
        assert pos + nbytes <= buf.size, "the result file ends early"
        a = buf[pos:pos + nbytes].view(dtype)
        pos += nbytes
        return a
    for c in cases:
        if int(take(4, np.int32)[0]) != 0:
            res.append(None)
            continue
        T16 = (c.T + 15) // 16 * 16
        n_out = c.nslab * c.T * c.ldo + GUARD if c.ldo else 0
        n_oh = T16 * c.ldh + GUARD if c.ldh else 0
        r = {"out": take(n_out * 4, np.uint32), "ohi": take(n_oh * 2, np.uint16), "olo": take(n_oh * 2, np.uint16), "pay": [], "sc": []}
        for p in c.probs:
            a, b = payload_sizes(p)
            r["pay"].append(take(a, np.uint8))
            r["sc"].append(take(b, np.uint8))
        res.append(r)
    assert pos == buf.size, "the result file is longer than the cases account for"
    return res


# ------------------------------------------------------------------------------------------------
# the planner on the CPU (tests/cpp/gemm_plan_test.cpp, argument "probe"), and the probe's build
# ------------------------------------------------------------------------------------------------
def shape_words(p):
    """rows K fmt partial kcopies smallk (gemm_plan.h shape_of)."""
    kcopies = p.post != POST_MIX and p.act == ACT_NONE and not p.bias and not p.opd
    smallk = p.xoff == 0 and p.f32 and not p.opd and p.post == POST_NONE
    return [p.rows, p.K, p.fmt, int(p.partial), int(kcopies), int(smallk)]


def plan_line(c):
    words = [c.T, int(c.hilo), c.mode, c.force_spb, c.tile_shape, c.ksplit, c.xcd, c.nslab, len(c.probs)]
    return " ".join(str(w) for w in words + [x for p in c.probs for x in shape_words(p)])


def build_planner(out_dir):
    exe = os.path.join(str(out_dir), "gemm_plan_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "gemm_plan_test.cpp"), "-o", exe])
    return exe


def plan_cpu(exe, cases):
    out = subprocess.run([exe, "probe"], input="\n".join(plan_line(c) for c in cases) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    plans = [json.loads(l) for l in out.stdout.splitlines()]
    assert len(plans) == len(cases)
    return plans


def compile_probe(out_dir):
    """hipcc -c of the probe for gfx950 (no GPU needed)."""
    from ai00_server_amd import build as B
    return B.compile_probe("gemm_probe", os.path.join(str(out_dir), "gemm_probe.o"))


def build_probe():
    """The probe, linked against the kernel objects the library build leaves in the tree (ai00_server_amd/build.py build_probe)."""
    from ai00_server_amd import build as B
    return B.build_probe("gemm_probe", verbose=False)


# ------------------------------------------------------------------------------------------------
# checking one case's results against the reference
# ------------------------------------------------------------------------------------------------
def f32_of(u32):
    return u32.view(np.float32).astype(np.float64)


def explain(case, d, i, t, row, diff):
    """Which 32-k steps' partial sums would explain a difference (dropped: -sum, doubled: +sum)."""
    s = kstep_sums(case, d, i)[t, row]
    hit = [f"k-step {j} (k {32 * j}..{32 * j + 31}) {'doubled' if diff == s[j] else 'dropped'}" for j in range(s.size) if s[j] != 0 and abs(diff) == abs(s[j])]
    return "; ".join(hit[:4]) if hit else "no single k-step"


def mismatch(case, d, i, got, want, what, plan, exact=True, ratios=None):
    """[] or one message naming the case, the plan, the count and the first few differing elements."""
    if exact:
        bad = ~(got == want)                                            # NaN never equals: a sentinel or a NaN in a valid output is a difference
    else:
        tol = FP32_TOL * np.maximum(1.0, np.abs(want))
        err = np.abs(got - want)
        bad = ~(err <= tol)
        if ratios is not None:
            ratios.append((case.name, i, float(np.nanmax(err / tol))))
    if not bad.any():
        return []
    idx = np.argwhere(bad)
    p = case.probs[i]
    first = []
    for t, row in idx[:4]:
        why = explain(case, d, i, t, row, got[t, row] - want[t, row]) if exact and np.isfinite(got[t, row]) and case.family != "onehot" else ""
        first.append(f"(t {t}, row {row}, got {got[t, row]!r}, want {want[t, row]!r}{', ' + why if why else ''})")
    return [f"{case.name}: problem {i} ({FMT_NAME[p.fmt]} {p.rows}x{p.K}) {what}: {len(idx)} of {got.size} elements differ: {' '.join(first)}; plan {json.dumps(plan)}"]


def check_case(case, d, res, plan, ratios=None):
    """Every failure of one case as a list of messages (empty: the case passed)."""
    if res is None or plan.get("status") != "ran":
        return [f"{case.name}: the probe refused the case: {plan}"]
    msgs = []
    T, T16 = case.T, (case.T + 15) // 16 * 16
    # the load-time kernels: payload and scales against the oracle's quantisers, in the layout rwkv_kernels.h states
    for i, p in enumerate(case.probs):
        pay, sc = expected_payload(p, d["W"][i])
        if not np.array_equal(res["pay"][i], pay):
            msgs.append(f"{case.name}: problem {i}: tiled payload differs in {int((res['pay'][i] != pay).sum())} bytes of {pay.size}")
        if not np.array_equal(res["sc"][i], sc):
            msgs.append(f"{case.name}: problem {i}: scales differ in {int((res['sc'][i] != sc).sum())} bytes of {sc.size}")
    if case.single:
        got = f32_of(res["out"][:256]).reshape(16, 16)
        return msgs + mismatch(case, d, 0, got, reference(case, d, 0), "single MFMA", plan)
    exact = case.family != "act"
    tile = plan["path"] == "tile"
    if case.ldo:
        body = res["out"][:case.nslab * T * case.ldo].reshape(case.nslab, T, case.ldo)
        owned = np.zeros(body.shape, bool)
        for i, p in enumerate(case.probs):
            if not p.f32:
                continue
            ksb = plan["probs"][i]["ksb"]
            sl = (slice(None), slice(p.ocol, p.ocol + p.rows))
            owned[:ksb, :, p.ocol:p.ocol + p.rows] = True
            slabs = f32_of(body[:ksb][(slice(None),) + sl])
            want = reference(case, d, i)
            if ksb == 1:
                msgs += mismatch(case, d, i, slabs[0], want, "fp32 output", plan, exact, ratios)
            else:
                msgs += mismatch(case, d, i, slabs.sum(axis=0), want, f"sum of the {ksb} partial slabs", plan)
                if not tile:                                            # decode K split: slab kb is the reference over k in [kb Kb, (kb + 1) Kb)
                    Kb = plan["probs"][i]["Kb"]
                    for kb in range(ksb):
                        msgs += mismatch(case, d, i, slabs[kb], reference(case, d, i, kb * Kb, (kb + 1) * Kb), f"partial slab {kb} (k {kb * Kb}..{(kb + 1) * Kb - 1})", plan)
        stray = ~owned & (body != SENT32)
        if stray.any():
            msgs.append(f"{case.name}: {int(stray.sum())} fp32 elements outside what the launch owns were written, first (slab, t, column) {np.argwhere(stray)[:4].tolist()}; plan {json.dumps(plan)}")
        if (res["out"][-GUARD:] != SENT32).any():
            msgs.append(f"{case.name}: the guard band behind the fp32 buffer was written; plan {json.dumps(plan)}")
    if case.ldh:
        for key in ("ohi", "olo"):
            body = unpack_opd(res[key][:T16 * case.ldh], T16, case.ldh)
            owned = np.zeros(body.shape, bool)
            for i, p in enumerate(case.probs):
                if not p.opd or (key == "olo" and p.no_lo):
                    continue
                owned[:T, p.hcol:p.hcol + p.rows] = True
                hi, lo = split_hilo(reference(case, d, i))
                got = body[:T, p.hcol:p.hcol + p.rows].view(np.float16).astype(np.float64)
                msgs += mismatch(case, d, i, got, (hi if key == "ohi" else lo).astype(np.float64), f"operand output {key[1:]}", plan)
            stray = ~owned & (body != SENT16)
            if stray.any():
                msgs.append(f"{case.name}: {int(stray.sum())} halfs of operand output {key[1:]} outside what the launch owns were written (rows >= T, columns between "
                            f"the problems), first (t, column) {np.argwhere(stray)[:4].tolist()}; plan {json.dumps(plan)}")
            if (res[key][-GUARD:] != SENT16).any():
                msgs.append(f"{case.name}: the guard band behind operand output {key[1:]} was written; plan {json.dumps(plan)}")
    return msgs


def emulate(case, d, plan):
    """What a correct probe run returns, built from the reference: the CPU test runs check_case on it (and on a damaged copy)."""
    T, T16 = case.T, (case.T + 15) // 16 * 16
    r = {"pay": [], "sc": []}
    out = np.full(case.nslab * T * case.ldo + GUARD if case.ldo else 0, SENT32, np.uint32)
    oh = {k: np.full((T16, case.ldh), SENT16, np.uint16) for k in ("ohi", "olo")}
    body = out[:case.nslab * T * case.ldo].reshape(case.nslab, T, case.ldo) if case.ldo else None
    for i, p in enumerate(case.probs):
        pay, sc = expected_payload(p, d["W"][i])
        r["pay"].append(pay)
        r["sc"].append(sc)
        ksb = plan["probs"][i]["ksb"]
        if p.f32:
            Kb = p.K // ksb
            for kb in range(ksb):
                k1 = p.K if kb == ksb - 1 else (kb + 1) * Kb
                body[kb, :, p.ocol:p.ocol + p.rows] = reference(case, d, i, kb * Kb, k1).astype(np.float32).view(np.uint32)
        if p.opd:
            hi, lo = split_hilo(reference(case, d, i))
            oh["ohi"][:T, p.hcol:p.hcol + p.rows] = hi.view(np.uint16)
            if not p.no_lo:
                oh["olo"][:T, p.hcol:p.hcol + p.rows] = lo.view(np.uint16)
    r["out"] = out
    for k in oh:
        r[k] = np.concatenate([pack_opd(oh[k]), np.full(GUARD, SENT16, np.uint16)]) if case.ldh else np.zeros(0, np.uint16)
    return r


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------
def _three(rows, K, kf16=None, **kw):
    """One problem per weight format (the fp16 one may have its own K: the tail variants)."""
    return [Prob(rows, kf16 or K, F16, **kw), Prob(rows, K, INT8, **kw), Prob(rows, K, NF4, **kw)]


def decode_variant_cases():
    """All 20 instantiations (NT, HILO) x SHOT x TAIL, each with the three formats in one launch.  Single shot needs spb <= 2 (fp16 holds two
    rounds); not single shot: five strips per block, more than any format holds (streamed), or the ring (17..32 rows, quantised, plain)."""
    out = []
    for hilo, group in ((False, "decode_plain"), (True, "decode_hilo")):
        for T in ((1, 15, 16, 17, 31, 32, 33, 64, 65, 192) if not hilo else (1, 16, 17, 32, 65)):
            for shot in (True, False):
                for tail in (False, True):
                    nt2_plain = not hilo and 17 <= T <= 32
                    rows = 272 if (nt2_plain and shot) else 80         # NT = 2 plain is single shot only beside an fp16 matrix of more than 256 rows
                    if T in (15, 31, 33, 64, 192) and (shot != tail):  # the in-between step sizes take two of the four combinations
                        continue
                    probs = _three(rows, 512, kf16=416 if tail else 512)
                    out.append(Case(f"dec-T{T}-{'hilo' if hilo else 'plain'}-{'shot' if shot else 'stream'}-{'tail' if tail else 'full'}", group, T, probs,
                                    hilo=hilo, mode=2, force_spb=(2 if shot else 5)))
    # the ring: quantised only, 17..32 rows, plain (fp16 of at most 256 rows rides along)
    out.append(Case("dec-ring-T17", "decode_plain", 17, [Prob(96, 1024, INT8), Prob(96, 1024, NF4), Prob(64, 256, F16)], mode=2, tags=("ring",)))
    out.append(Case("dec-ring-T32-spb3", "decode_plain", 32, [Prob(112, 768, INT8), Prob(80, 768, NF4)], mode=2, force_spb=3, tags=("ring",)))
    # streamed at eight strips per block, ragged last block (rows / 16 = 13)
    out.append(Case("dec-stream8-T1", "decode_plain", 1, _three(208, 512), mode=2, force_spb=8))
    out.append(Case("dec-stream8-T40-hilo", "decode_hilo", 40, _three(208, 512), hilo=True, mode=2, force_spb=8))
    return out


def decode_split_cases():
    g = "decode_split"
    out = []
    # fp16 with K % 256 != 0, with and without a K split (the split keeps 32-k alignment: Kb = 208, 104 is no multiple of 32)
    out.append(Case("dec-tail-nosplit", g, 3, [Prob(48, 416, F16)], mode=2))
    out.append(Case("dec-tail-split", g, 5, [Prob(48, 1248, F16, partial=True)], mode=2, tags=("tail_split",)))
    out.append(Case("dec-tail-split-T20", g, 20, [Prob(48, 1248, F16, partial=True)], mode=2, tags=("tail_split",)))
    # the tail flag set by an fp16 problem while an Int8 problem rides along
    out.append(Case("dec-tail-beside-int8", g, 9, [Prob(64, 352, F16), Prob(64, 512, INT8)], mode=2, tags=("tail_mixed",)))
    # K > 2560: more slices than waves; the hi + lo two-tile deal of eight waves over ten slices at K = 2560
    out.append(Case("dec-K2816-int8", g, 1, [Prob(32, 2816, INT8)], mode=2))
    out.append(Case("dec-K3072-f16-T20", g, 20, [Prob(32, 3072, F16)], mode=2))
    out.append(Case("dec-K2816-nf4-T40", g, 40, [Prob(32, 2816, NF4)], mode=2))
    out.append(Case("dec-K2560-hilo-T17", g, 17, [Prob(32, 2560, INT8), Prob(32, 2560, F16)], hilo=True, mode=2, tags=("deal8of10",)))
    out.append(Case("dec-K2816-hilo-T32", g, 32, [Prob(32, 2816, NF4)], hilo=True, mode=2))
    # partial problems at every valid ksb 2..8: the planner takes the largest valid split <= 8 of a small matrix
    for ksb, K, fmt in ((2, 512, INT8), (3, 768, NF4), (4, 1024, INT8), (5, 1280, NF4), (6, 1536, INT8), (7, 1792, INT8), (8, 2048, NF4),
                        (2, 64, F16), (3, 96, F16), (5, 160, F16), (7, 224, F16), (6, 192, F16)):
        out.append(Case(f"dec-partial-ksb{ksb}-{FMT_NAME[fmt]}-K{K}", g, 1 + ksb, [Prob(48, K, fmt, partial=True, post=POST_MUL if ksb == 4 else POST_NONE)],
                        mode=2, tags=(f"ksb{ksb}",)))
    out.append(Case("dec-partial-hilo-T33", g, 33, [Prob(48, 1536, INT8, partial=True)], hilo=True, mode=2))
    # the engine's r/k/v/g + decay LoRA launch in small: quantised 256-row matrices beside a 64-row fp16 one, epilogues differ, xoff != 0, ldx > K
    for T, hilo in ((1, False), (18, False), (40, True)):
        probs = [Prob(256, 256, INT8, xoff=0), Prob(256, 256, INT8, xoff=256, bias=True), Prob(256, 256, INT8, xoff=512, post=POST_MUL),
                 Prob(256, 256, NF4, xoff=768, act=ACT_RELU2, opd=True), Prob(64, 256, F16, xoff=1024, post=POST_MIX, bias=True)]
        out.append(Case(f"dec-five-T{T}{'-hilo' if hilo else ''}", g, T, probs, hilo=hilo, mode=2, xpad=64, tags=("five",)))
    # large grids: more than 1024 blocks at one wave (spb = 8, unforced), and an unforced spb = 2
    out.append(Case("dec-grid-16400x256", g, 1, [Prob(16400, 256, F16)], mode=2, tags=("big_grid",)))
    out.append(Case("dec-grid-4112x2048", g, 2, [Prob(4112, 2048, INT8)], mode=2, tags=("spb_unforced",)))
    return out


def smallk_cases():
    out = []
    for T in (1, 17, 64):
        for hilo in (False, True):
            probs = [Prob(80, 32, F16), Prob(48, 64, F16, bias=True), Prob(112, 96, F16, act=ACT_RELU2, bias=True), Prob(32, 320, F16)]   # 5 + 3 + 7 + 2 strips
            out.append(Case(f"smallk-T{T}{'-hilo' if hilo else ''}", "smallk", T, probs, hilo=hilo))
    return out


def tile_cases():
    """Every shape with every format and operand form it supports, ragged row tiles (144 / 272 rows), T in {193, 250, 257}."""
    out = []
    Ts = (193, 250, 257)
    for shape in range(13):
        kind = TILE_KIND[shape]
        group = f"tile_kind{kind}"
        rows = 272 if TILE_ROWS[shape] == 256 else 144                   # one full row tile and a ragged one
        forms = [True] if kind == 3 else [False] if kind == 2 else ([False] if shape == 5 else [False, True])
        for j, hilo in enumerate(forms):
            T = Ts[(shape + j) % 3]
            pipelined = kind >= 2
            # chunked: fp16 K % 128 != 0; pipelined: K = 128 x odd (fp16 only: quantised K is a multiple of 256)
            probs = [Prob(rows, 384 if pipelined else 416, F16, bias=True, opd=(shape % 2 == 0)), Prob(rows, 512, INT8, post=POST_MUL),
                     Prob(rows if shape % 3 else 48, 256 if shape % 2 else 768, NF4, act=ACT_RELU2)]
            out.append(Case(f"tile{shape}-T{T}{'-hilo' if hilo else ''}", group, T, probs, hilo=hilo, mode=1, tile_shape=shape, ksplit=1,
                            xcd=(shape + j) % 3, tags=("multi",)))
    # K copies 2, 3, 4 of a linear problem: chunked, pipelined plain, pipelined hi + lo
    for ks in (2, 3, 4):
        out.append(Case(f"tile4-kcopies{ks}", "tile_kind0", 193, [Prob(80, 1184, F16, partial=True)], mode=1, tile_shape=4, ksplit=ks, xcd=1, tags=(f"kc{ks}",)))
        out.append(Case(f"tile11-kcopies{ks}", "tile_kind2", 250, [Prob(144, 1280, INT8, partial=True)], mode=1, tile_shape=11, ksplit=ks, xcd=ks % 3, tags=(f"kc{ks}",)))
        out.append(Case(f"tile12-kcopies{ks}", "tile_kind3", 257, [Prob(144, 896, F16, partial=True)], hilo=True, mode=1, tile_shape=12, ksplit=ks, xcd=2 - ks % 3, tags=(f"kc{ks}",)))
        out.append(Case(f"tile7-kcopies{ks}", "tile_kind1", 193, [Prob(144, 768, NF4, partial=True)], mode=1, tile_shape=7, ksplit=ks, xcd=0, tags=(f"kc{ks}",)))
    # what the planner itself picks at these sizes (no forced shape)
    out.append(Case("tile-auto-plain", "tile_kind2", 193, [Prob(144, 512, INT8), Prob(64, 512, F16, act=ACT_RELU2)], tags=("auto",)))
    out.append(Case("tile-auto-hilo", "tile_kind3", 250, [Prob(144, 512, NF4)], hilo=True, tags=("auto",)))
    out.append(Case("tile-auto-linear", "tile_kind0", 193, [Prob(144, 2304, F16, partial=True)], tags=("auto",)))
    return out


def onehot_cases():
    out = []
    for fmt, group in ((INT8, "onehot_int8"), (NF4, "onehot_nf4")):
        K, rows = 512, 48
        modes = ("hi", "lo", "both")
        for j in range(8):                                              # 8 x 64 tokens = every column of K = 512 (perm start differs per case)
            lm = modes[j % 3]
            out.append(Case(f"onehot-{FMT_NAME[fmt]}-dec{j}-{lm}", group, 64, [Prob(rows, K, fmt)], hilo=lm != "hi", mode=2, family="onehot", lo_mode=lm, perm_base=64 * j))
        out.append(Case(f"onehot-{FMT_NAME[fmt]}-T1", group, 1, [Prob(rows, K, fmt)], mode=2, family="onehot", lo_mode="hi"))
        out.append(Case(f"onehot-{FMT_NAME[fmt]}-tile4", group, 257, [Prob(rows, K, fmt)], mode=1, tile_shape=4, ksplit=1, family="onehot", lo_mode="hi"))
        out.append(Case(f"onehot-{FMT_NAME[fmt]}-tile11", group, 256, [Prob(rows, K, fmt)], mode=1, tile_shape=11, ksplit=1, family="onehot", lo_mode="hi"))
        out.append(Case(f"onehot-{FMT_NAME[fmt]}-tile12", group, 256, [Prob(rows, K, fmt)], hilo=True, mode=1, tile_shape=12, ksplit=1, family="onehot", lo_mode="both", perm_base=256))
    return out


def epilogue_cases():
    g = "epilogues"
    out = []
    # exact: bias, RELU2, POST_MUL, POST_MIX, operand output (both + fp32; operand only; hi only), saturation
    exact = [Prob(48, 256, F16, bias=True, post=POST_MIX), Prob(48, 256, NF4, act=ACT_RELU2, bias=True, post=POST_MUL),
             Prob(64, 256, INT8, bias=True, opd=True), Prob(48, 256, F16, f32=False, opd=True, act=ACT_RELU2), Prob(32, 256, INT8, f32=False, opd=True, no_lo=True)]
    for T, hilo, mode, shape in ((7, False, 2, -1), (20, True, 2, -1), (50, False, 2, -1), (193, False, 1, 3), (193, True, 1, 12), (250, False, 1, 10)):
        out.append(Case(f"epi-exact-T{T}{'-hilo' if hilo else ''}", g, T, [Prob(**vars(p)) for p in exact], hilo=hilo, mode=mode, tile_shape=shape,
                        ksplit=1 if mode == 1 else 0, tags=("epi_exact",)))
        out.append(Case(f"epi-saturate-T{T}{'-hilo' if hilo else ''}", g, T, [Prob(64, 256, F16, bias="big", opd=True), Prob(32, 256, INT8, bias="big", f32=False, opd=True)],
                        hilo=hilo, mode=mode, tile_shape=shape, ksplit=1 if mode == 1 else 0, tags=("saturate",)))
    # transcendental activations: exact accumulator, fp64 function at the Fp32 tolerance
    acts = [Prob(48, 256, F16, act=ACT_TANH, bias=True), Prob(48, 256, INT8, act=ACT_SIGMOID), Prob(48, 256, NF4, act=ACT_SILU, post=POST_MUL),
            Prob(48, 256, F16, act=ACT_DECAY7, bias=True, post=POST_MIX)]
    for T, hilo, mode, shape in ((5, False, 2, -1), (33, True, 2, -1), (193, False, 1, 4), (193, True, 1, 12), (193, False, 1, 11)):
        out.append(Case(f"epi-act-T{T}{'-hilo' if hilo else ''}-{'tile' + str(shape) if mode == 1 else 'dec'}", g, T, [Prob(**vars(p)) for p in acts], hilo=hilo,
                        mode=mode, tile_shape=shape, ksplit=1 if mode == 1 else 0, family="act", tags=("act",)))
    # one bare 16x16x32 MFMA on a lattice tile: the instrument for a finding that sits in the instruction, not in a kernel (DESIGN.md "GEMM probe")
    out.append(Case("single-mfma", g, 16, [Prob(16, 32, F16)], single=True))
    out.append(Case("epi-act-smallk", g, 17, [Prob(48, 96, F16, act=ACT_TANH, bias=True), Prob(48, 320, F16, act=ACT_SIGMOID)], family="act", tags=("act",)))
    return out


def all_cases():
    cases = decode_variant_cases() + decode_split_cases() + smallk_cases() + tile_cases() + onehot_cases() + epilogue_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return [c.layout() for c in cases]


GROUPS = ("decode_plain", "decode_hilo", "decode_split", "smallk", "tile_kind0", "tile_kind1", "tile_kind2", "tile_kind3", "onehot_int8", "onehot_nf4", "epilogues")


# ------------------------------------------------------------------------------------------------
# what the table must reach, read off plan lines (the CPU planner's, and again the lines the probe printed on the GPU)
# ------------------------------------------------------------------------------------------------
def coverage_gaps(cases, plans):
    """[] or what of the coverage list of DESIGN.md "GEMM probe" the table does not reach."""
    gaps = []
    ran = [(c, p) for c, p in zip(cases, plans) if p.get("status") == "ran" and not c.single]
    dec = [(c, p) for c, p in ran if p["path"] == "decode"]
    # decode: the 20 instantiations, each with every format
    for nt, hilo in ((1, 0), (1, 1), (2, 0), (2, 1), (4, 0)):
        for shot in (0, 1):
            for tail in (0, 1):
                fm = {q.fmt for c, p in dec if (p["NT"], p["hilo"], p["single_shot"], p["tail"]) == (nt, hilo, shot, tail) for q in c.probs}
                if fm != {F16, INT8, NF4}:
                    gaps.append(f"gemm_kernel<NT {nt}, HILO {hilo}, SHOT {shot}, TAIL {tail}> with formats {sorted(fm)}")
    need_T = {1, 15, 16, 17, 31, 32, 33, 64, 65, 192}
    if not need_T <= {c.T for c, _ in dec}:
        gaps.append(f"decode T {sorted(need_T - {c.T for c, _ in dec})}")
    maxr = lambda fmt, nt, hilo: 2 if (nt == 4 or (nt == 2 and hilo)) else (2 if fmt == F16 else (3 if (nt == 2 or hilo) else 4))
    probs_of = lambda sel: [(c, p, q, g) for c, p in sel for q, g in zip(c.probs, p["probs"])]
    D = probs_of(dec)
    checks = {
        "the ring (17-32 rows, quantised, plain, not single shot)": any(p["NT"] == 2 and not p["hilo"] and not p["single_shot"] and q.fmt != F16 and g["spb"] <= maxr(q.fmt, 2, 0) for c, p, q, g in D),
        "streamed, spb = 8": any(g["spb"] == 8 and c.force_spb == 8 for c, p, q, g in D),
        "ragged last block": any((q.rows // 16) % g["spb"] for c, p, q, g in D if g["spb"] > 1),
        "fp16 K % 256 != 0 without a K split": any(q.fmt == F16 and q.K % 256 and g["ksb"] == 1 for c, p, q, g in D),
        "fp16 Kb % 256 != 0 with a K split": any(q.fmt == F16 and g["Kb"] % 256 and g["ksb"] > 1 for c, p, q, g in D),
        "tail launch with an Int8 problem riding along": any(p["tail"] and {F16, INT8} <= {q.fmt for q in c.probs} for c, p in dec),
        "K > 2560, more slices than waves": any(q.K > 2560 and g["nslice"] > g["nw"] for c, p, q, g in D),
        "hi + lo two-tile deal of eight waves over ten slices": any(p["hilo"] and p["NT"] == 2 and g["nw"] == 8 and g["nslice"] == 10 for c, p, q, g in D),
        "five-problem launch": any(len(c.probs) == 5 and any(q.xoff for q in c.probs) and c.ldx > max(q.xoff + q.K for q in c.probs) for c, p in dec),
        "more than 1024 one-strip blocks at one wave (spb = 8 unforced)": any(g["nw"] == 1 and g["spb"] == 8 and not c.force_spb and q.rows // 16 > 1024 for c, p, q, g in D),
        "unforced spb > 1": any(g["spb"] > 1 and not c.force_spb for c, p, q, g in D),
        "two passes of the t0 loop": any(c.T > 16 * p["NT"] for c, p in dec),
    }
    for ksb in range(2, 9):
        checks[f"partial problem at ksb = {ksb}"] = any(q.partial and g["ksb"] == ksb for c, p, q, g in D)
    sk = [(c, p) for c, p in ran if p["path"] == "smallk"]
    checks["small-K K in {32, 64, 96, 320}"] = {32, 64, 96, 320} <= {q.K for c, p in sk for q in c.probs}
    checks["small-K T in {1, 17, 64}, plain and hi + lo"] = {(T, h) for T in (1, 17, 64) for h in (0, 1)} <= {(c.T, int(c.hilo)) for c, p in sk}
    checks["small-K strip count no multiple of four"] = any(p["total_blocks"] % 4 for c, p in sk if len(c.probs) > 1)
    tl = [(c, p) for c, p in ran if p["path"] == "tile"]
    for shape in range(13):
        forms = [1] if shape == 12 else [0] if shape in (5, 10, 11) else [0, 1]
        for h in forms:
            fm = {q.fmt for c, p in tl if p["shape"] == shape and p["hilo"] == h for q in c.probs}
            if fm != {F16, INT8, NF4}:
                gaps.append(f"tile shape {shape} hilo {h} with formats {sorted(fm)}")
    checks["tile T in {193, 250, 257}"] = {193, 250, 257} <= {c.T for c, p in tl}
    for rt in (64, 128, 256):
        checks[f"ragged row tile on a {rt}-row shape"] = any(TILE_ROWS[p["shape"]] == rt and q.rows % rt for c, p in tl for q in c.probs)
    checks["K % 128 != 0 on a chunked shape"] = any(p["shape"] <= 9 and q.K % 128 for c, p in tl for q in c.probs)
    checks["K = 128 x odd on a pipelined shape"] = {10, 11, 12} <= {p["shape"] for c, p in tl for q in c.probs if (q.K // 128) % 2 and q.K % 128 == 0}
    for ks in (2, 3, 4):
        checks[f"tile K copies {ks}"] = any(p["ksplit"] == ks and c.probs[0].partial for c, p in tl)
    checks["xcd_map 0, 1, 2"] = {0, 1, 2} <= {p["xcd_map"] for c, p in tl}
    checks["multi-problem tile launch"] = any(len(c.probs) > 1 for c, p in tl)
    checks["operand output with fp32, operand only, saturated"] = (any(q.opd and q.f32 for c, p in ran for q in c.probs) and any(q.opd and not q.f32 for c, p in ran for q in c.probs)
                                                                 and any(q.bias == "big" and q.opd for c, p in ran for q in c.probs))
    for a in (ACT_TANH, ACT_SIGMOID, ACT_RELU2, ACT_SILU, ACT_DECAY7):
        checks[f"activation {a} on the decode and tile kernels"] = {"decode", "tile"} <= {p["path"] for c, p in ran for q in c.probs if q.act == a}
    return gaps + [k for k, ok in checks.items() if not ok]

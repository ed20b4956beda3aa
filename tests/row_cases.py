"""The row / WKV / state probe's case table, shared by tests/test_gpu_row_exact.py (runs tests/cpp/row_probe.hip on the GPU) and
tests/test_row_cases_cpu.py (proves the table without one): one launch per case (DESIGN.md "Row and recurrence probe").

Every buffer a launch may write starts as a NaN pattern (0x7FC0DEAD / 0x7EAD) with a guard band on both sides; state and token-shift
buffers carry real values in the slots of the step and the pattern in every other slot and in the gap between slots; input rows of no
sequence hold the pattern too.  What a launch does not own must hold its bits afterwards, and no NaN may reach an owned output.

  exact     WKV inputs from grids on which every product and partial sum is an fp32 value: the state must meet the float64 reference
            in every bit, whichever kernel form ran.  V5: w in {0, 1} (+ 1/2 up to 8 rows), k / v / state in quarters.  V6: time_decay
            -200, integer D2 and td, row sums in [0, 60] (w = 1) or [205, 280] (w = 0).  V7: w7 as V5, k * k_k with four non-zeros of
            equal power-of-two magnitude per (token, head) (kappa = +-1/2 exactly), a in {0, 1/2, 1} and non-zero on kappa's support on
            at most two tokens per sequence (each such token deepens the state's binary fraction by three bits).
  general   random values (V6 decays spread over [-12, 4]) against float64 at the project's Fp32 bound 2e-5 * max(1, |ref|):
            elementwise for the row kernels and WKV-4, the infinity norm of the (slot, head) tile or (row, head) for WKV state and y.

Layouts, stated once.  Activations r / k / v / g / w7 / a7 / vg7 / v_first are fp32 [T][C] row-major, td is [T][Dd], D2 is f16 [C][Dd].
The internal WKV state of a slot is [H][64][64] = T[head][p = value index][q = key index] at state + slot * slot_stride.  Every f16
operand (y, the mixes, ln_out) is read through the operand layout of rwkv_kernels.hip `opd_off`: 1 KiB tiles of 16 tokens x 32 k, tile
(t / 16, k / 32) of a [ceil16(T)][ld] operand at tile index (t / 16) * (ld / 32) + k / 32, lane ((k / 8) % 4) * 16 + t % 16 owning 8 k."""
import os
import zlib
from dataclasses import dataclass, field

import numpy as np

from tests.gemm_cases import pack_opd, unpack_opd                   # the operand layout, cross-checked against opd_off by test_gemm_cases_cpu.py
from tests.probe_io import GUARD, SENT16, SENT32, Buf, b_in, b_out, bits, read_results, write_cases as write_case_file   # the container, stated once, there

FP32_TOL = 2e-5                                                    # the project's Fp32 tolerance (tests/test_gpu_dims.py)
F32, F64 = np.float32, np.float64
K_WKV, K_WKV4, K_LN_SHIFT, K_EMBED, K_LN_OUT, K_STATE_PACK = range(6)
KIND_NAME = ("wkv", "wkv4", "ln_shift", "embed", "ln_out", "state_pack")
PARAMS = (("version", "H", "C", "n_seq", "dense", "slot_stride", "Dd", "layer", "ldh", "max_rows", "multi_row", "T", "nslots"),
          ("C", "n_seq", "dense", "slot_stride", "ldh", "multi_row", "T", "nslots"),
          ("T", "C", "np", "pstride", "sx_slot_stride", "dense", "mode", "nmix", "ldh", "nslots"),
          ("T", "C", "V"),
          ("n_out", "C", "np", "pstride", "ldh", "T"),
          ("L", "C", "H", "v4", "transposed", "to_slab", "layer_only"))
_ROLES = ("seq_slot seq_begin seq_len state r k v g wdec u td D2 w7 a7 vg7 k_k k_a r_k v_first lnw lnb yhi ylo x_in x_out P sx slot prev last "
          "xx dx mu0 mu1 mu2 mu3 mu4 mu5 ohi0 ohi1 ohi2 ohi3 ohi4 ohi5 olo0 olo1 olo2 olo3 olo4 olo5 emb token out_rows slab sxa sxf wkvst").split()
ROLE = {n: i for i, n in enumerate(_ROLES)}                        # the Role enum of row_probe.hip
SEQ_SLOT = (3, 0, 4, 1)                                            # five slots, slot 2 is in no step
NSLOTS = 5
GROUPS = ("wkv5", "wkv6", "wkv7", "wkv4", "ln_shift_1024", "ln_shift_512", "embed_ln_out", "state_pack")


@dataclass
class Case:
    name: str
    group: str
    kind: int
    p: dict
    o: dict = field(default_factory=dict)                          # what make() needs beyond the launcher arguments


def seed_of(case):
    return zlib.crc32(case.o.get("seed", case.name).encode())


def nan32(shape):
    return np.full(shape, SENT32, np.uint32).view(F32)


def ceil16(t):
    return (t + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------
# the case file and the result file (tests/cpp/row_probe.hip)
# ------------------------------------------------------------------------------------------------
def write_cases(path, cases, datas):
    return write_case_file(path, 0x42525052, cases, datas, lambda c: PARAMS[c.kind], ROLE)


def plan_line(c):
    """The JSON line the probe prints for the case."""
    return {"case": c.name, "launcher": KIND_NAME[c.kind], **{k: int(c.p[k]) for k in PARAMS[c.kind]}}


def compile_probe(out_dir):
    from ai00_server_amd import build as B
    return B.compile_probe("row_probe", os.path.join(str(out_dir), "row_probe.o"))


def build_probe():
    from ai00_server_amd import build as B
    return B.build_probe("row_probe", verbose=False)


# ------------------------------------------------------------------------------------------------
# which kernel a launch reaches: the launchers' selection restated from their arguments alone
# ------------------------------------------------------------------------------------------------
def kernel_of(line):
    k = line["launcher"]
    if k == "wkv":
        v, Dd, multi, mr = line["version"], line["Dd"], line["multi_row"], line["max_rows"]
        chunk_dd = v != 6 or Dd in (64, 128)
        dd = Dd if v == 6 else 64
        if multi and 0 < mr <= 8 and chunk_dd:
            return f"wkv_chunk<{v},{dd},8>"
        if multi and chunk_dd:
            return f"wkv_chunk<{v},{dd},32>"
        return f"wkv_kernel v{v} Dd{dd} " + ("dense" if line["dense"] else "multi" if multi else "rows")
    if k == "wkv4":
        return "wkv4_chunk_kernel" if line["multi_row"] else "wkv4_kernel"
    if k == "ln_shift":
        T, C = line["T"], line["C"]
        xcd = int(T > 64)
        if T <= 256:
            return f"ln_shift<{1 if C <= 4096 else 2},1024> xcd{xcd}"
        return f"ln_shift<{1 if C <= 2048 else 2 if C <= 4096 else 4},512> xcd{xcd}"
    if k in ("embed", "ln_out"):
        C = line["C"]
        return f"{k}<{1 if C <= 1024 else 2 if C <= 2048 else 4 if C <= 4096 else 8}>"
    return "state_pack v4%d tr%d to_slab%d layer%d" % (line["v4"], line["transposed"], line["to_slab"], line["layer_only"])


WANTED = ([f"wkv_chunk<{v},{d},{ch}>" for v, d in ((5, 64), (6, 64), (6, 128), (7, 64)) for ch in (8, 32)]
          + ["wkv_kernel v5 Dd64 dense", "wkv_kernel v7 Dd64 dense"] + [f"wkv_kernel v6 Dd{d} dense" for d in (32, 64, 96, 128)]
          + [f"wkv_kernel v6 Dd{d} multi" for d in (32, 96)]
          + ["wkv4_kernel", "wkv4_chunk_kernel"]
          + ["ln_shift<1,1024> xcd0", "ln_shift<1,1024> xcd1", "ln_shift<2,1024> xcd0", "ln_shift<2,1024> xcd1",
             "ln_shift<1,512> xcd1", "ln_shift<2,512> xcd1", "ln_shift<4,512> xcd1"]
          + [f"{k}<{pt}>" for k in ("embed", "ln_out") for pt in (1, 2, 4, 8)]
          + ["state_pack v40 tr%d to_slab%d layer%d" % (tr, ts, lo) for tr in (0, 1) for ts in (0, 1) for lo in (-1, 1)]
          + ["state_pack v41 tr0 to_slab%d layer%d" % (ts, lo) for ts in (0, 1) for lo in (-1, 1)])


def coverage_gaps(lines):
    ran = {kernel_of(l) for l in lines}
    gaps = [w for w in WANTED if w not in ran]
    short_declined = [l for l in lines if l["launcher"] == "wkv" and l["version"] == 6 and l["Dd"] in (32, 96) and l["multi_row"] and 0 < l["max_rows"] <= 8]
    if not short_declined:
        gaps.append("no multi-row V6 step with Dd 32 / 96 and max_rows <= 8 (the short form must decline it)")
    for form in ("wkv_chunk<7,64,8>", "wkv_chunk<7,64,32>", "wkv_kernel v7 Dd64 dense"):      # v_first written (layer 0) and read (any other layer)
        layers = {l["layer"] != 0 for l in lines if kernel_of(l) == form}
        if layers != {False, True}:
            gaps.append(f"{form} ran with layer == 0: {False in layers}, with layer != 0: {True in layers}")
    if not any(l["launcher"] == "wkv" and l["multi_row"] and l["max_rows"] == 0 for l in lines):
        gaps.append("no multi-row step with max_rows = 0")
    return gaps


# ------------------------------------------------------------------------------------------------
# comparing with the reference
# ------------------------------------------------------------------------------------------------
def ulp16(x):
    """Spacing of f16 at |x| (normal range down to the subnormal step)."""
    _, e = np.frexp(np.abs(x))
    return np.exp2(np.maximum(e - 1, -14) - 10.0)


def f16_sat(x):
    return np.clip(x, -65504.0, 65504.0)


def first_bad(bad, got, want, n=3):
    return " ".join(f"({tuple(int(v) for v in i)}: got {got[tuple(i)]!r}, want {want[tuple(i)]!r})" for i in np.argwhere(bad)[:n])


class Checker:
    def __init__(self, case, ratios):
        self.c, self.msgs, self.ratios, self.worst = case, [], ratios, 0.0

    def say(self, what, bad, got, want):
        self.msgs.append(f"{self.c.name}: {what}: {int(bad.sum())} of {bad.size} elements differ: {first_bad(bad, got, want)}")

    def same_bits(self, what, got, want):
        """Bit for bit (uint views): ownership, permutations, exact grids."""
        got, want = np.asarray(got), np.asarray(want)
        bad = got != want
        if bad.any():
            self.say(what, bad, got, want)

    def exact(self, what, got32, want64):
        """fp32 results against float64 values that are fp32 values: every bit (a NaN never equals)."""
        bad = ~(got32.astype(F64) == want64)
        if bad.any():
            self.say(what + " (exact grid)", bad, got32, want64)

    def close(self, what, got, want, bound, slack=0.0):
        """|got - want| <= bound + slack; the ratio kept is the part of the error beyond `slack` (half an f16 step of a hi-only operand) over bound."""
        err = np.abs(got - want)
        bad = ~(err <= bound + slack)
        with np.errstate(invalid="ignore"):
            r = float(np.max(np.where(np.isnan(err), np.inf, np.maximum(err - slack, 0.0) / bound))) if err.size else 0.0
        self.worst = max(self.worst, r)
        if bad.any():
            self.say(f"{what} (worst error / bound {r:.3f})", bad, got, want)

    def guards(self, res):
        for role, a in res.items():
            s = SENT32 if a.dtype == np.uint32 else SENT16
            if (a[:GUARD] != s).any() or (a[-GUARD:] != s).any():
                self.msgs.append(f"{self.c.name}: the guard band of {role} was written")

    def operand(self, what, res, hi, lo, T, ld, rows, C, want, bound):
        """An f16 operand [ceil16(T)][ld]: `rows` (output row -> row of want / bound) are owned in columns < C; the rest holds the pattern."""
        T16 = ceil16(T)
        h = unpack_opd(res[hi][GUARD:-GUARD], T16, ld)
        own = np.zeros((T16, ld), bool)
        idx = np.array(sorted(rows), int)
        own[idx, :C] = True
        if (h[~own] != SENT16).any():
            self.msgs.append(f"{self.c.name}: {what} hi: {int((h[~own] != SENT16).sum())} unowned elements written (rows {sorted(set(np.argwhere((h != SENT16) & ~own)[:, 0]))[:6]})")
        src = np.array([rows[i] for i in idx], int)
        w = f16_sat(want[src])
        g = h.view(np.float16)[idx, :C].astype(F64)
        if lo is not None:
            l = unpack_opd(res[lo][GUARD:-GUARD], T16, ld)
            if (l[~own] != SENT16).any():
                self.msgs.append(f"{self.c.name}: {what} lo: {int((l[~own] != SENT16).sum())} unowned elements written")
            self.close(what + " hi + lo", g + l.view(np.float16)[idx, :C].astype(F64), w, bound[src])
        else:
            self.close(what + " hi", g, w, bound[src], 0.5 * ulp16(w))


def ew_bound(want):
    return FP32_TOL * np.maximum(1.0, np.abs(want))


def head_bound(want):
    """[.., C] -> the bound of every element from the infinity norm over its head's 64 channels."""
    m = np.abs(want).reshape(want.shape[:-1] + (-1, 64)).max(-1, keepdims=True)
    return np.broadcast_to(FP32_TOL * np.maximum(1.0, m), m.shape[:-1] + (64,)).reshape(want.shape)


# ------------------------------------------------------------------------------------------------
# WKV V5 / V6 / V7
# ------------------------------------------------------------------------------------------------
def layout(lens, rng):
    """Sequences with gaps of unowned rows between them; T is no multiple of 16."""
    t, seqs = 1, []
    for s, n in zip(SEQ_SLOT, lens):
        seqs.append((s, t, n))
        t += n + int(rng.integers(1, 3))
    T = t + 1
    if T % 16 == 0:
        T += 3
    return seqs, T


def rows_of(seqs):
    return [t for _, b, n in seqs for t in range(b, b + n)]


def quarters(rng, shape, lim=8, q=4.0):
    return (rng.integers(-lim, lim + 1, shape) / q).astype(F32)


def make_wkv(c):
    P, o = c.p, c.o
    rng = np.random.default_rng(seed_of(c))
    ver, H, C, T, Dd, exact = P["version"], P["H"], P["C"], P["T"], P["Dd"], o["exact"]
    seqs = o["seqs"]
    own = rows_of(seqs)
    short = max(n for _, _, n in seqs) <= 8
    d = {"seqs": seqs}

    def act(vals):                                                  # [T][C] with the pattern on rows of no sequence
        a = nan32((T, vals.shape[1]))
        a[own] = vals[own]
        return a
    wset = np.array([0.0, 1.0, 0.5] if short else [0.0, 1.0], F32)
    st = nan32((NSLOTS, P["slot_stride"]))
    for s, _, _ in seqs:
        st[s, :H * 4096] = quarters(rng, H * 4096) if exact else rng.normal(0, 0.5, H * 4096)
    d["state"] = st
    d["r"] = act(rng.normal(0, 0.7, (T, C)).astype(F32))
    d["g"] = act(rng.normal(0, 1.0, (T, C)).astype(F32))
    d["lnw"] = rng.uniform(0.5, 1.5, C).astype(F32)
    d["lnb"] = rng.normal(0, 0.1, C).astype(F32)
    k = quarters(rng, (T, C)) if exact else rng.normal(0, 0.6, (T, C)).astype(F32)
    v = quarters(rng, (T, C)) if exact else rng.normal(0, 0.8, (T, C)).astype(F32)
    if ver in (5, 6):
        d["u"] = quarters(rng, C) if exact else rng.normal(0, 0.5, C).astype(F32)
    if ver == 5:
        d["wdec"] = wset[rng.integers(0, len(wset), C)] if exact else np.exp(-np.exp(rng.uniform(-8, 1, C))).astype(F32)
    if ver == 6:
        if exact:                                                   # row sum = D2[c][d1] + D2[c][d2], d1 in the lower half of Dd, d2 in the upper
            d["wdec"] = np.full(C, -200.0, F32)
            D2 = rng.integers(0, 31, (C, Dd)).astype(np.float16)
            big = rng.random((C, Dd // 2)) < 0.4
            D2[:, :Dd // 2][big] = rng.integers(205, 251, int(big.sum())).astype(np.float16)
            td = np.zeros((T, Dd), F32)
            td[np.arange(T), rng.integers(0, Dd // 2, T)] = 1.0
            td[np.arange(T), Dd // 2 + rng.integers(0, Dd // 2, T)] = 1.0
        else:                                                       # decays spread over [-12, 4]: w from nearly 1 to nearly 0
            d["wdec"] = rng.uniform(-11, 3, C).astype(F32)
            D2 = rng.normal(0, 0.1, (C, Dd)).astype(np.float16)
            td = rng.normal(0, 0.3, (T, Dd)).astype(F32)
        d["D2"] = D2
        tdn = nan32((T, Dd))
        tdn[own] = td[own]
        d["td"] = tdn
    if ver == 7:
        layer = P["layer"]
        if exact:
            k_k = np.where(rng.random(C) < 0.5, 0.0, rng.choice([1.0, 2.0], C)).astype(F32)
            for h in range(H):                                      # at least eight channels of every head carry k_k
                k_k[h * 64 + rng.choice(64, 8, replace=False)] = 1.0
            k = np.where(k_k == 0, quarters(rng, (T, C), 4, 2.0), 0.0).astype(F32)
            a7 = rng.choice([0.0, 0.5, 1.0], (T, C)).astype(F32)
            for _, b, n in seqs:
                dirty = set(rng.choice(n, min(n, 2), replace=False).tolist())
                for i in range(n):
                    for h in range(H):
                        cand = h * 64 + np.flatnonzero(k_k[h * 64:h * 64 + 64])
                        Q = rng.choice(cand, 4, replace=False)
                        x = rng.choice([0.5, 1.0])
                        k[b + i, Q] = rng.choice([-1.0, 1.0], 4) * x / k_k[Q]
                        if i not in dirty:
                            a7[b + i, Q] = 0.0
            d["k_a"] = rng.choice([0.0, 0.5, 1.0], C).astype(F32)
            d["w7"] = act(wset[rng.integers(0, len(wset), (T, C))])
            vg = rng.choice([0.0, 1.0], (T, C)).astype(F32)
            vf = quarters(rng, (T, C))
        else:
            k_k = rng.uniform(0.5, 1.5, C).astype(F32)
            a7 = rng.uniform(0, 1, (T, C)).astype(F32)
            d["k_a"] = rng.uniform(0, 1, C).astype(F32)
            d["w7"] = act(np.exp(-0.606531 / (1 + np.exp(-rng.normal(0, 2, (T, C))))).astype(F32))
            vg = rng.uniform(0, 1, (T, C)).astype(F32)
            vf = rng.normal(0, 0.8, (T, C)).astype(F32)
        zs, zb, zn = seqs[2]                                        # one token of one head with k == 0: the fmaxf(sqrtf(ss), 1e-12f) branch
        k[zb + zn // 2, :64] = 0.0
        d["k_k"], d["a7"] = k_k, act(a7)
        d["r_k"] = rng.normal(0, 0.3, C).astype(F32)
        if layer != 0:
            d["vg7"], d["v_first"] = act(vg), act(vf)
    d["k"], d["v"] = act(k), act(v)
    dense = P["dense"]
    bufs = []
    if not dense:
        bufs += [b_in("seq_slot", np.array([s for s, _, _ in seqs], np.int32)), b_in("seq_begin", np.array([b for _, b, _ in seqs], np.int32)),
                 b_in("seq_len", np.array([n for _, _, n in seqs], np.int32))]
    bufs.append(b_in("state", d["state"], back=True))
    for nm in ("r", "k", "v", "g", "wdec", "u", "td", "D2", "w7", "a7", "vg7", "k_k", "k_a", "r_k", "lnw", "lnb"):
        if nm in d:
            bufs.append(b_in(nm, d[nm]))
    if ver == 7:
        bufs.append(b_in("v_first", d["v_first"], back=True) if P["layer"] != 0 else b_out("v_first", T * C, 4))
    bufs.append(b_out("yhi", ceil16(T) * P["ldh"], 2))
    if o["ylo"]:
        bufs.append(b_out("ylo", ceil16(T) * P["ldh"], 2))
    d["bufs"] = bufs
    return d


def _tree(x):
    while x.shape[-1] > 1:
        if x.shape[-1] % 2:                                          # an odd level (Dd = 96): the last element rides up alone
            x = np.concatenate([x, np.zeros(x.shape[:-1] + (1,), x.dtype)], -1)
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def wkv_eval(c, d, ft, order=None):
    """The WKV step in dtype `ft`: (state [NSLOTS][H][64][64] in the internal T[p][q] layout, y [T][C] or None).  order None: numpy's own
    summation; 0: token by token with sequential sums; 1: the packed form (V5 / V6: two tokens folded into one update; V7: pairwise tree sums)."""
    P = c.p
    ver, H, C, T, exact = P["version"], P["H"], P["C"], P["T"], c.o["exact"]
    g = lambda n: d[n].astype(ft)
    st = d["state"][:, :H * 4096].astype(ft).reshape(NSLOTS, H, 64, 64).copy()
    y = np.full((T, C), np.nan, ft)
    r, k, v, gt, lnw, lnb = g("r"), g("k"), g("v"), g("g"), g("lnw"), g("lnb")
    one = ft(1.0)

    def dot(a, b):                                                  # sum over the last axis of a * b
        x = a * b
        if order == 0:
            acc = np.zeros(x.shape[:-1], ft)
            for q in range(x.shape[-1]):
                acc = acc + x[..., q]
            return acc
        return _tree(x) if order == 1 else x.sum(-1)

    for slot, b, n in d["seqs"]:
        for h in range(H):
            cs = slice(h * 64, h * 64 + 64)
            S = st[slot, h]
            if ver != 7:
                u = g("u")[cs]
                ws = []
                for t in range(b, b + n):
                    if ver == 5:
                        w = g("wdec")[cs]
                    else:
                        w = np.exp(-np.exp(g("wdec")[cs] + dot(d["D2"][cs].astype(ft), g("td")[t][None, :])))
                        if exact:
                            w = w.astype(F32).astype(ft)            # on the grid w is within 1e-60 of 0 or 1; the proof checks it is one of them
                    ws.append(w)
                if order == 1:                                      # two tokens per update: S <- kv2 + w2 kv1 + (w2 w1) S
                    i = 0
                    while i < n:
                        t = b + i
                        kv1 = np.outer(v[t, cs], k[t, cs])
                        if i + 1 < n:
                            kv2 = np.outer(v[t + 1, cs], k[t + 1, cs])
                            S = (kv2 + ws[i + 1] * kv1) + (ws[i + 1] * ws[i]) * S
                            i += 2
                        else:
                            S = kv1 + ws[i] * S
                            i += 1
                    st[slot, h] = S
                    continue
                for i, t in enumerate(range(b, b + n)):
                    kv = np.outer(v[t, cs], k[t, cs])               # [p = value][q = key]
                    out = dot(u * kv + S, r[t, cs][None, :])
                    S = kv + ws[i] * S
                    y[t, cs] = _gn(out, lnw[cs], lnb[cs], ft) * gt[t, cs]
            else:
                kk_p, ka_p, rk_p = g("k_k")[cs], g("k_a")[cs], g("r_k")[cs]
                for t in range(b, b + n):
                    kk = k[t, cs] * kk_p
                    ss = dot(kk, kk)
                    kn = kk / np.maximum(np.sqrt(ss), ft(1e-12))
                    av = g("a7")[t, cs]
                    k2 = k[t, cs] * (one + (av - one) * ka_p)
                    vv = v[t, cs]
                    if P["layer"] != 0:
                        vv = vv + (g("v_first")[t, cs] - vv) * g("vg7")[t, cs]
                    sa = dot(S, (-kn)[None, :])
                    S = S * g("w7")[t, cs][None, :] + np.outer(sa, kn * av) + np.outer(vv, k2)
                    out = dot(S, r[t, cs][None, :])
                    y[t, cs] = (_gn(out, lnw[cs], lnb[cs], ft) + dot(r[t, cs] * k2, rk_p) * vv) * gt[t, cs]
            st[slot, h] = S
    return st, (None if order == 1 and ver != 7 else y)


def _gn(out, w, b, ft):
    mean = out.sum() / ft(64)
    dd = out - mean
    var = (dd * dd).sum() / ft(64)
    return dd / np.sqrt(var + ft(64e-5)) * w + b


def check_wkv(c, d, res, ck):
    P, o = c.p, c.o
    H, C, T, ldh = P["H"], P["C"], P["T"], P["ldh"]
    st64, y64 = wkv_eval(c, d, F64)
    got = res["state"][GUARD:-GUARD].reshape(NSLOTS, -1)
    init = bits(d["state"]).reshape(NSLOTS, -1)
    used = [s for s, _, _ in d["seqs"]]
    for s in range(NSLOTS):
        if s not in used:
            ck.same_bits(f"state of slot {s}, not in the step", got[s], init[s])
    ck.same_bits("the gaps between state slots", got[:, H * 4096:], init[:, H * 4096:])
    gs = got[used, :H * 4096].view(F32).reshape(len(used), H, 64, 64)
    if o["exact"]:
        ck.exact("state", gs, st64[used])
    else:
        m = np.abs(st64[used]).max((2, 3), keepdims=True)
        ck.close("state", gs.astype(F64), st64[used], np.broadcast_to(FP32_TOL * np.maximum(1.0, m), gs.shape))
    own = rows_of(d["seqs"])
    if P["version"] == 7:
        vf = res["v_first"][GUARD:-GUARD].reshape(T, C)
        want = bits(d["v_first"]).reshape(T, C) if P["layer"] != 0 else np.full((T, C), SENT32, np.uint32)
        if P["layer"] == 0:
            want[own] = bits(d["v"]).reshape(T, C)[own]
        ck.same_bits("v_first", vf, want)
    ck.operand("y", res, "yhi", "ylo" if o["ylo"] else None, T, ldh, {t: t for t in own}, C, y64, head_bound(np.nan_to_num(y64)))


# ------------------------------------------------------------------------------------------------
# WKV-4
# ------------------------------------------------------------------------------------------------
def make_wkv4(c):
    P, o = c.p, c.o
    rng = np.random.default_rng(seed_of(c))
    C, T = P["C"], P["T"]
    seqs = o["seqs"]
    own = rows_of(seqs)
    d = {"seqs": seqs}
    st = nan32((NSLOTS, P["slot_stride"]))
    for i, (s, _, _) in enumerate(seqs):
        st[s, :C] = rng.normal(0, 1, C)
        st[s, C:2 * C] = rng.uniform(0.5, 3, C)
        st[s, 2 * C:3 * C] = -1e30 if i % 2 == 0 else np.round(rng.normal(0, 10, C) * 1024) / 1024     # a fresh slot, or a running maximum (on the 2^-10 grid)
        if i % 2 == 0:
            st[s, :2 * C] = 0.0
    d["state"] = st

    def act(vals):
        a = nan32((T, C))
        a[own] = vals[own]
        return a
    r = (1 / (1 + np.exp(-rng.normal(0, 1.5, (T, C))))).astype(F32)
    # |k| up to several tens.  (aa, bb, pp) is compared ELEMENT by element although a common factor e^-pp is free between them: with arbitrary values every
    # pp + w rounds at pp's own magnitude, and a run of 33 rows without a new maximum sums those roundings into aa and bb (the plain fp32 restatement
    # itself reached 0.97 of the bound that way).  So k, u, w and the running maxima lie on a grid of 2^-10: pp + w, u + k and every exponent's argument
    # are then exact, and what is left to compare is expf, the products and the division.
    grid = lambda x: (np.round(np.asarray(x, F64) * 1024) / 1024).astype(F32)
    k = grid(rng.normal(0, 1, (T, C)) * rng.choice([1.0, 8.0, 25.0], C))
    v = rng.normal(0, 1, (T, C)).astype(F32)
    sat = 7                                                         # this channel's r * wkv leaves the f16 range, with both signs
    r[:, sat] = 1.0
    v[:, sat] = np.where(np.arange(T) % 2 == 0, 3e5, -3e5)
    for s, _, _ in seqs:
        if st[s, 2 * C] > -1e29:
            st[s, sat] = 2e5 * st[s, C + sat]
    d["r"], d["k"], d["v"] = act(r), act(k), act(v)
    d["wdec"] = np.minimum(grid(-np.exp(rng.uniform(-6, 2.5, C))), F32(-1 / 1024))      # wide decays: w from -0.002 to -12
    d["u"] = grid(rng.normal(0, 2, C))
    bufs = []
    if not P["dense"]:
        bufs += [b_in("seq_slot", np.array([s for s, _, _ in seqs], np.int32)), b_in("seq_begin", np.array([b for _, b, _ in seqs], np.int32)),
                 b_in("seq_len", np.array([n for _, _, n in seqs], np.int32))]
    bufs.append(b_in("state", st, back=True))
    bufs += [b_in(nm, d[nm]) for nm in ("r", "k", "v", "wdec", "u")]
    bufs.append(b_out("yhi", ceil16(T) * P["ldh"], 2))
    if o["ylo"]:
        bufs.append(b_out("ylo", ceil16(T) * P["ldh"], 2))
    d["bufs"] = bufs
    return d


def wkv4_eval(c, d, ft):
    C, T = c.p["C"], c.p["T"]
    st = d["state"][:, :3 * C].astype(ft).reshape(NSLOTS, 3, C).copy()
    y = np.full((T, C), np.nan, ft)
    u, w = d["u"].astype(ft), d["wdec"].astype(ft)
    with np.errstate(over="ignore", under="ignore"):
        for slot, b, n in d["seqs"]:
            aa, bb, pp = st[slot]
            for t in range(b, b + n):
                r, k, v = (d[nm][t].astype(ft) for nm in ("r", "k", "v"))
                ww = u + k
                p = np.maximum(pp, ww)
                e1, e2 = np.exp(pp - p), np.exp(ww - p)
                y[t] = r * ((e1 * aa + e2 * v) / (e1 * bb + e2))
                ww = pp + w
                p = np.maximum(ww, k)
                e1, e2 = np.exp(ww - p), np.exp(k - p)
                aa, bb, pp = e1 * aa + e2 * v, e1 * bb + e2, p
            st[slot] = aa, bb, pp
    return st, y


def check_wkv4(c, d, res, ck):
    P = c.p
    C, T = P["C"], P["T"]
    st64, y64 = wkv4_eval(c, d, F64)
    got = res["state"][GUARD:-GUARD].reshape(NSLOTS, -1)
    init = bits(d["state"]).reshape(NSLOTS, -1)
    used = [s for s, _, _ in d["seqs"]]
    for s in range(NSLOTS):
        if s not in used:
            ck.same_bits(f"state of slot {s}, not in the step", got[s], init[s])
    ck.same_bits("the gaps between state slots", got[:, 3 * C:], init[:, 3 * C:])
    want = st64[used].reshape(len(used), -1)
    ck.close("state (aa, bb, pp)", got[used, :3 * C].view(F32).astype(F64), want, ew_bound(want))
    own = rows_of(d["seqs"])
    assert np.abs(y64[own]).max() > 65504, "the saturating channel does not saturate"
    ck.operand("y", res, "yhi", "ylo" if c.o["ylo"] else None, T, P["ldh"], {t: t for t in own}, C, y64, ew_bound(f16_sat(np.nan_to_num(y64))))


# ------------------------------------------------------------------------------------------------
# row kernels: ln_shift, embed, ln_out
# ------------------------------------------------------------------------------------------------
def ln_eval(x, w, b, ft):
    """Two-pass LayerNorm over the last axis, eps 1e-5."""
    C = ft(x.shape[-1])
    mean = x.sum(-1, keepdims=True) / C
    dd = x - mean
    var = (dd * dd).sum(-1, keepdims=True) / C
    return dd / np.sqrt(var + ft(1e-5)) * w + b


def ragged_meta(T, rng):
    """Rows of up to four slots, interleaved in runs: one slot has a single row, the others many, no slot's rows adjacent to all of its others."""
    slots = list(SEQ_SLOT)
    slot = np.empty(T, np.int32)
    slot[0] = slots[0]
    t, i = 1, 0
    while t < T:
        n = min(T - t, int(rng.integers(1, 4)))
        slot[t:t + n] = slots[1 + i % 3]
        t, i = t + n, i + 1
    prev, last = np.full(T, -1, np.int32), np.full(T, -1, np.int32)
    for s in set(slot.tolist()):
        rows = np.flatnonzero(slot == s)
        prev[rows[1:]] = rows[:-1]
        last[rows[0]] = rows[-1]
    return slot, prev, last


def make_ln_shift(c):
    P, o = c.p, c.o
    rng = np.random.default_rng(seed_of(c))
    T, C, npar, nmix, nslots = P["T"], P["C"], P["np"], P["nmix"], P["nslots"]
    d = {}
    d["x_in"] = (rng.normal(0, 1, (T, C)) + rng.normal(0, 0.5, (T, 1))).astype(F32)       # every row its own values
    if npar:
        Pb = nan32((npar, P["pstride"]))
        Pb[:, :T * C] = rng.normal(0, 0.3, (npar, T * C))
        d["P"] = Pb
    d["lnw"] = rng.uniform(0.5, 1.5, C).astype(F32)
    d["lnb"] = rng.normal(0, 0.1, C).astype(F32)
    if P["dense"]:
        slot, prev, last = np.arange(T, dtype=np.int32), np.full(T, -1, np.int32), np.arange(T, dtype=np.int32)
    else:
        slot, prev, last = ragged_meta(T, rng)
    d["slot"], d["prev"], d["last"] = slot, prev, last
    sx = nan32((nslots, P["sx_slot_stride"]))
    for s in set(slot.tolist()):
        sx[s, :C] = rng.normal(0, 1, C)
    d["sx"] = sx
    for m in range(nmix):
        d[f"mu{m}"] = rng.uniform(0, 1, C).astype(F32)
    bufs = [b_in("x_in", d["x_in"], back=True)] + ([b_in("P", d["P"], back=True)] if npar else []) + [b_in("lnw", d["lnw"]), b_in("lnb", d["lnb"]), b_in("sx", sx, back=True)]
    if not P["dense"]:
        bufs += [b_in("slot", slot), b_in("prev", prev), b_in("last", last)]
    for m in range(nmix):
        bufs += [b_in(f"mu{m}", d[f"mu{m}"]), b_out(f"ohi{m}", ceil16(T) * P["ldh"], 2)]
        if o["olo"][m]:
            bufs.append(b_out(f"olo{m}", ceil16(T) * P["ldh"], 2))
    for nm in ("x_out", "xx", "dx"):
        if o[nm]:
            bufs.append(b_out(nm, T * C, 4))
    d["bufs"] = bufs
    return d


def row_sum_f32(d, T, C, npar):
    """x_in + partials in the kernel's fixed order j = 0 .. np-1, in fp32: the bit-exact reference of x_out."""
    x = d["x_in"].copy()
    for j in range(npar):
        x = x + d["P"][j, :T * C].reshape(T, C)
    return x


def ln_shift_eval(c, d, ft):
    P = c.p
    T, C, npar = P["T"], P["C"], P["np"]
    x = d["x_in"].astype(ft)
    for j in range(npar) if ft is F64 else reversed(range(npar)):      # the fp32 restatement adds the slabs in the other order
        x = x + d["P"][j, :T * C].reshape(T, C).astype(ft)
    xx = ln_eval(x, d["lnw"].astype(ft), d["lnb"].astype(ft), ft)
    slot, prev, last = d["slot"], d["prev"], d["last"]
    pv = np.where((prev >= 0)[:, None], xx[np.maximum(prev, 0)], d["sx"][slot, :C].astype(ft))
    sx_new = {int(slot[t]): xx[last[t]] for t in range(T) if last[t] >= 0}
    dx = pv - xx
    ops = []
    for m in range(P["nmix"]):
        mu = d[f"mu{m}"].astype(ft)
        ops.append(xx * mu + pv * (ft(1.0) - mu) if P["mode"] == 0 else xx + dx * mu)
    return xx, dx, sx_new, ops


def check_ln_shift(c, d, res, ck):
    P, o = c.p, c.o
    T, C, npar = P["T"], P["C"], P["np"]
    xx, dx, sx_new, ops = ln_shift_eval(c, d, F64)
    ck.same_bits("x_in (an input)", res["x_in"], b_in("x_in", d["x_in"]).image)
    if npar:
        ck.same_bits("P (an input)", res["P"], b_in("P", d["P"]).image)
    if o["x_out"]:
        ck.same_bits("x_out against the fp32 sum in the order j = 0 .. np-1", res["x_out"][GUARD:-GUARD].reshape(T, C), bits(row_sum_f32(d, T, C, npar)).reshape(T, C))
    if o["xx"]:
        ck.close("xx_out", res["xx"][GUARD:-GUARD].view(F32).reshape(T, C).astype(F64), xx, ew_bound(xx))
    if o["dx"]:
        ck.close("dx_out", res["dx"][GUARD:-GUARD].view(F32).reshape(T, C).astype(F64), dx, ew_bound(dx))
    got = res["sx"][GUARD:-GUARD].reshape(P["nslots"], -1)
    init = bits(d["sx"]).reshape(P["nslots"], -1)
    used = sorted(sx_new)
    for s in range(P["nslots"]):
        if s not in sx_new:
            ck.same_bits(f"sx of slot {s}, not in the step", got[s], init[s])
    ck.same_bits("the gaps between sx slots", got[:, C:], init[:, C:])
    want = np.stack([sx_new[s] for s in used])
    ck.close("sx after the step", got[used, :C].view(F32).astype(F64), want, ew_bound(want))
    for m in range(P["nmix"]):
        ck.operand(f"mix {m}", res, f"ohi{m}", f"olo{m}" if o["olo"][m] else None, T, P["ldh"], {t: t for t in range(T)}, C, ops[m], ew_bound(ops[m]))


def make_embed(c):
    P = c.p
    rng = np.random.default_rng(seed_of(c))
    T, C, V = P["T"], P["C"], P["V"]
    d = {"emb": (rng.normal(0, 1, (V, C)) + rng.normal(0, 0.5, (V, 1))).astype(np.float16), "lnw": rng.uniform(0.5, 1.5, C).astype(F32),
         "lnb": rng.normal(0, 0.1, C).astype(F32), "token": np.array([-1, 0, V - 1, V + 7, 17][:T], np.int32)}
    d["bufs"] = [b_in("emb", d["emb"]), b_in("lnw", d["lnw"]), b_in("lnb", d["lnb"]), b_in("token", d["token"]), b_out("x_out", T * C, 4)]
    return d


def embed_eval(c, d, ft):
    tok = np.clip(d["token"], 0, c.p["V"] - 1)                      # the kernel clamps; so does the reference
    return ln_eval(d["emb"][tok].astype(ft), d["lnw"].astype(ft), d["lnb"].astype(ft), ft)


def check_embed(c, d, res, ck):
    want = embed_eval(c, d, F64)
    ck.close("x", res["x_out"][GUARD:-GUARD].view(F32).reshape(want.shape).astype(F64), want, ew_bound(want))


def make_ln_out(c):
    P, o = c.p, c.o
    rng = np.random.default_rng(seed_of(c))
    T, C, npar = P["T"], P["C"], P["np"]
    d = {"x_in": (rng.normal(0, 1, (T, C)) + rng.normal(0, 0.5, (T, 1))).astype(F32), "lnw": rng.uniform(0.5, 1.5, C).astype(F32), "lnb": rng.normal(0, 0.1, C).astype(F32)}
    bufs = [b_in("x_in", d["x_in"])]
    if npar:
        Pb = nan32((npar, P["pstride"]))
        Pb[:, :T * C] = rng.normal(0, 0.3, (npar, T * C))
        d["P"] = Pb
        bufs.append(b_in("P", Pb))
    bufs += [b_in("lnw", d["lnw"]), b_in("lnb", d["lnb"])]
    if o["out_rows"] is not None:
        d["out_rows"] = np.array(o["out_rows"], np.int32)
        bufs.append(b_in("out_rows", d["out_rows"]))
    bufs.append(b_out("ohi0", ceil16(P["n_out"]) * P["ldh"], 2))
    if o["olo"]:
        bufs.append(b_out("olo0", ceil16(P["n_out"]) * P["ldh"], 2))
    d["bufs"] = bufs
    return d


def ln_out_eval(c, d, ft):
    P = c.p
    T, C = P["T"], P["C"]
    x = d["x_in"].astype(ft)
    for j in range(P["np"]) if ft is F64 else reversed(range(P["np"])):
        x = x + d["P"][j, :T * C].reshape(T, C).astype(ft)
    rows = d["out_rows"] if "out_rows" in d else np.arange(P["n_out"])
    return ln_eval(x[rows], d["lnw"].astype(ft), d["lnb"].astype(ft), ft)


def check_ln_out(c, d, res, ck):
    P = c.p
    want = ln_out_eval(c, d, F64)
    ck.operand("ln_out", res, "ohi0", "olo0" if c.o["olo"] else None, P["n_out"], P["ldh"], {i: i for i in range(P["n_out"])}, P["C"], want, ew_bound(want))


# ------------------------------------------------------------------------------------------------
# state_pack: a permutation
# ------------------------------------------------------------------------------------------------
def sp_perm(P):
    """Flat index of the internal element behind every slab element the launch touches: (which of sxa / sxf / wkv, index), per slab index."""
    L, C, H, v4, tr, lo = P["L"], P["C"], P["H"], P["v4"], P["transposed"], P["layer_only"]
    N = 3 if v4 else 64
    total = N * C if lo >= 0 else L * (N + 2) * C
    idx = np.arange(total)
    if lo >= 0:
        l, row, ch = np.full(total, lo), 1 + idx // C, idx % C
    else:
        l, row, ch = idx // ((N + 2) * C), idx % ((N + 2) * C) // C, idx % C
    which = np.where(row == 0, 0, np.where(row == N + 1, 1, 2))
    if v4:
        w = (l * 3 + (row - 1)) * C + ch
    else:
        i, h, j = row - 1, ch // 64, ch % 64
        p, q = (j, i) if tr else (i, j)
        w = ((l * H + h) * 64 + p) * 64 + q
    return which, np.where(which == 2, w, l * C + ch)


def make_state_pack(c):
    P = c.p
    rng = np.random.default_rng(seed_of(c))                         # a to_slab = 0 case and its to_slab = 1 twin share the seed: the round trip
    L, C, H, v4, lo = P["L"], P["C"], P["H"], P["v4"], P["layer_only"]
    N = 3 if v4 else 64
    nslab = N * C if lo >= 0 else L * (N + 2) * C
    nw = L * 3 * C if v4 else L * H * 4096
    X = rng.permutation(nslab).astype(F32) + F32(0.25)               # every slab element its own value
    which, src = sp_perm(P)
    internal = [nan32(L * C), nan32(L * C), nan32(nw)]
    for k in range(3):
        internal[k][src[which == k]] = X[which == k]
    d = {"slab": X, "internal": internal}
    if P["to_slab"]:
        d["bufs"] = [b_out("slab", nslab, 4)] + [b_in(nm, a, back=True) for nm, a in zip(("sxa", "sxf", "wkvst"), internal)]
    else:
        d["bufs"] = [b_in("slab", X, back=True)] + [b_out(nm, a.size, 4) for nm, a in zip(("sxa", "sxf", "wkvst"), internal)]
    return d


def check_state_pack(c, d, res, ck):
    # both directions expect the same images: the slab X and the internal arrays holding X's elements at their places, the pattern elsewhere
    ck.same_bits("slab", res["slab"][GUARD:-GUARD], bits(d["slab"]))
    for nm, a in zip(("sxa", "sxf", "wkvst"), d["internal"]):
        ck.same_bits(nm, res[nm][GUARD:-GUARD], bits(a))


MAKE = (make_wkv, make_wkv4, make_ln_shift, make_embed, make_ln_out, make_state_pack)
CHECK = (check_wkv, check_wkv4, check_ln_shift, check_embed, check_ln_out, check_state_pack)


def make(case):
    return MAKE[case.kind](case)


def check_case(case, d, res, line, ratios=None):
    """[] or messages; appends (group, case, worst error / bound) to ratios."""
    ck = Checker(case, ratios)
    if line != plan_line(case):
        ck.msgs.append(f"{case.name}: the probe printed {line}, the table says {plan_line(case)}")
    ck.guards(res)
    CHECK[case.kind](case, d, res, ck)
    if ratios is not None and case.kind != K_STATE_PACK:
        ratios.append((case.group, case.name, ck.worst))
    return ck.msgs


def emulate(case, d, ft=F32):
    """The result buffers a correct launch leaves, computed in `ft` by the plain numpy restatement: what check_case must accept.  (The exact
    state of an exact WKV case comes out of this in fp32 too.)"""
    res = {}
    P, o = case.p, case.o
    for b in d["bufs"]:
        if b.flags & 1:
            res[b.role] = (np.full(b.n + 2 * GUARD, SENT32 if b.esize == 4 else SENT16, np.uint32 if b.esize == 4 else np.uint16) if b.flags & 2 else b.image.copy())
    pay = lambda role: res[role][GUARD:-GUARD]

    def put_opd(hi, lo, T, ld, rows, C, vals):
        T16 = ceil16(T)
        v = np.clip(vals.astype(F32), -65504, 65504)
        h = v.astype(np.float16)
        for role, part in ((hi, h), (lo, (v - h.astype(F32)).astype(np.float16))):
            if role is not None:
                a = unpack_opd(pay(role).copy(), T16, ld)
                a[rows, :C] = part.view(np.uint16)
                pay(role)[:] = pack_opd(a)
    if case.kind in (K_WKV, K_WKV4):
        st, y = (wkv_eval if case.kind == K_WKV else wkv4_eval)(case, d, ft)
        n = st[0].size
        used = [s for s, _, _ in d["seqs"]]
        pay("state").reshape(NSLOTS, -1)[used, :n] = bits(st[used].astype(F32)).reshape(len(used), n)
        own = rows_of(d["seqs"])
        if case.kind == K_WKV and P["version"] == 7 and P["layer"] == 0:
            pay("v_first").reshape(P["T"], P["C"])[own] = bits(d["v"]).reshape(P["T"], P["C"])[own]
        put_opd("yhi", "ylo" if o["ylo"] else None, P["T"], P["ldh"], own, P["C"], y[own])
    elif case.kind == K_LN_SHIFT:
        T, C = P["T"], P["C"]
        xx, dx, sx_new, ops = ln_shift_eval(case, d, ft)
        if o["x_out"]:
            pay("x_out")[:] = bits(row_sum_f32(d, T, C, P["np"]))
        if o["xx"]:
            pay("xx")[:] = bits(xx.astype(F32))
        if o["dx"]:
            pay("dx")[:] = bits(dx.astype(F32))
        for s, v in sx_new.items():
            pay("sx").reshape(P["nslots"], -1)[s, :C] = bits(v.astype(F32))
        for m in range(P["nmix"]):
            put_opd(f"ohi{m}", f"olo{m}" if o["olo"][m] else None, T, P["ldh"], np.arange(T), C, ops[m])
    elif case.kind == K_EMBED:
        pay("x_out")[:] = bits(embed_eval(case, d, ft).astype(F32))
    elif case.kind == K_LN_OUT:
        put_opd("ohi0", "olo0" if o["olo"] else None, P["n_out"], P["ldh"], np.arange(P["n_out"]), P["C"], ln_out_eval(case, d, ft))
    else:
        if P["to_slab"]:
            pay("slab")[:] = bits(d["slab"])
        else:
            for nm, a in zip(("sxa", "sxf", "wkvst"), d["internal"]):
                pay(nm)[:] = bits(a)
    return res


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------
SHORT_LENS = ((1, 2, 7, 8), (8, 8, 8, 8), (3, 5, 6, 1))
LONG_LENS = ((9, 1, 32, 33), (31, 64, 65, 2), (70, 1, 1, 1))


def _wkv(name, ver, lens, exact, i, Dd=64, layer=0, dense=False, unknown=False, seed=None):
    H = (1, 3)[(i // 2 + i) % 2]                                    # i counts cases: exact / general pairs are (odd, even), so neither is tied to one H or to ylo
    C = 64 * H
    if dense:
        seqs, T = [(s, s, 1) for s in range(4)], 5                  # slot i = row i; row 4 and slot 4 belong to no sequence
    else:
        seqs, T = layout(lens, np.random.default_rng(zlib.crc32(repr(lens).encode())))
    mr = max(n for _, _, n in seqs)
    p = dict(version=ver, H=H, C=C, n_seq=len(seqs), dense=int(dense), slot_stride=H * 4096 + 64, Dd=Dd if ver == 6 else 0, layer=layer if ver == 7 else 0,
             ldh=C + (32 if i % 3 == 0 else 0), max_rows=0 if unknown else mr, multi_row=int(mr > 1), T=T, nslots=NSLOTS)
    o = dict(seqs=seqs, exact=exact, ylo=(i // 3) % 2 == 0)
    if seed:
        o["seed"] = seed
    return Case(name, f"wkv{ver}", K_WKV, p, o)


def wkv_cases():
    out, i = [], 0
    for ver in (5, 6, 7):
        for Dd in ((64, 128) if ver == 6 else (64,)):
            tag = f"v{ver}" + (f"_dd{Dd}" if ver == 6 else "")
            for form, table in (("short", SHORT_LENS), ("long", LONG_LENS)):
                for lens in table:
                    for exact in (True, False):
                        i += 1
                        ln = "-".join(map(str, lens))
                        nm = f"{tag}_{form}_{ln}_{'exact' if exact else 'general'}"
                        out.append(_wkv(nm, ver, lens, exact, i, Dd, layer=(0, 2)[(i // 4) % 2]))
                        if lens == (3, 5, 6, 1):                   # its twin with max_rows = 0 ("unknown"): the long form on the same data
                            out.append(_wkv(nm + "_unknown", ver, lens, exact, i, Dd, layer=(0, 2)[(i // 4) % 2], unknown=True, seed=nm))
            for exact in (True, False):
                i += 1
                out.append(_wkv(f"{tag}_dense_{'exact' if exact else 'general'}", ver, None, exact, i, Dd, layer=(0, 2)[i % 2], dense=True))
        if ver == 6:
            for Dd in (32, 96):
                for exact in (True, False):
                    i += 1
                    e = "exact" if exact else "general"
                    out.append(_wkv(f"v6_dd{Dd}_dense_{e}", 6, None, exact, i, Dd, dense=True))
                    out.append(_wkv(f"v6_dd{Dd}_rows_1-9-33-8_{e}", 6, (1, 9, 33, 8), exact, i + 1, Dd))
                    out.append(_wkv(f"v6_dd{Dd}_rows_3-5-6-1_{e}", 6, (3, 5, 6, 1), exact, i, Dd))
    return out


def twins(cases):
    """(short-form case, its max_rows = 0 twin): the same data through CH = 8 and CH = 32."""
    by = {c.name: c for c in cases}
    return [(by[c.o["seed"]], c) for c in cases if c.kind == K_WKV and c.name.endswith("_unknown") and kernel_of(plan_line(c)).startswith("wkv_chunk")]


def wkv4_cases():
    out, i = [], 0
    for C in (64, 320):
        for nm, lens, dense in (("dense", None, True), ("rows_1-2-33-8", (1, 2, 33, 8), False), ("rows_1-1-1-1", (1, 1, 1, 1), False)):
            for ylo in (True, False):
                i += 1
                if dense:
                    seqs, T = [(s, s, 1) for s in range(4)], 5
                else:
                    seqs, T = layout(lens, np.random.default_rng(i))
                mr = max(n for _, _, n in seqs)
                p = dict(C=C, n_seq=len(seqs), dense=int(dense), slot_stride=3 * C + 64, ldh=C + (32 if i % 3 == 0 else 0), multi_row=int(mr > 1), T=T, nslots=NSLOTS)
                out.append(Case(f"v4_c{C}_{nm}_{'hilo' if ylo else 'hi'}", "wkv4", K_WKV4, p, dict(seqs=seqs, ylo=ylo)))
    return out


def ln_shift_cases():
    shapes = [(64, t) for t in (1, 5, 64, 65, 67, 71)] + [(4096, 5), (4096, 71), (4160, 1), (4160, 65), (4160, 67), (8192, 5), (8192, 64), (8192, 71),
                                                            (64, 257), (64, 263), (2048, 257), (2112, 257), (4160, 257)]
    modes = ((0, 4), (1, 1), (1, 2), (1, 6))
    out = []
    for i, (C, T) in enumerate(shapes):
        mode, nmix = modes[i % 4]
        npar = (0, 1, 3, 8)[(i // 2) % 4]
        if C >= 4096 and T >= 64:                                    # the widest launches stay small files
            nmix, npar = min(nmix, 2), min(npar, 3)
            mode = 1 if nmix != 4 else 0
        dense = i % 2 == 0 and T > 1
        nslots = T + 1 if dense else NSLOTS
        p = dict(T=T, C=C, np=npar, pstride=T * C + 96, sx_slot_stride=C + 64, dense=int(dense), mode=mode, nmix=nmix, ldh=C + (64 if i % 3 == 1 else 0), nslots=nslots)
        o = dict(olo=[(m + i) % 2 == 0 for m in range(nmix)], x_out=i % 4 != 3, xx=i % 3 != 2, dx=i % 3 != 1)
        out.append(Case(f"ln_shift_c{C}_t{T}", "ln_shift_512" if T > 256 else "ln_shift_1024", K_LN_SHIFT, p, o))
    return out


def embed_ln_out_cases():
    out = []
    for i, C in enumerate((64, 1088, 2112, 4160, 8192)):
        out.append(Case(f"embed_c{C}", "embed_ln_out", K_EMBED, dict(T=5, C=C, V=48)))
        for j, rows in enumerate((None, (4, 1, 3))):
            npar = (0, 2)[(i + j) % 2]
            p = dict(n_out=5 if rows is None else len(rows), C=C, np=npar, pstride=5 * C + 96, ldh=C + (32 if j else 0), T=5)
            out.append(Case(f"ln_out_c{C}_{'all' if rows is None else 'compacted'}", "embed_ln_out", K_LN_OUT, p, dict(out_rows=rows, olo=(i + j) % 2 == 1)))
    return out


def state_pack_cases():
    out = []
    for v4, tr in ((0, 1), (0, 0), (1, 0)):
        for lo in (-1, 1):
            for ts in (0, 1):
                p = dict(L=2, C=192, H=3, v4=v4, transposed=tr, to_slab=ts, layer_only=lo)
                out.append(Case(f"state_pack_v4{v4}_tr{tr}_layer{lo}_{'to_slab' if ts else 'from_slab'}", "state_pack", K_STATE_PACK, p, dict(seed=f"sp{v4}{tr}{lo}")))
    return out


def all_cases():
    cases = wkv_cases() + wkv4_cases() + ln_shift_cases() + embed_ln_out_cases() + state_pack_cases()
    assert len({c.name for c in cases}) == len(cases)
    assert {c.group for c in cases} == set(GROUPS)
    return cases

"""The top-n probe's case table and reference, shared by tests/test_gpu_topn_exact.py (runs tests/cpp/topn_probe.hip on the GPU),
tests/test_gpu_topn.py (the same rows through the ABI) and tests/test_topn_cases_cpu.py (proves both without a GPU): one launch_topn_rows per
case (DESIGN.md 3.8 "Top-n lists").

Every buffer has a 256-element guard band on both sides and every block a spare row on both sides; every write-only buffer starts as the pattern
0x7FC0DEAD.  What the launch does not own must hold its bits afterwards.

The reference is `topn_ref`: a stable sort on (-x, id) over the entries above -inf, ln-probabilities in float64.  No row is skipped and no margin
caps a comparison: the ids of a list are a function of the row's bits.

`candidates` restates the one data-dependent branch of the kernel — how many entries reach the bound taken from the 256 lane maxima, and so
whether the row takes the exact search — so that the table can PROVE it holds rows on both sides of it (rule: a rare branch needs its own input)."""
import os
import zlib
from dataclasses import dataclass, field

import numpy as np

from tests.probe_io import GUARD, SENT32, b_in, b_out, bits, own, read_results, untouched   # noqa: F401  (the container: stated once, there)
from tests.probe_io import write_cases as write_case_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL = 2e-5                                                    # the project's Fp32 tolerance (tests/test_gpu_score.py derives it)
F32, F64 = np.float32, np.float64
INF = np.inf
TOPN_MAX, TOPN_NONE, TOPN_CAND, THREADS = 32, 0xFFFFFFFF, 1024, 256    # RWKV_TOPN_MAX, RWKV_TOPN_NONE; TOPN_CAND, SCORE_THREADS of the kernel
MAGIC = 0x4E504F54
PARAMS = ("n_rows", "V", "n", "side")
ROLE = {n: i for i, n in enumerate("logits out_ids out_logp side_ms side_rows".split())}   # the Role enum of topn_probe.hip
VOCABS = (16, 272, 65520, 65536)
NS = (1, 5, 20, 32)
GROUPS = tuple(f"V{V}" for V in VOCABS)


@dataclass
class Case:
    name: str
    group: str
    kind: int
    p: dict
    o: dict = field(default_factory=dict)                          # rows: which rows of the vocabulary's table ride in the launch


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def lse64(row):
    """(m, ln S) of a row in float64; S = 0 (ln S = -inf) for a row of nothing but -inf."""
    x = np.asarray(row, F64)
    m = x.max()
    if m == -INF:
        return m, -INF
    with np.errstate(divide="ignore", invalid="ignore"):
        return m, float(np.log(np.exp(x - m).sum()))


def topn_ref(row, n):
    """ids (uint32 [n]) and ln-probabilities (float64 [n]) of the list of `row`."""
    x = np.asarray(row, F32)
    ids, lp = np.full(n, TOPN_NONE, np.uint32), np.full(n, -INF, F64)
    if np.isnan(x).any() or (x == INF).any():
        lp[:] = np.nan
        return ids, lp
    live = np.nonzero(x > -INF)[0]
    xl = x[live].astype(F64) + 0.0                                 # -0 + 0 = +0: the two zeros are one real number
    order = live[np.lexsort((live, -xl))][:n]                      # last key first: -x ascending, then the id ascending
    m, lns = lse64(x)
    ids[:order.size] = order
    lp[:order.size] = (x[order].astype(F64) - m) - lns
    return ids, lp


def candidates(row, n):
    """How many entries the kernel's first gather finds: composites (key, ~id) at or above the n-th largest of the 256 lane maxima, lane of
    id i = (i >> 2) % 256.  More than TOPN_CAND: the row takes the exact search.  (Rows without +inf / NaN.)"""
    x = np.asarray(row, F32)
    V = x.size
    ids = np.arange(V)
    live = x > -INF
    # rank every live entry by (x descending, id ascending): rank 0 is the largest composite
    order = ids[live][np.lexsort((ids[live], -(x[live].astype(F64) + 0.0)))]
    rank = np.full(V, V, np.int64)
    rank[order] = np.arange(order.size)
    lane_best = np.full(THREADS, V, np.int64)
    np.minimum.at(lane_best, (ids >> 2) % THREADS, rank)
    bound = np.sort(lane_best)[n - 1]                              # V: fewer than n live lanes, every live entry is a candidate
    return int(order.size) if bound >= V else int(bound) + 1


# ------------------------------------------------------------------------------------------------
# the rows of a vocabulary
# ------------------------------------------------------------------------------------------------
def tie_ids(V):
    """40 ids (all of a smaller row) of one repeated top value: a whole float4, both sides of a lane, a wave and a block-stride boundary,
    the last float4 of the row."""
    want = [0, 1, 2, 3, 4, 7, 8, 255, 256, 257, 1020, 1023, 1024, 1027, 2048, 4095, 4096, V - 1, V - 2, V - 3, V - 4, V - 5, V - 16, V - 17, V // 2, V // 2 + 1]
    ids = sorted({i for i in want if 0 <= i < V})
    rng = np.random.default_rng(V)
    while len(ids) < min(40, V):
        ids = sorted(set(ids) | {int(rng.integers(V))})
    return ids


_ROWS = {}


def rows_of(V):
    """name -> fp32 row; the table of a vocabulary, made once."""
    if V in _ROWS:
        return _ROWS[V]
    rng = np.random.default_rng(zlib.crc32(f"topn{V}".encode()))
    R = {}
    for e in (3, 6):                                               # dyadic: c on 2^e ids, -inf elsewhere: every listed logp is -e ln 2
        if 2 ** e <= V:
            x = np.full(V, -INF, F32)
            x[rng.choice(V, 2 ** e, replace=False)] = F32(1.5)
            R[f"dyadic{e}"] = x
    for k in range(8):
        R[f"normal{k}"] = (rng.standard_normal(V) * 3).astype(F32)
    R["equal"] = np.full(V, F32(-7.25))
    x = (rng.standard_normal(V) * 3).astype(F32)
    x[tie_ids(V)] = F32(17.5)
    R["tie40"] = x
    x = (rng.standard_normal(V) * 3).astype(F32)
    x[1::2] = -INF
    R["alt_inf"] = x
    x = (rng.standard_normal(V) * 3).astype(F32)
    x[(7 * V) // 11] = F32(1e4)
    R["spike"] = x
    x = -np.abs(rng.standard_normal(V) * 3).astype(F32) - F32(1)   # the largest entries are zeros of both signs: one value, ordered by id
    z = rng.choice(V, min(12, V // 2), replace=False)
    x[z] = np.where(np.arange(z.size) % 2 == 0, F32(-0.0), F32(0.0))
    R["zeros"] = x
    R["ramp"] = (-np.arange(V) * 0.001).astype(F32)
    R["striped"] = (-((np.arange(V) >> 2) % THREADS)).astype(F32)   # lane l owns only the value -l: the bound admits n - 1 lanes' worth of entries
    x = np.full(V, -INF, F32)
    x[rng.choice(V, 3, replace=False)] = rng.standard_normal(3).astype(F32)
    R["three_live"] = x
    R["all_inf"] = np.full(V, -INF, F32)
    x = (rng.standard_normal(V) * 3).astype(F32)
    x[V // 3] = np.nan
    R["nan"] = x
    x = (rng.standard_normal(V) * 3).astype(F32)
    x[V - 1] = INF
    R["pos_inf"] = x
    _ROWS[V] = R
    return R


_REF = {}


def ref_of(V, name, n):
    """The list of a named row, computed once per (V, row) at TOPN_MAX and cut: a list's first n places do not depend on n."""
    key = (V, name)
    if key not in _REF:
        _REF[key] = topn_ref(rows_of(V)[name], TOPN_MAX)
    ids, lp = _REF[key]
    return ids[:n], lp[:n]


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
def all_cases():
    cases = []
    for V in VOCABS:
        names = list(rows_of(V))
        g = f"V{V}"
        for n in NS:
            side = 1 if n in (1, 20) else 0
            cases.append(Case(f"{g}_n{n}_all", g, 0, {"n_rows": len(names), "V": V, "n": n, "side": side}, {"rows": names}))
            cases.append(Case(f"{g}_n{n}_all_side{1 - side}", g, 0, {"n_rows": len(names), "V": V, "n": n, "side": 1 - side}, {"rows": names}) if n in (5, 20) else None)
            five = ["normal0", "tie40", "striped", "equal", "nan"]
            cases.append(Case(f"{g}_n{n}_five", g, 0, {"n_rows": 5, "V": V, "n": n, "side": 0}, {"rows": five}))
            for nm in ("tie40", "striped", "normal0"):
                cases.append(Case(f"{g}_n{n}_one_{nm}", g, 0, {"n_rows": 1, "V": V, "n": n, "side": 0}, {"rows": [nm]}))
    return [c for c in cases if c is not None]


def write_cases(path, cases, datas):
    return write_case_file(path, MAGIC, cases, datas, lambda c: PARAMS, ROLE)


def plan_line(c):
    return {"case": c.name, "launcher": "topn_rows", **{k: int(c.p[k]) for k in PARAMS}}


def build_probe():
    from ai00_server_amd import build as B
    return B.build_probe("topn_probe", verbose=False)


def make(c):
    V, n, nr = c.p["V"], c.p["n"], c.p["n_rows"]
    x = np.stack([rows_of(V)[nm] for nm in c.o["rows"]])
    assert x.shape == (nr, V)
    bufs = [b_in("logits", x, back=True, spare=V), b_out("out_ids", nr * n, spare=n), b_out("out_logp", nr * n, spare=n)]
    if c.p["side"]:
        bufs += [b_out("side_ms", nr * 2, spare=2), b_out("side_rows", nr * V, spare=V)]
    return {"bufs": bufs, "x": x}


def reference_results(c, d):
    """What a correct launch returns (logp rounded from float64): the CPU tests check the checker against this and against mistakes."""
    V, n, nr = c.p["V"], c.p["n"], c.p["n_rows"]
    res = untouched(d)
    bo = {b.role: b for b in d["bufs"]}
    ids = np.stack([ref_of(V, nm, n)[0] for nm in c.o["rows"]])
    lp = np.stack([ref_of(V, nm, n)[1] for nm in c.o["rows"]]).astype(F32)
    for role, a in (("out_ids", ids), ("out_logp", lp)):
        res[role] = res[role].copy()
        own(res, bo[role])[:] = bits(a)
    if c.p["side"]:
        ms = np.array([lse64(r) for r in d["x"]], F64).astype(F32)
        for r, nm in enumerate(c.o["rows"]):                       # a poisoned row: ln S is NaN
            if nm in ("nan", "pos_inf"):
                ms[r, 1] = np.nan
        # consistent with the lists: logp is (x - m) - ln S of the side values in fp32
        for role, a in (("side_ms", ms), ("side_rows", d["x"])):
            res[role] = res[role].copy()
            own(res, bo[role])[:] = bits(a)
        with np.errstate(invalid="ignore"):
            for r in range(nr):
                k = ids[r] != TOPN_NONE
                lp[r, k] = (d["x"][r, ids[r, k]] - ms[r, 0]) - ms[r, 1]
        own(res, bo["out_logp"])[:] = bits(lp)
    return res


def check_case(c, d, res, line, ratios=None):
    """Findings as strings; `ratios` collects (case, what, worst error / bound)."""
    V, n, nr = c.p["V"], c.p["n"], c.p["n_rows"]
    msgs, worst = [], 0.0
    if line != plan_line(c):
        msgs.append(f"{c.name}: the probe ran {line}, the table says {plan_line(c)}")
    bo = {b.role: b for b in d["bufs"]}
    if (res["logits"] != bo["logits"].image).any():
        msgs.append(f"{c.name}: the logits block, a spare row or a guard band of it was written")
    for b in d["bufs"]:
        if b.flags & 2:
            a, e = res[b.role], GUARD + b.off
            if (a[:e] != SENT32).any() or (a[a.size - e:] != SENT32).any():
                msgs.append(f"{c.name}: a guard band or spare row of {b.role} was written")
    ids = own(res, bo["out_ids"]).reshape(nr, n)
    lpb = own(res, bo["out_logp"]).reshape(nr, n)
    lp = lpb.view(F32)
    ids_ok = set()
    for r, nm in enumerate(c.o["rows"]):
        wi, wl = ref_of(V, nm, n)
        if (ids[r] != wi).any():
            k = int(np.nonzero(ids[r] != wi)[0][0])
            msgs.append(f"{c.name}: row {r} ({nm}): ids differ from place {k}: got {ids[r][k:k + 4]}, want {wi[k:k + 4]}")
            continue
        ids_ok.add(r)
        if (lpb[r] == SENT32).any():
            msgs.append(f"{c.name}: row {r} ({nm}): a place of out_logp was not written")
            continue
        if np.isnan(wl).all():
            if not np.isnan(lp[r]).all():
                msgs.append(f"{c.name}: row {r} ({nm}): a poisoned row must list NaN, got {lp[r][:4]}")
            continue
        pad = wi == TOPN_NONE
        if (lp[r][pad] != -INF).any():
            msgs.append(f"{c.name}: row {r} ({nm}): a place without an entry must hold -inf, got {lp[r][pad][:4]}")
        got, want = lp[r][~pad].astype(F64), wl[~pad]
        # dyadic rows: exp and every sum are exact, S = 2^e, so the one rounding is logf's (1 ulp of e ln 2); else the project's fp32 class
        bound = np.abs(want) * 2.0 ** -23 if nm.startswith("dyadic") else FP32_TOL * np.maximum(1.0, np.abs(want))
        err = np.abs(got - want)
        if err.size:
            with np.errstate(invalid="ignore", divide="ignore"):
                q = float(np.max(np.where(np.isnan(err), np.inf, np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0)))))
            worst = max(worst, q)
            if not (err <= bound).all():
                k = int(np.nonzero(~(err <= bound))[0][0])
                msgs.append(f"{c.name}: row {r} ({nm}): logp of place {k}: got {got[k]!r}, want {want[k]!r} (error / bound {q:.3f})")
        if nm == "equal" and V & (V - 1) == 0 and (np.abs(got + np.log2(V) * np.log(2.0)) > np.log2(V) * np.log(2.0) * 2.0 ** -23).any():
            msgs.append(f"{c.name}: row {r}: an all-equal row of {V} entries lists {got[:2]}, not -ln V")
    if c.p["side"]:
        x = d["x"]
        if (own(res, bo["side_rows"]) != bits(x)).any():
            msgs.append(f"{c.name}: the side copy of the rows differs from the rows")
        ms = own(res, bo["side_ms"]).view(F32).reshape(nr, 2)
        for r, nm in enumerate(c.o["rows"]):
            m, lns = lse64(x[r]) if nm not in ("nan", "pos_inf") else (None, np.nan)
            if np.isnan(lns):
                if not np.isnan(ms[r, 1]):
                    msgs.append(f"{c.name}: row {r} ({nm}): ln S of a poisoned row is {ms[r, 1]!r}")
                continue
            if ms[r, 0] != F32(m):
                msgs.append(f"{c.name}: row {r} ({nm}): side m {ms[r, 0]!r}, the row's maximum is {m!r}")
            if lns == -INF:
                if ms[r, 1] != -INF:
                    msgs.append(f"{c.name}: row {r} ({nm}): ln S of a row of -inf is {ms[r, 1]!r}")
                continue
            if not abs(float(ms[r, 1]) - lns) <= FP32_TOL * max(1.0, abs(lns)):
                msgs.append(f"{c.name}: row {r} ({nm}): side ln S {ms[r, 1]!r}, want {lns!r}")
            if r not in ids_ok:
                continue
            k = ids[r] != TOPN_NONE                                # the list is the side values' (x - m) - ln S, in every bit
            with np.errstate(invalid="ignore"):
                re = ((x[r, ids[r, k]] - ms[r, 0]).astype(F32) - ms[r, 1]).astype(F32)
            if (bits(re) != lpb[r][k]).any():
                msgs.append(f"{c.name}: row {r} ({nm}): logp is not (x - m) - ln S of the side outputs bit for bit")
    if ratios is not None:
        ratios.append((c.name, c.name, worst))
    return msgs


def cross_checks(cases, results, datas):
    """A row's list has the same bits however many rows ride in the launch, with or without the side outputs."""
    seen, msgs = {}, []
    for c, res, d in zip(cases, results, datas):
        bo = {b.role: b for b in d["bufs"]}
        n, nr = c.p["n"], c.p["n_rows"]
        ids, lp = own(res, bo["out_ids"]).reshape(nr, n), own(res, bo["out_logp"]).reshape(nr, n)
        for r, nm in enumerate(c.o["rows"]):
            key = (c.p["V"], n, nm)
            got = (ids[r].tobytes(), lp[r].tobytes() if nm not in ("nan", "pos_inf") else b"")
            if key in seen and seen[key][1] != got:
                msgs.append(f"{c.name}: row {nm} differs in bits from the same row in {seen[key][0]}")
            seen.setdefault(key, (c.name, got))
    return msgs

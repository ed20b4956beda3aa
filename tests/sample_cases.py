"""The sampling / vocabulary-row probe's case table, shared by tests/test_gpu_sample_exact.py (runs tests/cpp/sample_probe.hip on the GPU)
and tests/test_sample_cases_cpu.py (proves the table without one): one launch per case, a sampler case launched twice (DESIGN.md "Sampling
and vocabulary-row probe").

Every buffer has a 256-element guard band on both sides, every logits block and the SampleRow array a spare row / entry on both sides, and
every write-only buffer starts as the pattern 0x7FC0DEAD (bytes: 0xAD).  What a launch does not own must hold its bits afterwards.

Sampler rows come in three families, none of which skips a row or caps a margin:

  A  dyadic     logits c on 2^e ids and -inf elsewhere: p = 2^-e in every bit, every sum the kernels form is the reference's fp32 sequential
                sum, so token AND out_prob bits are exact at any depth.  Draws are fp32 numbers taken from the restated CDF itself.
  B  flattened  distinct or level logits, temperature 1000: every kept rank owns about 1 / k of the CDF and `u` is the middle of rank i's
                interval; the half width is asserted >= 64 x the first-order fp32 bound (i + 90) * 2^-24.  out_prob at 2e-5 relative.
  C  calibrated level rows through several windows, Mirostat: the level probabilities' bits come from calibration rows of the same launch
                (`out_prob` of a Nucleus row aimed at the middle of a level), after which the fp32 restatement is exact.

The reference is one function, `emulate` + `draw`: the candidate order (key descending, ties to the lower id), the kept prefix and the draw
of oracle/rwkv_ref.py nucleus_ref / typical_ref / mirostat_ref, stated window by window as the kernels walk it so that the same text can
be run with one mistake at a time (MISTAKES) and can say which branches a row reaches (the coverage proof)."""
import os
import zlib
from dataclasses import dataclass, field

import numpy as np

from tests.probe_io import GUARD, SENT8, SENT32, Buf, b_in, b_out, bits, own, read_results, untouched   # the container: stated once, there
from tests.probe_io import read_cases as read_case_file, write_cases as write_case_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL = 2e-5                                                    # the project's Fp32 tolerance (tests/test_gpu_dims.py)
F32, F64 = np.float32, np.float64
K_NUCLEUS, K_SOFTMAX, K_SCORE, K_ARGMAX, K_ADJUST, K_MASK = range(6)
KIND_NAME = ("nucleus", "softmax", "score_rows", "argmax", "logit_adjust", "logit_mask")
PARAMS = (("n_rows", "V", "any_nucleus_typical", "any_mirostat", "any_wide"), ("n_rows", "V"), ("n_rows", "V"), ("n_rows", "V"),
          ("n_rows", "V", "n"), ("n_rows", "V", "n"))
_ROLES = "logits sp out_tok out_prob out_tok2 out_prob2 out targets scratch_v scratch_i rows toks vals allow".split()
ROLE = {n: i for i, n in enumerate(_ROLES)}                        # the Role enum of sample_probe.hip
GROUPS = ("dyadic_full", "dyadic_sets", "flattened", "calibrated", "routing", "softmax", "score_rows", "argmax", "logit_edit")
NUC, TYP, MIRO, WIDE = 0, 1, 2, 4                                  # SampleRow.kind
NC_NARROW, NC_MAX, NARROW_TOP_K, SEGS = 1024, 8192, 256, 32         # NUC_CAND, NUC_CAND_MAX, the narrow kernel's top_k clamp, ARGMAX_SEG
SCORE_SKIP = 0xFFFFFFFF
U_TOP = float(F32(0.99999994))                                     # the largest fp32 below 1
SP_DTYPE = np.dtype([("top_p", "<f4"), ("top_k", "<i4"), ("temperature", "<f4"), ("uniform", "<f4"), ("kind", "<i4"), ("tau", "<f4")])
MISTAKES = ("window_8191", "retire_lt", "need_k", "draw_lt", "no_find_or_first", "thr_low", "ties_high_id", "id_bound_low", "id_bound_high")
INF = np.inf


@dataclass
class Case:
    name: str
    group: str
    kind: int
    p: dict
    o: dict = field(default_factory=dict)                          # what make() needs beyond the launcher arguments


def seed_of(case):
    return zlib.crc32(case.name.encode())


# ------------------------------------------------------------------------------------------------
# the case file and the result file (tests/cpp/sample_probe.hip)
# ------------------------------------------------------------------------------------------------
def write_cases(path, cases, datas):
    return write_case_file(path, 0x42525053, cases, datas, lambda c: PARAMS[c.kind], ROLE)


def read_cases(path):
    return read_case_file(path, 0x42525053)


def plan_line(c):
    """The JSON line the probe prints for the case."""
    return {"case": c.name, "launcher": KIND_NAME[c.kind], **{k: int(c.p[k]) for k in PARAMS[c.kind]}}


def compile_probe(out_dir):
    from ai00_server_amd import build as B
    return B.compile_probe("sample_probe", os.path.join(str(out_dir), "sample_probe.o"))


def build_probe():
    from ai00_server_amd import build as B
    return B.build_probe("sample_probe", verbose=False)


# ------------------------------------------------------------------------------------------------
# the sampler's reference: candidates in windows, the kept prefix, the draw
# ------------------------------------------------------------------------------------------------
def classes(key, live):
    """Dense ranks of the sort key: 0 for a dead entry, 1 .. m ascending over the distinct keys of the live ones (equal keys: equal rank)."""
    cls = np.zeros(key.size, np.int64)
    if live.any():
        cls[live] = np.unique(key[live], return_inverse=True)[1].reshape(-1) + 1
    return cls


def emulate(P, cls, kind, cut, top_k, tau, wide, exact, mistake=None, trace=None):
    """The ids the sampler keeps, in order: what nucleus_kernel (wide = False) or sample_wide_kernel (wide = True) walk in pass A.
    P: the probabilities by id (fp32 values when `exact`, else float64); cls: `classes` of the sort key.  None: `top_k < 1` (token 0).
    `mistake` (one of MISTAKES) makes the one-line error a kernel could make; `trace` (a dict) receives the branches reached."""
    V = P.size
    ids = np.arange(V)
    ft = F32 if exact else F64
    miro = kind == MIRO
    tr = trace if trace is not None else {}
    if not miro and top_k < 1:
        tr["top_k_0"] = True
        return None
    if miro:
        with np.errstate(divide="ignore"):
            total_k = int(((P > 0) & ~(-np.log2(P.astype(ft)) > ft(tau))).sum()) + 1
    else:
        total_k = top_k
    NC = NC_MAX if (wide or miro) else NC_NARROW
    if not wide:
        total_k = min(total_k, NC if miro else NARROW_TOP_K)
    total_k = min(total_k, V)
    cap = NC - 1 if (mistake == "window_8191" and wide) else NC     # the walked part of a window, one short while `base` still steps by NC
    live = cls.copy()
    kept, cum, base, w = [], ft(0), 0, 0
    tr.update(windows=0, idb_wide=False, idb_narrow=False, need_mixed_later=False)
    while True:
        k = min(NC, total_k - base) if wide else total_k
        nlive = int((live > 0).sum())
        thr = int(np.partition(live, V - k)[V - k]) if nlive >= k else 0
        if mistake == "thr_low" and thr > 0:
            thr -= 1
        n_ge, n_gt = int((live >= max(thr, 1)).sum()), int((live > thr).sum())
        idb = 1 << 40
        if n_ge > (k if wide else NC):
            tr["idb_wide" if wide else "idb_narrow"] = True
            if w > 0 and n_gt > 0:
                tr["need_mixed_later"] = True
            need = k if mistake == "need_k" else k - n_gt
            ties = ids[live == thr]
            at = need - 1 + {"id_bound_low": -1, "id_bound_high": 1}.get(mistake, 0)   # the bound is the id of the need-th tie
            idb = (0 if mistake is None or need < 1 else -1) if at < 0 else (int(ties[at]) if at < ties.size else 1 << 40)
        adm = (live > 0) & ((live > thr) | ((live == thr) & (ids <= idb)))
        a = ids[adm]
        a = a[np.lexsort((-a if mistake == "ties_high_id" else a, -live[a]))]
        wn = min(a.size, cap, k)
        went = a[:wn]
        tr["windows"] = w + 1
        pw = P[went].astype(ft)
        before = np.cumsum(np.concatenate([[cum], pw]), dtype=ft)   # sequential in fp32, as thread 0 forms it
        stop = False
        take = wn
        if not miro:
            over = np.nonzero(before[:wn] > ft(F32(cut)))[0]
            if over.size:
                stop, take = True, int(over[0])
        kept.append(went[:take])
        cum = before[take]
        if stop or wn < k or base + wn >= total_k or not wide:
            tr["end"] = ("cut" if stop else "ran_out" if wn < k else "bound") + ("_w0" if w == 0 else "_beyond")
            tr["last_wn_lt_k"] = wn < k
            break
        ret = adm if mistake != "retire_lt" else (live > 0) & ((live > thr) | ((live == thr) & (ids < idb)))
        live = np.where(ret, 0, live)
        base += NC
        w += 1
    return np.concatenate(kept)                                     # empty only under a mistake that admits nothing (a cut below 0 is not in the table)


def draw(Pk, kind, T, u, exact, mistake=None, trace=None):
    """(index into the kept list, out_prob) of the draw `u` over the kept probabilities `Pk`, sequential sums in the kernels' order."""
    ft = F32 if exact else F64
    Pk = Pk.astype(ft)
    uf = ft(F32(u))
    if kind == MIRO:
        cmp_ = np.cumsum(Pk, dtype=ft)
        total = cmp_[-1]
        x = ft(uf * total)
    else:
        q = np.power(Pk, ft(F32(1.0) / F32(T))).astype(ft)
        total = np.cumsum(q, dtype=ft)[-1]
        cmp_ = np.cumsum((q / total).astype(ft), dtype=ft)
        x = uf
    hit = np.nonzero(x < cmp_ if mistake == "draw_lt" else x <= cmp_)[0]
    pick = int(hit[0]) if hit.size else (Pk.size - 1 if mistake == "no_find_or_first" else 0)
    if trace is not None:
        trace["draw"] = ("found" if hit.size else "first") + ("_later" if (pick >= NC_MAX if hit.size else Pk.size > NC_MAX) else "_early")
    prob = ft(np.log2(total) - np.log2(Pk[pick])) if kind == MIRO else Pk[pick]
    return pick, prob, cmp_, x


def softmax64(x):
    x = x.astype(F64)
    e = np.exp(x - x.max())
    return e / e.sum()


def sort_key(x, kind):
    """The float64 sort key by id, higher first: the logit (Nucleus, Mirostat: p is monotone in it) or -|(-ln p) - H| (Typical)."""
    if kind != TYP:
        return x.astype(F64)
    p = softmax64(x)
    live = p > 0
    y = np.zeros_like(p)
    y[live] = -np.log(p[live])
    return -np.abs(y - (p * y).sum())


class Src:
    """One logits row and what the reference needs of it.  fam A: P is exact (2^-e on the live ids); B: float64 softmax; C: the level
    probabilities' fp32 bits, `cal` — from the device's calibration rows, or, before a launch, numpy's fp32 softmax as a stand-in."""

    def __init__(self, x, fam, levels=None):
        self.x, self.fam, self.levels = np.ascontiguousarray(x, F32), fam, levels
        self.live = self.x > -INF
        self._cls, self._walk = {}, {}
        if fam == "A":
            n = int(self.live.sum())
            assert n & (n - 1) == 0 and np.unique(self.x[self.live]).size == 1
            self.e = n.bit_length() - 1
        if fam == "C":
            xs = np.array([v for v, _ in levels], F32)
            ex = np.exp((xs - xs.max()).astype(F32)).astype(F32)
            cnt = np.array([len(i) for _, i in levels])
            self.cal = (ex / F32((ex.astype(F64) * cnt).sum())).astype(F32)

    exact = property(lambda self: self.fam != "B")

    def P(self, cal=None):
        if self.fam == "A":
            return np.where(self.live, F32(2.0) ** F32(-self.e), F32(0)).astype(F32)
        if self.fam == "B":
            return softmax64(self.x)
        p = np.zeros(self.x.size, F32)
        for (v, ids), pl in zip(self.levels, self.cal if cal is None else cal):
            p[ids] = pl
        return p

    def cls(self, kind):
        k = TYP if kind == TYP else NUC
        if k not in self._cls:
            self._cls[k] = classes(sort_key(self.x, kind), self.live)
        return self._cls[k]

    def walk(self, r, mistake=None, trace=None, cal=None):
        """The kept ids of row spec `r` (cached: rows of a launch differ mostly in `u` alone)."""
        key = (r["kind"], r["cut"], r["top_k"], r["tau"], r["wide"], mistake, None if cal is None else tuple(bits(cal)))
        if key not in self._walk:
            t = {}
            self._walk[key] = (emulate(self.P(cal), self.cls(r["kind"]), r["kind"], r["cut"], r["top_k"], r["tau"], r["wide"], self.exact, mistake, t), t)
        kept, t = self._walk[key]
        if trace is not None:
            trace.update(t)
        return kept


def expect(src, r, mistake=None, trace=None, cal=None):
    """(token, out_prob) of row spec `r` over `src`; out_prob is exact when src.exact."""
    kept = src.walk(r, mistake, trace, cal)
    if kept is None:
        return 0, F32(0)
    if kept.size == 0:                                              # nothing admitted: the wide kernel writes token 0, the narrow ones the id of an empty slot
        return (0 if r["wide"] else -1), F32(0)
    pick, prob, _, _ = draw(src.P(cal)[kept], r["kind"], r["T"], r["u"], src.exact, mistake, trace)
    return int(kept[pick]), prob


def cdf(src, r):
    """(kept ids, the restated CDF, the number the draw compares with it is u itself (Nucleus / Typical) or u * sum (Mirostat))."""
    kept = src.walk(r)
    _, _, c, _ = draw(src.P()[kept], r["kind"], r["T"], 0.5, src.exact)
    return kept, c


def row(src, kind, u, top_k=0, top_p=2.0, T=1.0, tau=0.0, wide=False, role="draw", **extra):
    """A row spec.  `cut` is what the walk compares the cumulative with (top_p, Typical: tau); Mirostat's tau is max_surprise."""
    return dict(src=src, kind=kind, u=float(F32(u)), top_k=int(top_k), top_p=float(top_p), T=float(T), tau=float(tau), wide=bool(wide),
                cut=float(tau if kind == TYP else top_p), role=role, **extra)


def narrow_exact(S, r):
    """Does a narrow kernel serve the row exactly (then it runs plain AND with SAMPLE_WIDE, and the bits must be the same)?"""
    if r["kind"] != MIRO:
        return r["top_k"] <= NARROW_TOP_K
    P = S.P()
    with np.errstate(divide="ignore"):
        return int(((P > 0) & ~(-np.log2(P.astype(F64)) > r["tau"])).sum()) + 1 < NC_MAX


def both(S, rows):
    """Every row wide, and narrow too where a narrow kernel serves it exactly."""
    out = []
    for r in rows:
        out.append({**r, "wide": True})
        if narrow_exact(S[r["src"]], r):
            out.append({**r, "wide": False})
    return out


# ---- family A ------------------------------------------------------------------------------------
def dyadic(V, ids, c=1.5):
    x = np.full(V, -INF, F32)
    x[np.asarray(ids)] = c
    return Src(x, "A")


def at_and_above(S, r0, ranks):
    """Rows drawing exactly c[i] (picks i) and the next float above (picks i + 1, or the first element behind the last), for i in ranks;
    an entry (i, above) of `ranks` asks for that one draw alone.  The CDF is that of the WIDE walk, the sampler's meaning: a row also runs
    narrow only where the narrow kernel's walk is the same (`both`)."""
    assert r0["wide"]
    kept, c = cdf(S[r0["src"]], r0)
    if r0["kind"] == MIRO:
        c = c / c[-1]                                               # the draw compares u * sum: family A's sums are powers of two, the quotient is exact
    pairs = sorted({(i, ab) for x in ranks for i, ab in ([x] if isinstance(x, tuple) else [(x, False), (x, True)]) if 0 <= i < kept.size})
    out = []
    for i, above in pairs:
        u = np.nextafter(c[i], F32(2)) if above else c[i]
        if 0 <= u <= 1:
            out.append({**r0, "u": float(u), "aim": (int(i), above)})
    return out


def aimed_rank(S, r):
    """The rank a row carrying `aim` = (i, above) must pick: i, or i + 1 for the float above c[i], or the first element behind the last."""
    i, above = r["aim"]
    n = int(S[r["src"]].walk(r).size)
    return (i + 1) % n if above else i


def gen_dyadic_full(c):
    """V = 65536 (the FULL instantiations), x = c everywhere (e = 16) or on a random set: the deep windows."""
    o, V = c.o, c.p["V"]
    rng = np.random.default_rng(seed_of(c))
    e = o.get("e", 16)
    S = [dyadic(V, np.sort(rng.choice(V, 1 << e, replace=False)) if e < 16 else np.arange(V))]
    rows, kind, T = [], o["skind"], o.get("T", 1.0)
    cutkw = "tau" if kind == TYP else "top_p"
    if o["what"] == "edges":                                        # top_k = V, no cut: eight windows, draws at every window edge
        r0 = row(0, kind, 0.5, top_k=V, T=T, tau=(2.0 if kind == TYP else 30.0), wide=True)
        k = 1 << e
        rows = at_and_above(S, r0, [0, 1, k - 2, k - 1, 8190, 8191, 8192, 8193, 16383, 16384, 24575, 24576, 32767, 32768, 40960, 49151, 49152, 57343, 57344])
    elif o["what"] == "counts":                                     # top_k reached exactly; find_or_first when the last cumulative stays below u
        for k in o["ks"]:
            r0 = row(0, kind, U_TOP, top_k=k, T=T, tau=2.0, wide=True)
            rows.append(r0)
            rows += at_and_above(S, r0, [k - 1, k // 2])[:3]
    elif o["what"] == "cuts":                                       # the walk stops at the last entry of window 0, the first of window 1, inside window 2
        for n in o["ns"]:
            r0 = row(0, kind, 0.5, top_k=V, T=T, wide=True, **{cutkw: (n - 1) * 2.0 ** -e})
            assert src_kept(S, r0) == n
            rows.append({**r0, "u": U_TOP})
            rows += at_and_above(S, r0, [0, n - 2, n - 1, 8191, 8192])
    elif o["what"] == "miro":                                       # tau = e +- 1/2: every candidate, or one
        for tau in (e + 0.5, e - 0.5):
            r0 = row(0, MIRO, 0.5, tau=tau, wide=True)
            rows += at_and_above(S, r0, [0, 1, 8191, 8192, 16383, 16384, (1 << e) - 2, (1 << e) - 1])
    rows = both(S, rows)
    assert 1 <= len(rows) <= 64, (c.name, len(rows))
    return S, rows


def src_kept(S, r):
    return int(S[r["src"]].walk(r).size)


def id_sets(V, rng):
    """(name, ids, top_ks): the id sets of family A that aim at the element-id arithmetic."""
    top = V - 1
    mid = np.sort(np.concatenate([[0], rng.choice(np.arange(1, 0x3FFF), 98, replace=False), [0x3FFF, 0x4000],
                                  rng.choice(np.arange(0x4001, top - 1), 2048 - 103, replace=False), [top - 1, top]])) if V > 0x4100 else None
    sets = [("random", np.sort(rng.choice(V, 1 << min(12, int(np.log2(V)) - 1), replace=False)), (1, 2, 100, 256)),
            ("one_thread", np.arange(1 << int(np.log2(V // 1024))) * 1024 + 777 if V >= 2048 else np.array([V // 2]), (1, 3, 64, 256)),
            ("one_register", (V // 1024 - 1) * 1024 + np.arange(1024) if V >= 2048 else np.arange(8, 16), (1, 255, 256)),
            ("ends", np.array([0, V - 1]), (1, 2, 256)),
            ("single", np.array([V - 3]), (1, 256))]
    if V > 33000:
        sets.append(("high", np.sort(rng.choice(np.arange(32768, V), 1 << 13, replace=False)), (1, 200, 256)))
    if mid is not None:                                             # the id bound at 0, 0x3FFF, 0x4000 and at the last id but one (the highest id can never be
        sets.append(("bounds", mid, (1, 100, 101, 2047)))           # the bound: it would need every tie, and then no bound is searched)
    return sets


def gen_dyadic_sets(c):
    """Id sets through the narrow kernels and, the same rows flagged SAMPLE_WIDE, through the wide one: all kinds, top_k and 1 / T."""
    V = c.p["V"]
    rng = np.random.default_rng(seed_of(c))
    S, rows = [], []
    for name, ids, ks in id_sets(V, rng):
        if name not in c.o["sets"]:
            continue
        S.append(dyadic(V, ids))
        s, n = len(S) - 1, len(ids)
        e = S[s].e
        temps = (1.0, 0.5) + ((2.0,) if e % 2 == 0 else ())        # 1 / T in {1, 2, 1/2}: p^(1/T) stays a power of two
        for j, k in enumerate(sorted({min(k, V) for k in ks})):    # the engine hands the kernels min(top_k, num_vocab)
            for kind in (NUC, TYP):
                r0 = row(s, kind, 0.5, top_k=k, T=temps[j % len(temps)], tau=2.0, wide=True, set=name)
                m = min(k, n)                                       # the kept count: a draw at the first rank and draws that tell m - 1 kept entries from m
                spots = [(0, False), (m - 2, True), (m - 1, False)] if V >= 20000 else [0, (1, False), (m - 2, True), m - 1]
                rows += at_and_above(S, r0, spots)
        for tau in (e + 0.5, e - 0.5):
            rows += at_and_above(S, row(s, MIRO, 0.5, tau=tau, wide=True, set=name), [0, (n - 1, False)])
    if "top_k" in c.o["sets"]:                                      # top_k in {0, 1, 256, 257, V}
        S.append(dyadic(V, np.sort(rng.choice(V, 1 << min(10, int(np.log2(V)) - 1), replace=False))))
        for kind in (NUC, TYP):
            for k in sorted({min(k, V) for k in (0, 1, 256, 257, V)}):
                rows.append(row(len(S) - 1, kind, 0.75, top_k=k, tau=2.0, set="top_k"))
    rows = both(S, rows)
    assert len(rows) <= (64 if V >= 65520 else 256), (c.name, len(rows))
    return S, rows


# ---- family B ------------------------------------------------------------------------------------
def flat_rows(S, s, kind, k, n_rows, wide, tau=0.0):
    """One row per rank (all of them, or 0, 1, k - 2, k - 1 and a stride between): u is the middle of the rank's interval of the CDF."""
    r0 = row(s, kind, 0.5, top_k=k, T=1000.0, tau=(2.0 if kind == TYP else tau), wide=wide)
    kept, c = cdf(S[s], r0)
    n = kept.size
    ranks = np.arange(n) if n <= n_rows else np.unique(np.concatenate([[0, 1, n - 2, n - 1], np.linspace(2, n - 3, n_rows - 4).astype(int)]))
    lo = np.concatenate([[0.0], c[:-1]]) / c[-1]
    hi = c / c[-1]
    return [{**r0, "u": float(F32((lo[i] + hi[i]) / 2)), "rank": int(i), "half": float((hi[i] - lo[i]) / 2)} for i in ranks]


def level_row(V, rng, counts, gap=0.25, holes=0):
    """Logit levels top down with gaps >= `gap`; counts[l] ids on level l, `holes` ids at -inf, the rest far below on distinct values."""
    perm = rng.permutation(V)
    x = np.full(V, -INF, F32)
    rest = perm[sum(counts) + holes:]
    x[rest] = (-20.0 - np.arange(rest.size) * 1e-3).astype(F32)
    lv, at, levels = 4.0, 0, []
    for n in counts:
        ids = np.sort(perm[at:at + n])
        x[ids] = lv
        levels.append((lv, ids))
        at += n
        lv -= gap + 0.25 * float(rng.integers(0, 3))
    return x, levels


def gen_flattened(c):
    V, o = c.p["V"], c.o
    rng = np.random.default_rng(seed_of(c))
    n_rows = o.get("nr", 64)
    if o["what"] == "distinct":                                     # N(0, 3^2), every key distinct, -inf holes (a masked row)
        x = np.unique((rng.standard_normal(4 * V) * 3).astype(F32))
        x = rng.permutation(x[np.concatenate([[True], np.diff(x) >= 1e-5])])[:V].copy()
        x[rng.choice(V, V // 8, replace=False)] = -INF
        S = [Src(x, "B")]
        k = min(o["k"], int(S[0].live.sum()))
        rows = flat_rows(S, 0, o["skind"], k, n_rows, o["wide"])
        if not o["wide"]:
            rows += [{**r, "wide": True} for r in rows[:: max(1, len(rows) // 16)]]
    else:                                                           # levels: the k-th key inside a tie class
        x, levels = level_row(V, rng, o["counts"], gap=(0.5 if o["skind"] == TYP else 0.25), holes=o.get("holes", 0))
        S = [Src(x, "B", levels)]
        k, tau = o["k"], 0.0
        if o["skind"] == MIRO:                                      # max_surprise between the surprises of levels 0 and 1, or half a bit under level 0's
            s0, s1 = (-np.log2(softmax64(x)[ids[0]]) for _, ids in levels[:2])
            tau = float(F32((s0 + s1) / 2 if o["tau"] == "between" else s0 - 0.5))
        rows = flat_rows(S, 0, o["skind"], k, n_rows, o["wide"], tau=tau)
        if narrow_exact(S[0], rows[0]):                            # the same rows through the other kernel
            rows += [{**r, "wide": not o["wide"]} for r in rows]
    assert len(rows) <= 256
    return S, rows


# ---- family C ------------------------------------------------------------------------------------
def aim_miro(c, total, i):
    """fp32 draws u with fl(u * total) == c[i] (picks i) and the first above it (picks i + 1), searched a few steps around c[i] / total."""
    u = F32(c[i] / total)
    for _ in range(8):
        if F32(u * total) > c[i]:
            u = np.nextafter(u, F32(0))
        elif F32(np.nextafter(u, F32(2)) * total) <= c[i]:
            u = np.nextafter(u, F32(2))
    return [float(u), float(np.nextafter(u, F32(2)))]


def gen_calibrated(c):
    V, o = c.p["V"], c.o
    rng = np.random.default_rng(seed_of(c))
    counts = o["counts"]
    perm = rng.permutation(V)
    x = np.full(V, -INF, F32)
    levels, at = [], 0
    for l, n in enumerate(counts):
        ids = np.sort(perm[at:at + n])
        x[ids] = F32(2.0 - 0.75 * l)
        levels.append((float(2.0 - 0.75 * l), ids))
        at += n
    S = [Src(x, "C", levels)]
    live = sum(counts)
    rows, edge = [], np.cumsum(counts)
    for l in range(len(counts)):                                    # calibration: Nucleus, wide, top_k = V, T = 1000, u in the middle of the level's span
        rows.append(row(0, NUC, (edge[l] - counts[l] / 2) / live, top_k=V, T=1000.0, wide=True, role="cal", level=l))
    p64 = softmax64(x)
    surprise = [-np.log2(p64[ids[0]]) for _, ids in levels]
    for t in o["taus"]:                                             # None: every live entry; l: between the surprises of levels l and l + 1
        tau = 30.0 if t is None else float(F32((surprise[t] + surprise[t + 1]) / 2))
        assert min(abs(tau - s) for s in surprise) >= 0.1
        r0 = row(0, MIRO, 0.5, tau=tau, wide=True)
        kept, cc = cdf(S[0], r0)
        at_ = sorted({i for i in [0, 8190, 8191, 8192, 8193, 16383, 16384, kept.size - 2, kept.size - 1] + [int(e) + d for e in edge for d in (-1, 0)] if 0 <= i < kept.size})
        for i in at_:
            rows += [{**r0, "u": u, "aim": (i, j == 1)} for j, u in enumerate(aim_miro(cc, cc[-1], i)) if u <= 1]
    assert len(rows) <= 64, len(rows)
    return S, rows


# ---- routing -------------------------------------------------------------------------------------
def gen_routing(c):
    V = c.p["V"]
    rng = np.random.default_rng(seed_of(c))
    S = [dyadic(V, np.sort(rng.choice(V, 64, replace=False)))]
    rows = []
    for rep in range(2):
        for kind in (NUC, TYP, MIRO):
            for wide in (False, True):
                rows.append(row(0, kind, 0.3 + 0.4 * rep, top_k=40, tau=(6.5 if kind == MIRO else 2.0), wide=wide))
    return S, rows


GEN = {"dyadic_full": gen_dyadic_full, "dyadic_sets": gen_dyadic_sets, "flattened": gen_flattened, "calibrated": gen_calibrated, "routing": gen_routing}


_GEN = {}


def gen(c):
    """The sources and row specs of a sampler case, generated once (the row count is a launcher argument, so the table needs them too)."""
    if c.name not in _GEN:
        _GEN[c.name] = GEN[c.group](c)
    return _GEN[c.name]


def make_sampler(c):
    S, rows = gen(c)
    V, n = c.p["V"], len(rows)
    assert n == c.p["n_rows"], (c.name, n, c.p["n_rows"])
    x = np.stack([S[r["src"]].x for r in rows])
    sp = np.zeros(n, SP_DTYPE)
    for j, r in enumerate(rows):
        assert 0 <= r["top_k"] <= V and 0.0 <= r["u"] <= 1.0 and r["T"] > 0 and S[r["src"]].live.any(), (c.name, j)   # what the probe refuses
        sp[j] = (r["top_p"], r["top_k"], r["T"], r["u"], r["kind"] | (WIDE if r["wide"] else 0), r["tau"])
    bufs = [b_in("logits", x, back=True, spare=V), b_in("sp", sp.view(np.uint32), back=True, spare=6), b_out("out_tok", n), b_out("out_tok2", n)]
    if c.o.get("prob", True):
        bufs += [b_out("out_prob", n), b_out("out_prob2", n)]
    return {"bufs": bufs, "S": S, "rows": rows}


def served(c, r):
    """Is the row's kernel launched under the case's flags?"""
    return bool(c.p["any_wide"] if r["wide"] else c.p["any_mirostat"] if r["kind"] == MIRO else c.p["any_nucleus_typical"])


def kernel_of_row(c, r):
    full = "FULL" if c.p["V"] == 65536 else "part"
    return ("sample_wide" if r["wide"] else "nucleus<8192,miro>" if r["kind"] == MIRO else "nucleus<1024>") + "," + full


def calibration(c, d, res, ck=None):
    """Family C: the level probabilities' bits from the calibration rows' out_prob (None elsewhere); they must meet float64 at 2e-5 relative."""
    if c.group != "calibrated":
        return None
    S = d["S"][0]
    bo = {b.role: b for b in d["bufs"]}
    tok, prob = own(res, bo["out_tok"]).view(np.int32), own(res, bo["out_prob"]).view(F32)
    p64 = softmax64(S.x)
    cal = S.cal.copy()
    for j, r in enumerate(d["rows"]):
        if r["role"] == "cal":
            ids = S.levels[r["level"]][1]
            want = p64[ids[0]]
            if ck is not None:
                if tok[j] not in ids:
                    ck.msgs.append(f"{c.name}: calibration row {j}: token {tok[j]} is not on level {r['level']}")
                ck.close(f"calibration row {j} (level {r['level']})", np.array([F64(prob[j])]), np.array([want]), np.array([FP32_TOL * want]))
            cal[r["level"]] = prob[j]
    return cal


def check_sampler(c, d, res, ck):
    bo = {b.role: b for b in d["bufs"]}
    n = len(d["rows"])
    ck.same_bits("logits (the block, its spare rows and guard bands)", res["logits"], bo["logits"].image)
    ck.same_bits("SampleRow array", res["sp"], bo["sp"].image)
    tok, tok2 = own(res, bo["out_tok"]), own(res, bo["out_tok2"])
    has_prob = "out_prob" in bo
    prob, prob2 = (own(res, bo["out_prob"]), own(res, bo["out_prob2"])) if has_prob else (None, None)
    ck.same_bits("out_tok of the second launch", tok2, tok)
    if has_prob:
        ck.same_bits("out_prob of the second launch", prob2, prob)
    cal = calibration(c, d, res, ck)
    twins = {}
    for j, r in enumerate(d["rows"]):
        S = d["S"][r["src"]]
        if not served(c, r):                                        # no kernel of the launch owns the row: the pattern stays
            if tok[j] != SENT32 or (has_prob and prob[j] != SENT32):
                ck.msgs.append(f"{c.name}: row {j} was written although its kind's flag is off")
            continue
        if r["role"] == "cal":
            continue
        wt, wp = expect(S, r, cal=cal)
        gt = int(tok.view(np.int32)[j])
        if gt != wt:
            ck.msgs.append(f"{c.name}: row {j} ({kernel_of_row(c, r)}, kind {r['kind']}, top_k {r['top_k']}, cut {r['cut']}, T {r['T']}, tau {r['tau']}, u {r['u']!r}, "
                           f"{r.get('aim', r.get('rank', ''))}): token {gt}, want {wt}")
        if has_prob:
            gp = prob.view(F32)[j]
            if S.fam == "A":
                if bits(np.array([gp], F32))[0] != bits(np.array([wp], F32))[0]:
                    ck.msgs.append(f"{c.name}: row {j} ({kernel_of_row(c, r)}, kind {r['kind']}, T {r['T']}): out_prob {gp!r}, want {wp!r} in every bit")
            elif r["kind"] == MIRO:
                ck.close(f"row {j} surprise", np.array([F64(gp)]), np.array([F64(wp)]), np.array([FP32_TOL * max(1.0, abs(float(wp)))]))
            else:
                ck.close(f"row {j} out_prob", np.array([F64(gp)]), np.array([F64(wp)]), np.array([FP32_TOL * float(wp)]))
        key = (r["src"], r["kind"], r["top_k"], r["cut"], r["T"], r["tau"], r["u"])
        mine = (int(tok[j]), int(prob[j]) if has_prob else 0)
        if narrow_exact(S, r) and twins.setdefault(key, mine) != mine:   # the bit rule: the narrow kernel's bits from the wide one
            ck.msgs.append(f"{c.name}: row {j}: narrow and wide differ on the same row: {twins[key]} against {mine}")


# ------------------------------------------------------------------------------------------------
# comparing with the reference
# ------------------------------------------------------------------------------------------------
class Checker:
    def __init__(self, case):
        self.c, self.msgs, self.worst = case, [], 0.0

    def same_bits(self, what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        bad = got != want
        if bad.any():
            i = np.nonzero(bad)[0][:3]
            self.msgs.append(f"{self.c.name}: {what}: {int(bad.sum())} of {bad.size} elements differ: " + " ".join(f"([{k}]: got {got[k]:#x}, want {want[k]:#x})" for k in i))

    def close(self, what, got, want, bound):
        err = np.abs(got - want)
        bad = ~(err <= bound)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = float(np.max(np.where(np.isnan(err), np.inf, np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))))) if err.size else 0.0
        self.worst = max(self.worst, r)
        if bad.any():
            i = np.nonzero(bad.reshape(-1))[0][:3]
            self.msgs.append(f"{self.c.name}: {what} (worst error / bound {r:.3f}): {int(bad.sum())} of {bad.size} differ: "
                             + " ".join(f"([{k}]: got {got.reshape(-1)[k]!r}, want {want.reshape(-1)[k]!r})" for k in i))

    def guards(self, d, res):
        for b in d["bufs"]:
            if b.flags & 1:
                a = res[b.role]
                s = SENT32 if a.dtype == np.uint32 else SENT8
                e = GUARD + b.off
                if (a[:e] != s).any() or (a[a.size - e:] != s).any():
                    self.msgs.append(f"{self.c.name}: a guard band or spare row of {b.role} was written")


# ------------------------------------------------------------------------------------------------
# softmax
# ------------------------------------------------------------------------------------------------
def softmax_bound(V):
    """Relative: the addition chain of the sum of exp (V / 256 per thread, the wave and block sums) in units of 2^-24, times a margin of 4."""
    return 4 * (V / 256 + 16) * 2.0 ** -24


def make_softmax(c):
    V, n = c.p["V"], c.p["n_rows"]
    rng = np.random.default_rng(seed_of(c))
    # the kernel rounds x - m to fp32 before the exp: a relative |x - m| * 2^-25 on the result, which the chain bound does not count.  Rows
    # stay within a range of 16 (8 of the bound's 16 + V / 256 units of 2^-24); the row of a shifted range holds large logits of both signs
    x = np.clip(rng.standard_normal((n, V)) * 3, -8, 8).astype(F32)
    x[0, rng.choice(V, V // 4, replace=False)] = -INF               # masked entries: exactly 0
    if n > 1:
        x[1] = F32(-7.25)                                           # all equal: exactly 1 / V when V is a power of two
        x[2] = x[2] * F32(0.5) + np.where(np.arange(V) % 2 == 0, F32(300.0), F32(296.0)).astype(F32)
        x[3, : V // 2] = -INF
    if c.o.get("equal"):
        x[0] = F32(3.5)
    return {"bufs": [b_in("logits", x, back=True, spare=V), b_out("out", n * V, spare=V)], "x": x}


def softmax_f32(x):
    """The kernel's order in fp32: per thread a sequential sum over i = t, t + 256, ..; a butterfly over the wave; the four waves in order."""
    V = x.size
    m = x.max()
    e = np.exp((x - m).astype(F32)).astype(F32)
    pad = np.zeros((-V) % 256, F32)
    s = np.cumsum(np.concatenate([e, pad]).reshape(-1, 256), axis=0, dtype=F32)[-1]
    s = s.reshape(4, 64)
    for k in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, np.arange(64) ^ k]).astype(F32)
    tot = F32(F32(F32(s[0, 0] + s[1, 0]) + s[2, 0]) + s[3, 0])
    return (e * (F32(1) / tot)).astype(F32)


def check_softmax(c, d, res, ck, got=None):
    V, n = c.p["V"], c.p["n_rows"]
    bo = {b.role: b for b in d["bufs"]}
    if got is None:
        ck.same_bits("logits", res["logits"], bo["logits"].image)
        got = own(res, bo["out"]).view(F32).reshape(n, V)
    x = d["x"]
    for r in range(n):
        want = softmax64(x[r])
        ck.close(f"row {r}", got[r].astype(F64), want, softmax_bound(V) * want)
        if ((got[r] != 0) & (x[r] == -INF)).any():
            ck.msgs.append(f"{c.name}: row {r}: a -inf entry is not exactly 0")
        if np.unique(x[r]).size == 1 and V & (V - 1) == 0 and (got[r] != F32(1.0 / V)).any():
            ck.msgs.append(f"{c.name}: row {r}: an all-equal row of {V} entries is not exactly 1 / V")


# ------------------------------------------------------------------------------------------------
# score_rows
# ------------------------------------------------------------------------------------------------
def score_targets(V):
    return sorted({t for t in (0, 3, 4, 1023, 1024, 4095, 4096, V - 1) if t < V})


def make_score(c):
    V, n = c.p["V"], c.p["n_rows"]
    rng = np.random.default_rng(zlib.crc32(c.o["seed"].encode()))
    tg = score_targets(V)
    nfull = len(tg) + 4
    x = (rng.standard_normal((nfull, V)) * 3).astype(F32)
    tgt = np.array(tg + [V // 2, SCORE_SKIP, 5 % V, V - 1], np.uint32)
    x[len(tg), V // 2] = -INF                                        # a masked target between scored rows
    x[len(tg), rng.choice(V, V // 3, replace=False)] = -INF
    x[len(tg) + 2] = -INF                                            # dyadic rows: -e ln 2
    x[len(tg) + 2, rng.choice(np.arange(1, V), min(V // 2, 256) - 1, replace=False)] = 0.5
    x[len(tg) + 2, 5 % V] = 0.5
    x[len(tg) + 3] = F32(-2.0)
    want = np.zeros(nfull, F64)
    for r in range(nfull):
        if tgt[r] == SCORE_SKIP:
            want[r] = np.nan
        else:
            with np.errstate(divide="ignore"):
                want[r] = np.log(softmax64(x[r])[tgt[r]])
    want[len(tg) + 2] = -np.log2(min(V // 2, 256)) * np.log(2.0)
    want[len(tg) + 3] = -np.log2(V) * np.log(2.0) if V & (V - 1) == 0 else want[len(tg) + 3]
    lo = c.o.get("row", 0)
    sel = slice(lo, lo + n)
    assert lo + n <= nfull
    return {"bufs": [b_in("logits", x[sel], back=True, spare=V), b_in("targets", tgt[sel]), b_out("out", n)], "x": x[sel], "tgt": tgt[sel], "want": want[sel]}


def check_score(c, d, res, ck, got=None):
    bo = {b.role: b for b in d["bufs"]}
    if got is None:
        ck.same_bits("logits", res["logits"], bo["logits"].image)
        got = own(res, bo["out"]).view(F32)
    want = d["want"]
    for r in range(c.p["n_rows"]):
        if d["tgt"][r] == SCORE_SKIP:
            if not np.isnan(got[r]) or bits(got[r:r + 1])[0] == SENT32:
                ck.msgs.append(f"{c.name}: row {r}: a skipped row must be written as NaN, got {got[r]!r} ({bits(got[r:r + 1])[0]:#x})")
        elif want[r] == -INF:
            if got[r] != -INF:
                ck.msgs.append(f"{c.name}: row {r}: a -inf target gives {got[r]!r}")
        else:
            ck.close(f"row {r}", got[r:r + 1].astype(F64), want[r:r + 1], FP32_TOL * np.maximum(1.0, np.abs(want[r:r + 1])))


# ------------------------------------------------------------------------------------------------
# argmax
# ------------------------------------------------------------------------------------------------
def make_argmax(c):
    V = c.p["V"]
    rng = np.random.default_rng(seed_of(c))
    per = -(-V // SEGS)
    rows = []

    def base():
        return (rng.standard_normal(V) * 2).astype(F32) - F32(20)

    spots = sorted({i for s in range(1, SEGS) for i in (per * s - 1, per * s) if 0 < i < V} | {0, V - 1})
    if c.o["what"] == "spots":                                      # the maximum at 0, V - 1 and on both sides of every segment boundary
        for i in spots:
            x = base()
            x[i] = 5.0
            rows.append(x)
    else:
        x = base(); x[[V - 1, V // 2, 3 % V]] = 5.0; rows.append(x)                         # ties across segments: the lowest id
        x = base(); x[[min(V - 1, 300), min(V - 1, 70), min(V - 1, 65)]] = 5.0; rows.append(x)   # across waves and threads
        x = base(); x[[min(V - 1, 256 + 9), 9]] = 5.0; rows.append(x)                       # two trips of one thread
        x = np.full(V, -INF, F32); rows.append(x)                                          # nothing above -inf: token 0
        x = np.full(V, -INF, F32); x[V - 1] = -3.0e38; rows.append(x)
        x = np.full(V, -0.0, F32); x[V // 3] = 0.0; rows.append(x)                          # -0.0 == +0.0: id 0
        x = np.full(V, -1.0, F32); x[per:] = -0.0; x[V - 2] = 0.0; rows.append(x)
        x = np.full(V, 7.0, F32); rows.append(x)
    x = np.stack(rows)
    n = len(rows)
    assert n == c.p["n_rows"], (c.name, n)
    return {"bufs": [b_in("logits", x, back=True, spare=V), b_out("out", n), b_out("scratch_v", n * SEGS), b_out("scratch_i", n * SEGS)], "x": x}


def argmax_ref(x):
    """(token, stage 1's per-segment value and index) per row: np.argmax (the first maximum; -0.0 == +0.0), 0 for a row of nothing but -inf."""
    n, V = x.shape
    per = -(-V // SEGS)
    pv, pi = np.full((n, SEGS), -INF, F32), np.full((n, SEGS), 0x7fffffff, np.int32)
    for s in range(SEGS):
        lo, hi = s * per, min(V, s * per + per)
        if lo < hi:
            a = np.argmax(x[:, lo:hi], axis=1)
            v = x[np.arange(n), lo + a]
            pv[:, s] = v
            pi[:, s] = np.where(v > -INF, lo + a, 0x7fffffff)
    return np.argmax(x, axis=1).astype(np.int32), pv, pi


def check_argmax(c, d, res, ck, got=None):
    bo = {b.role: b for b in d["bufs"]}
    n = c.p["n_rows"]
    tok, pv, pi = argmax_ref(d["x"])
    if got is None:
        ck.same_bits("logits", res["logits"], bo["logits"].image)
        got = own(res, bo["out"])
        ck.same_bits("stage 1 indices", own(res, bo["scratch_i"]), bits(pi))
        sv = own(res, bo["scratch_v"]).view(F32).reshape(n, SEGS)
        if not (sv == pv).all():                                    # by value: the maximum of a segment of zeros may be either zero
            ck.msgs.append(f"{c.name}: stage 1 values differ in {int((sv != pv).sum())} segments")
    ck.same_bits("token", np.asarray(got).view(np.uint32), bits(tok))


# ------------------------------------------------------------------------------------------------
# logit_adjust / logit_mask
# ------------------------------------------------------------------------------------------------
def make_adjust(c):
    V, n, nr = c.p["V"], c.p["n"], c.p["n_rows"]
    rng = np.random.default_rng(seed_of(c))
    x = (rng.integers(-64, 65, (nr, V)) / 4.0).astype(F32)
    x[0, 1] = -INF
    flat = rng.choice(nr * V, n, replace=False)                     # the host merges duplicates: every (row, token) once
    rows, toks = (flat // V).astype(np.int32), (flat % V).astype(np.int32)
    toks[7::7] = -1                                                 # ignored
    toks[3::11] = V
    if n > 2:
        rows[1], toks[1] = 0, 1                                     # -inf + v stays -inf
        rows[2], toks[2] = nr - 1, V - 1
    vals = (rng.integers(-32, 33, n) / 4.0).astype(F32)
    want = x.copy()
    ok = (toks >= 0) & (toks < V)
    assert np.unique(rows[ok].astype(np.int64) * V + toks[ok]).size == ok.sum()
    want[rows[ok], toks[ok]] += vals[ok]
    return {"bufs": [b_in("logits", x, back=True, spare=V), b_in("rows", rows), b_in("toks", toks), b_in("vals", vals)], "want": want, "ok": int(ok.sum())}


def make_mask(c):
    V, n, nr = c.p["V"], c.p["n"], c.p["n_rows"]
    rng = np.random.default_rng(seed_of(c))
    x = (rng.standard_normal((nr, V)) * 3).astype(F32)
    x[:, 7] = -0.0
    rows = rng.permutation(nr)[:n].astype(np.int32)                 # neither sorted nor dense
    if n > 1 and (np.diff(rows) > 0).all():
        rows = rows[::-1].copy()
    allow = rng.choice(np.array([0, 0, 1, 0x80, 0xFF], np.uint8), (n, V))
    pat = np.array([[(w >> b) & 1 for b in range(4)] for w in range(16)], np.uint8).reshape(-1)   # every zero / non-zero pattern of a 4-byte word
    for j in range(n):
        wd = min(64, V)
        at = 0 if V <= 64 else 4 * int(rng.integers(0, (V - 64) // 4))
        allow[j, at:at + wd] = np.roll(pat * np.array([1, 0xFF, 0x80, 2], np.uint8)[(np.arange(64) + j) % 4], -16 * j)[:wd]
    want = x.copy()
    for j in range(n):
        want[rows[j], allow[j] == 0] = -INF
    return {"bufs": [b_in("logits", x, back=True, spare=V), b_in("rows", rows), b_in("allow", allow)], "want": want, "rows": rows}


def check_edit(c, d, res, ck, got=None):
    bo = {b.role: b for b in d["bufs"]}
    if got is None:
        got = own(res, bo["logits"])
    ck.same_bits("logits after the launch (touched elements exact, all others their own bits)", got, bits(d["want"]))


MAKE = (make_sampler, make_softmax, make_score, make_argmax, make_adjust, make_mask)
CHECK = (check_sampler, check_softmax, check_score, check_argmax, check_edit, check_edit)


def make(case):
    return MAKE[case.kind](case)


def check_case(case, d, res, line, ratios=None):
    """The findings of one case (an empty list: it passed); appends (group, case, worst error / bound) to `ratios`."""
    ck = Checker(case)
    if line != plan_line(case):
        ck.msgs.append(f"{case.name}: the probe repeated {line}, the table says {plan_line(case)}")
    ck.guards(d, res)
    CHECK[case.kind](case, d, res, ck)
    if ratios is not None and case.kind in (K_NUCLEUS, K_SOFTMAX, K_SCORE):
        ratios.append((case.group, case.name, ck.worst))
    return ck.msgs


def cross_checks(cases, results, datas):
    """Findings that need two cases: score_rows gives a row the same bits whether its launch carries one row, five or all of them."""
    by = {c.name: (c, d, r) for c, d, r in zip(cases, datas, results)}
    msgs = []
    for c, d, r in zip(cases, datas, results):
        t = c.o.get("twin")
        if c.kind == K_SCORE and t:
            ct, dt, rt = by[t]
            lo, n = c.o["row"], c.p["n_rows"]
            a, b = own(r, d["bufs"][2]), own(rt, dt["bufs"][2])[lo:lo + n]
            if (a != b).any():
                msgs.append(f"{c.name}: rows {lo} .. {lo + n - 1} differ from the same rows in {t}: {a} against {b}")
    return msgs


def reference_results(c, d, mistake=None):
    """What the probe would return from kernels that compute the reference (with `mistake`: the sampler's reference making that mistake):
    the CPU test feeds this to the GPU module's checks.  Float64 values are rounded to fp32; family C's bits are numpy's stand-ins."""
    res = untouched(d)
    for b in d["bufs"]:
        res.setdefault(b.role, None)
    bo = {b.role: b for b in d["bufs"]}
    if c.kind == K_NUCLEUS:
        for j, r in enumerate(d["rows"]):
            if not served(c, r):
                continue
            S = d["S"][r["src"]]
            if r["role"] == "cal":
                tok, prob = int(S.levels[r["level"]][1][0]), S.cal[r["level"]]
            else:
                tok, prob = expect(S, r, mistake)
            for suffix in ("", "2"):
                own(res, bo["out_tok" + suffix])[j] = np.uint32(int(tok) & 0xFFFFFFFF)
                if "out_prob" in bo:
                    own(res, bo["out_prob" + suffix])[j] = bits(np.array([prob], F32))[0]
    elif c.kind == K_SOFTMAX:
        own(res, bo["out"])[:] = bits(np.stack([softmax_f32(x) for x in d["x"]]))
    elif c.kind == K_SCORE:
        with np.errstate(invalid="ignore"):
            own(res, bo["out"])[:] = bits(d["want"].astype(F32))
    elif c.kind == K_ARGMAX:
        tok, pv, pi = argmax_ref(d["x"])
        own(res, bo["out"])[:] = bits(tok)
        own(res, bo["scratch_v"])[:] = bits(pv)
        own(res, bo["scratch_i"])[:] = bits(pi)
    else:
        own(res, bo["logits"])[:] = bits(d["want"])
    return {k: v for k, v in res.items() if v is not None}


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------
def _s(name, group, V, n_rows, flags=(1, 1, 1), **o):
    return Case(name, group, K_NUCLEUS, dict(n_rows=n_rows, V=V, any_nucleus_typical=flags[0], any_mirostat=flags[1], any_wide=flags[2]), o)


def sampler_cases():
    out = []
    full = 65536
    # the row counts are what the generators give; make_sampler asserts them (they are part of the launcher's arguments, hence of the table)
    for kind, nm in ((NUC, "nucleus"), (TYP, "typical")):
        out.append(_s(f"A_full_{nm}_edges", "dyadic_full", full, 0, skind=kind, what="edges"))
        out.append(_s(f"A_full_{nm}_counts_a", "dyadic_full", full, 0, skind=kind, what="counts", ks=(100, 1000, 8191, 8192, 8193, 12000, 16384)))
        out.append(_s(f"A_full_{nm}_counts_b", "dyadic_full", full, 0, skind=kind, what="counts", ks=(20000, 30000, 40000, 45000, 50000, 60000, full), T=(2.0 if kind == NUC else 0.5)))
        out.append(_s(f"A_full_{nm}_cuts", "dyadic_full", full, 0, skind=kind, what="cuts", ns=(3000, 8192, 8193, 20000), prob=(kind == NUC)))
        out.append(_s(f"A_full_{nm}_runs_out", "dyadic_full", full, 0, skind=kind, what="counts", e=13, ks=(8192, 8193, full)))
    out.append(_s("A_full_nucleus_runs_out_16384", "dyadic_full", full, 0, skind=NUC, what="counts", e=14, ks=(16383, 16384, 20000)))
    out.append(_s("A_full_mirostat", "dyadic_full", full, 0, skind=MIRO, what="miro"))
    out.append(_s("A_full_mirostat_e14", "dyadic_full", full, 0, skind=MIRO, what="miro", e=14))
    out.append(_s("A_full_mirostat_e12", "dyadic_full", full, 0, skind=MIRO, what="miro", e=12))
    for V, sets in ((full, ("random",)), (full, ("one_thread",)), (full, ("one_register",)), (full, ("ends", "single")), (full, ("high",)), (full, ("bounds",)),
                    (full, ("top_k",)), (65520, ("random",)), (65520, ("high",)), (65520, ("bounds",)), (20000, ("random", "one_thread", "one_register", "bounds")),
                    (4112, ("random", "ends", "single", "top_k")), (16, ("random", "one_thread", "one_register", "ends", "top_k"))):
        out.append(_s(f"A_sets_V{V}_{'_'.join(sets)}", "dyadic_sets", V, 0, sets=sets))
    # family B
    for V, o in ((16, dict(k=12, wide=False)), (512, dict(k=200, wide=False, nr=200)), (1040, dict(k=256, wide=False, nr=200)),
                 (4112, dict(k=300, wide=True, nr=256)), (8208, dict(k=300, wide=True, nr=128)), (20000, dict(k=300, wide=True, nr=64)),
                 (65520, dict(k=256, wide=False, nr=48)), (65520, dict(k=300, wide=True, nr=64)), (65536, dict(k=300, wide=True, nr=64)),
                 (65536, dict(k=256, wide=False, nr=48))):
        out.append(_s(f"B_distinct_V{V}_{'wide' if o['wide'] else 'narrow'}", "flattened", V, 0, skind=NUC, what="distinct", **o))
    # level rows: (counts, k): n_ge <= k; k < n_ge <= 1024; n_ge > 1024; with n_gt = 0 and n_gt > 0
    lv = (("ge_le_k_gt0", (30, 50, 400), 80), ("ge_le_k_gt_none", (60, 400), 60), ("ge_1024_gt0", (30, 500, 400), 120), ("ge_1024_gt_none", (700, 400), 100),
          ("ge_over_gt0", (40, 3000, 400), 150), ("ge_over_gt_none", (5000, 400), 200))
    for V in (8208, 65536):
        for nm, counts, k in lv:
            out.append(_s(f"B_levels_V{V}_{nm}", "flattened", V, 0, skind=NUC, what="levels", counts=counts, k=k, wide=True, nr=(24 if V == 65536 else 64), holes=V // 16))
    out.append(_s("B_levels_V20000_typical", "flattened", 20000, 0, skind=TYP, what="levels", counts=(40, 300, 2000), k=150, wide=True, nr=64, holes=100))
    # Mirostat, level rows: the k-th key (the first entry beyond max_surprise) in a tie class of more than 8192, with n_gt > 0; and n_gt = 0
    out.append(_s("B_levels_V20000_mirostat_gt0", "flattened", 20000, 0, skind=MIRO, what="levels", counts=(50, 12000), k=0, tau="between", wide=False, nr=51))
    out.append(_s("B_levels_V65536_mirostat_gt0", "flattened", 65536, 0, skind=MIRO, what="levels", counts=(20, 30000), k=0, tau="between", wide=True, nr=21))
    out.append(_s("B_levels_V65520_mirostat_gt_none", "flattened", 65520, 0, skind=MIRO, what="levels", counts=(9000, 100), k=0, tau="below", wide=False, nr=1))
    # family C
    out.append(_s("C_V65536_three_levels", "calibrated", 65536, 0, counts=(5000, 9000, 20000), taus=(None,)))
    out.append(_s("C_V40000_three_levels_cut", "calibrated", 40000, 0, counts=(5000, 9000, 20000), taus=(1,)))
    out.append(_s("C_V40000_two_levels", "calibrated", 40000, 0, counts=(9000, 20000), taus=(None,)))
    # routing: all eight flag combinations over two rows of each of the six kinds of row
    for f in range(8):
        fl = (f & 1, f >> 1 & 1, f >> 2 & 1)
        out.append(_s(f"routing_flags_{fl[0]}{fl[1]}{fl[2]}", "routing", 1040, 12, flags=fl, prob=(f != 5)))
    for c in out:                                                   # the row count of a generated case: a launcher argument, fixed here once
        if c.p["n_rows"] == 0:
            c.p["n_rows"] = len(gen(c)[1])
    return out


def utility_cases():
    out = []
    for V in (16, 272, 8208, 65520, 65536):
        for n in (1, 5):
            out.append(Case(f"softmax_V{V}_n{n}", "softmax", K_SOFTMAX, dict(n_rows=n, V=V), {}))
    out.append(Case("softmax_V16_equal", "softmax", K_SOFTMAX, dict(n_rows=1, V=16), dict(equal=True)))
    out.append(Case("softmax_V65536_equal", "softmax", K_SOFTMAX, dict(n_rows=1, V=65536), dict(equal=True)))
    for V in (16, 4112, 8208, 65536):
        nfull = len(score_targets(V)) + 4
        out.append(Case(f"score_V{V}_all", "score_rows", K_SCORE, dict(n_rows=nfull, V=V), dict(seed=f"score{V}")))
        for lo in range(0, nfull - 4, 5):                           # five rows per launch and ...
            out.append(Case(f"score_V{V}_five_{lo}", "score_rows", K_SCORE, dict(n_rows=5, V=V), dict(seed=f"score{V}", row=lo, twin=f"score_V{V}_all")))
        for lo in (0, nfull - 4, nfull - 2, nfull - 1):             # ... one row per launch: the same bits
            out.append(Case(f"score_V{V}_one_{lo}", "score_rows", K_SCORE, dict(n_rows=1, V=V), dict(seed=f"score{V}", row=lo, twin=f"score_V{V}_all")))
    for V in (16, 272, 4112, 65520, 65536):
        per = -(-V // SEGS)
        nspots = len({i for s in range(1, SEGS) for i in (per * s - 1, per * s) if 0 < i < V} | {0, V - 1})
        out.append(Case(f"argmax_V{V}_spots", "argmax", K_ARGMAX, dict(n_rows=nspots, V=V), dict(what="spots")))
        out.append(Case(f"argmax_V{V}_ties", "argmax", K_ARGMAX, dict(n_rows=8, V=V), dict(what="ties")))
    for n in (1, 255, 256, 257):
        out.append(Case(f"adjust_n{n}", "logit_edit", K_ADJUST, dict(n_rows=5, V=4112, n=n), {}))
    out.append(Case("adjust_V65536_n257", "logit_edit", K_ADJUST, dict(n_rows=3, V=65536, n=257), {}))
    for V, nr, n in ((16, 6, 3), (4112, 7, 4), (65536, 5, 3), (64, 4, 1)):
        out.append(Case(f"mask_V{V}_n{n}", "logit_edit", K_MASK, dict(n_rows=nr, V=V, n=n), {}))
    return out


_ALL = []


def all_cases():
    if not _ALL:
        _ALL.extend(sampler_cases() + utility_cases())
        assert len({c.name for c in _ALL}) == len(_ALL) and all(c.group in GROUPS for c in _ALL)
    return list(_ALL)


# ------------------------------------------------------------------------------------------------
# coverage, from the table alone
# ------------------------------------------------------------------------------------------------
def row_traces(c, d):
    """(row spec, trace) of every served sampler row of the case."""
    out = []
    for r in d["rows"]:
        if served(c, r):
            t = {}
            expect(d["S"][r["src"]], r, trace=t)
            t["kernel"] = kernel_of_row(c, r)
            t["single_typical"] = r["kind"] == TYP and int(d["S"][r["src"]].live.sum()) == 1
            out.append((r, t))
    return out


WANTED = ([f"{k},{f}" for k in ("nucleus<1024>", "nucleus<8192,miro>", "sample_wide") for f in ("FULL", "part")]
          + [f"windows {w}" for w in range(1, 9)] + ["end cut_w0", "end cut_beyond", "end ran_out_w0", "end ran_out_beyond", "end bound_w0", "end bound_beyond",
             "pass B last by n", "pass B last by wn < k", "id bound: n_ge > k", "id bound: n_ge > NC", "need with n_gt > 0 beyond window 0", "thr 0xFFFFFFFF", "top_k 0", "out_prob null",
             "find_or_first in window 0", "find_or_first beyond", "found beyond window 0"]
          + [f"flags {a}{b}{w}" for a in (0, 1) for b in (0, 1) for w in (0, 1)])


def coverage(cases, datas):
    """What the sampler cases reach (the strings of WANTED), from the table and the reference alone."""
    got = set()
    for c, d in zip(cases, datas):
        if c.kind != K_NUCLEUS:
            continue
        got.add("flags %d%d%d" % (c.p["any_nucleus_typical"], c.p["any_mirostat"], c.p["any_wide"]))
        if not c.o.get("prob", True):
            got.add("out_prob null")
        for r, t in row_traces(c, d):
            got.add(t["kernel"])
            if t.get("top_k_0"):
                got.add("top_k 0")
                continue
            if t["single_typical"]:
                got.add("thr 0xFFFFFFFF")
            if r["wide"]:
                got.add(f"windows {t['windows']}")
                got.add("end " + t["end"])
                if t["idb_wide"]:
                    got.add("id bound: n_ge > k")
                if t["need_mixed_later"]:
                    got.add("need with n_gt > 0 beyond window 0")
                if t["end"].endswith("_beyond"):
                    got.add("pass B last by wn < k" if t["last_wn_lt_k"] else "pass B last by n")
                    got.add({"found_later": "found beyond window 0", "first_later": "find_or_first beyond"}.get(t["draw"], "found in window 0 of pass B"))
                elif t["draw"].startswith("first"):
                    got.add("find_or_first in window 0")
            else:
                if t["idb_narrow"]:
                    got.add("id bound: n_ge > NC")
                if t["draw"].startswith("first"):
                    got.add("find_or_first in window 0")
    return got


def coverage_gaps(cases, datas):
    got = coverage(cases, datas)
    return [w for w in WANTED if w not in got]

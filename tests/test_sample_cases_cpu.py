"""CPU: the sampling / vocabulary-row probe's table proved without a GPU (tests/sample_cases.py, DESIGN.md "Sampling and vocabulary-row probe").

  * coverage, from the table and the reference alone: the six sampler instantiations, every window count 1 .. 8, every way pass A ends, both
    `last` conditions of pass B, both id-bound conditions, thr = 0xFFFFFFFF, top_k = 0, out_prob null, all eight flag combinations;
  * the windowed, vectorised reference equals oracle.rwkv_ref nucleus_ref / typical_ref / mirostat_ref on every case (every row whose walk is
    at most 2048 entries deep, and the deepest draw of every case beyond that: the oracle's loops are scalar Python);
  * family A's sums are exact, family B's margins and key gaps hold on every row, family C's calibration is consistent;
  * the reference (for the utilities: an fp32 restatement in the kernel's order) passes the very checks the GPU results face, the softmax
    restatement within a quarter of its bound;
  * the checks can fail: nine one-line mistakes, each stated as a kernel would make it, are each reported wherever they change a token,
    and at least once; the parent's arg-max of a row of nothing but -inf, a write into a guard band and a doubled adjustment are reported;
  * the case file's round trip, and the probe compiles for gfx950."""
import numpy as np
import pytest

from oracle import rwkv_ref as R
from tests import sample_cases as S

CASES = S.all_cases()
SAMPLER = [c for c in CASES if c.kind == S.K_NUCLEUS]
F32, F64 = np.float32, np.float64
_DATA = {}


def data(c):
    if c.name not in _DATA:
        _DATA[c.name] = S.make(c)
    return _DATA[c.name]


def test_the_table_reaches_every_branch():
    datas = [data(c) for c in CASES]
    assert S.coverage_gaps(CASES, datas) == []
    # a statement about the table, not a constant: without a family the proof fails
    for group in ("dyadic_full", "dyadic_sets", "calibrated", "routing"):
        keep = [(c, d) for c, d in zip(CASES, datas) if c.group != group]
        assert S.coverage_gaps([c for c, _ in keep], [d for _, d in keep]), group
    assert {c.p["V"] for c in SAMPLER if c.group == "flattened"} >= {16, 512, 1040, 4112, 8208, 20000, 65520, 65536}
    assert max((b.n + 2 * S.GUARD) * b.esize for c in CASES for b in data(c)["bufs"]) <= (66 * 65536 + 2 * S.GUARD) * 4   # 64 rows and two spare ones


def oracle(Sr, r, P):
    p = P.astype(F32)
    if r["kind"] == S.NUC:
        return R.nucleus_ref(p, r["top_p"], r["top_k"], r["T"], r["u"])[0], None
    if r["kind"] == S.TYP:
        return R.typical_ref(p, r["tau"], r["top_k"], r["T"], r["u"])[0], None
    tok, sur, _ = R.mirostat_ref(p, r["tau"], r["u"])
    return tok, sur


def test_the_reference_equals_the_oracle():
    n = deep = 0
    for c in SAMPLER:
        d = data(c)
        rows = [(j, r) for j, r in enumerate(d["rows"]) if r["role"] == "draw"]
        depth = [0 if d["S"][r["src"]].walk(r) is None else int(d["S"][r["src"]].walk(r).size) for _, r in rows]
        # the oracle takes narrow rows as it takes wide ones: the narrow kernels' clamps are the engine's routing, not the sampler's meaning
        todo = [x for x, k in zip(rows, depth) if k <= 2048 and (x[1]["wide"] or S.narrow_exact(d["S"][x[1]["src"]], x[1]))]
        if max(depth, default=0) > 2048:
            todo.append(rows[int(np.argmax(depth))])
            deep += 1
        for j, r in todo:
            Sr = d["S"][r["src"]]
            tok, prob = S.expect(Sr, r)
            otok, osur = oracle(Sr, r, Sr.P())
            assert tok == otok, (c.name, j, r["kind"], r["top_k"], r["u"], tok, otok)
            if osur is not None and Sr.exact:
                assert float(prob) == pytest.approx(osur, abs=1e-6), (c.name, j)
            n += 1
    assert n >= 2000 and deep >= 15


def test_family_A_is_exact():
    n = 0
    for c in SAMPLER:
        d = data(c)
        for r in d["rows"]:
            Sr = d["S"][r["src"]]
            if Sr.fam != "A":
                continue
            kept = Sr.walk(r)
            if kept is None:
                continue
            P = Sr.P()
            assert set(np.unique(P)) <= {F32(0), F32(2.0 ** -Sr.e)} and F64(P.astype(F64).sum()) == 1.0
            pk = P[kept]
            assert (np.cumsum(pk, dtype=F32).astype(F64) == np.cumsum(pk.astype(F64))).all()        # the cut's and Mirostat's running sums
            if r["kind"] != S.MIRO:
                inv = F32(1.0) / F32(r["T"])
                assert inv in (F32(1), F32(2), F32(0.5)) and (inv != F32(0.5) or Sr.e % 2 == 0)
                q = np.power(pk, inv)
                assert (q.astype(F64) == 2.0 ** (-Sr.e * float(inv))).all()                           # p^(1/T) is a power of two ...
                assert F64(np.cumsum(q, dtype=F32)[-1]) == kept.size * 2.0 ** (-Sr.e * float(inv))    # ... and its sequential sum exact
            n += 1
    assert n >= 800


def test_every_aimed_draw_is_decisive():
    """Families A and C: a row carrying aim = (i, above) sits exactly at the CDF boundary of rank i of the walk the row gets, or one float
    above it: it picks rank i, or i + 1 (the first element behind the last), so a kept count or a cumulative off by one entry moves it."""
    n = 0
    for c in SAMPLER:
        d = data(c)
        for j, r in enumerate(d["rows"]):
            if "aim" not in r:
                continue
            Sr = d["S"][r["src"]]
            kept = Sr.walk(r)
            assert kept[S.aimed_rank(d["S"], r)] == S.expect(Sr, r)[0], (c.name, j, r["aim"], r["top_k"], r["wide"])
            if not r["wide"]:                                       # the narrow kernel's own walk (its clamps included) is the wide one
                assert (kept == Sr.walk({**r, "wide": True})).all(), (c.name, j)
            n += 1
    assert n >= 900


def test_every_named_id_bound_reports_a_bound_one_tie_low():
    """The bounds set puts the id bound at 0, 0x3FFF, 0x4000 and at the last id but one; a bound one tie low must be reported at each of them,
    in every case that carries the set.  (One tie high changes nothing there: the sorted window still starts with the same k entries; it
    shows only where a later window misses the entry retired too early, which test_the_checks_can_fail counts.)"""
    seen = 0
    for c in SAMPLER:
        if c.group != "dyadic_sets" or "bounds" not in c.o["sets"]:
            continue
        d = data(c)
        msgs = S.check_case(c, d, S.reference_results(c, d, "id_bound_low"), S.plan_line(c))
        for top_k, bound in ((1, 0), (100, 0x3FFF), (101, 0x4000), (2047, c.p["V"] - 2)):
            rows = [j for j, r in enumerate(d["rows"]) if r.get("set") == "bounds" and r["kind"] != S.MIRO and r["top_k"] == top_k]
            assert rows
            Sr = d["S"][d["rows"][rows[0]]["src"]]
            assert np.nonzero(Sr.live)[0][top_k - 1] == bound       # the top_k-th lowest live id is the bound
            for wide in (True,) + ((False,) if top_k <= S.NARROW_TOP_K else ()):
                hit = [j for j in rows if d["rows"][j]["wide"] == wide and any(f": row {j} " in m for m in msgs)]
                assert hit, (c.name, top_k, wide)
        seen += 1
    assert seen == 3


def test_family_B_margins_and_key_gaps():
    n = 0
    for c in SAMPLER:
        if c.group != "flattened":
            continue
        d = data(c)
        Sr = d["S"][0]
        r0 = d["rows"][0]
        kept = Sr.walk({**r0, "wide": True})
        key = S.sort_key(Sr.x, r0["kind"])
        cls = Sr.cls(r0["kind"])
        order = np.lexsort((np.arange(key.size), -cls))[: kept.size + 1]
        assert (order[: kept.size] == kept).all()
        kk = np.unique(key[order])                                  # the distinct keys among the top k + 1
        gap = 0.05 if r0["kind"] == S.TYP else 1e-5
        assert kk.size < 2 or np.diff(kk).min() >= gap, (c.name, np.diff(kk).min())
        if Sr.levels is not None and r0["kind"] != S.TYP and kk.size > 1:   # level rows: gaps >= 0.25
            assert np.diff(kk).min() >= 0.25 - 1e-6
        for r in d["rows"]:
            assert r["half"] >= 64 * (r["rank"] + 90) * 2.0 ** -24, (c.name, r["rank"], r["half"])
            assert S.expect(Sr, r)[0] == kept[r["rank"]]
            n += 1
        if r0["kind"] == S.MIRO:                                    # max_surprise lies >= 0.1 away from every level's surprise
            sur = -np.log2(S.softmax64(Sr.x)[[ids[0] for _, ids in Sr.levels]])
            assert np.abs(sur - r0["tau"]).min() >= 0.1
    assert n >= 2000


def level_case_classes():
    """(n_ge against k and 1024 / 8192, n_gt > 0) of the level rows of family B, from the table."""
    seen = set()
    for c in SAMPLER:
        if c.group == "flattened" and c.o["what"] == "levels" and c.o["skind"] != S.TYP:
            d = data(c)
            Sr, r = d["S"][0], d["rows"][0]
            kept = Sr.walk(r)
            cls = Sr.cls(r["kind"])
            thr = cls[kept[-1]]
            n_ge, n_gt, k = int((cls >= thr).sum()), int((cls > thr).sum()), kept.size
            nc = S.NC_MAX if r["kind"] == S.MIRO else S.NC_NARROW
            seen.add(("miro" if r["kind"] == S.MIRO else "nucleus", "le_k" if n_ge <= k else "le_nc" if n_ge <= nc else "over_nc", n_gt > 0))
    return seen


def test_level_rows_put_the_kth_key_in_every_tie_class():
    seen = level_case_classes()
    assert seen >= {("nucleus", a, b) for a in ("le_k", "le_nc", "over_nc") for b in (False, True)} | {("miro", "over_nc", False), ("miro", "over_nc", True)}, seen


@pytest.mark.parametrize("group", S.GROUPS)
def test_the_reference_passes_the_gpu_checks(group):
    cases = [c for c in CASES if c.group == group]
    assert cases
    ratios, results = [], []
    for c in cases:
        d = data(c)
        res = S.reference_results(c, d)
        results.append(res)
        msgs = S.check_case(c, d, res, S.plan_line(c), ratios)
        assert not msgs, msgs[:4]
    assert S.cross_checks(cases, results, [data(c) for c in cases]) == []
    if ratios:
        worst = max(ratios, key=lambda x: x[2])
        print(f"worst error / bound of the reference restated in fp32, {group}: {worst[2]:.4f} ({worst[1]})")
        if group == "softmax":                                      # the fp32 restatement in the kernel's order: a quarter of the bound
            assert worst[2] <= 0.25


def test_softmax_bound_is_the_addition_chain():
    assert S.softmax_bound(65536) == 4 * (256 + 16) * 2.0 ** -24 and S.softmax_bound(16) == 4 * (16 / 256 + 16) * 2.0 ** -24


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_the_checks_can_fail(mistake):
    changed_total = 0
    for c in SAMPLER:
        d = data(c)
        changed = 0
        for r in d["rows"]:
            if S.served(c, r) and r["role"] == "draw":
                Sr = d["S"][r["src"]]
                changed += S.expect(Sr, r)[0] != S.expect(Sr, r, mistake)[0]
        msgs = S.check_case(c, d, S.reference_results(c, d, mistake), S.plan_line(c))
        assert sum(": token " in m for m in msgs) == changed, (c.name, changed, msgs[:3])
        changed_total += changed
    print(f"{mistake}: {changed_total} rows change their token")
    assert changed_total >= 1


def test_other_defects_are_reported():
    by = {c.name: c for c in CASES}
    c = by["argmax_V4112_ties"]                                      # the arg-max of a row of nothing but -inf before the fix
    d = data(c)
    res = S.reference_results(c, d)
    S.own(res, d["bufs"][1])[3] = 0x7fffffff
    assert any("token" in m for m in S.check_case(c, d, res, S.plan_line(c)))
    res = S.reference_results(c, d)                                  # stage 1 writing one segment too many
    res["scratch_i"][S.GUARD + 8 * S.SEGS] = 0
    assert any("guard band" in m for m in S.check_case(c, d, res, S.plan_line(c)))
    c = by["adjust_n257"]                                            # an adjustment applied twice, and one applied for token V (the next row's token 0)
    d = data(c)
    res = S.reference_results(c, d)
    S.own(res, d["bufs"][0])[5] ^= 0x00400000
    assert S.check_case(c, d, res, S.plan_line(c))
    c = by["mask_V4112_n4"]                                          # an unlisted row masked
    d = data(c)
    res = S.reference_results(c, d)
    free = [r for r in range(c.p["n_rows"]) if r not in d["rows"]][0]
    S.own(res, d["bufs"][0])[free * c.p["V"] + 9] = 0xFF800000
    assert S.check_case(c, d, res, S.plan_line(c))
    c = by["routing_flags_100"]                                      # a row written although its kernel was not launched; a second launch that differs
    d = data(c)
    res = S.reference_results(c, d)
    j = [j for j, r in enumerate(d["rows"]) if not S.served(c, r)][0]
    S.own(res, d["bufs"][2])[j] = 0
    assert any("flag is off" in m for m in S.check_case(c, d, res, S.plan_line(c)))
    res = S.reference_results(c, d)
    S.own(res, d["bufs"][3])[0] ^= 1
    assert any("second launch" in m for m in S.check_case(c, d, res, S.plan_line(c)))
    c = by["score_V4112_one_0"]                                      # one row per launch differing from the same row among twelve
    cases = [by["score_V4112_all"], c]
    results = [S.reference_results(x, data(x)) for x in cases]
    S.own(results[1], data(c)["bufs"][2])[0] ^= 1
    assert S.cross_checks(cases, results, [data(x) for x in cases])


def test_case_file_round_trip(tmp_path):
    cases = [c for c in CASES if c.name in ("routing_flags_101", "softmax_V16_n5", "score_V16_all", "argmax_V16_ties", "adjust_n1", "mask_V16_n3")]
    assert len(cases) == 6
    datas = [data(c) for c in cases]
    path = str(tmp_path / "cases.bin")
    S.write_cases(path, cases, datas)
    back = S.read_cases(path)
    assert len(back) == len(cases)
    for c, d, (name, kind, par, bufs) in zip(cases, datas, back):
        assert (name, kind, list(par)) == (c.name, c.kind, [c.p[k] for k in S.PARAMS[c.kind]])
        assert len(bufs) == len(d["bufs"])
        for b, (role, esize, flags, nbytes, off, img) in zip(d["bufs"], bufs):
            assert (role, esize, flags, nbytes, off) == (S.ROLE[b.role], b.esize, b.flags, (b.n + 2 * S.GUARD) * b.esize, (S.GUARD + b.off) * b.esize)
            assert (img is None) == bool(b.flags & 2) and (img is None or (img == b.image).all())
    assert "out_prob" not in {b.role for b in datas[0]["bufs"]}       # an absent role: a null pointer
    # the results of a probe that writes nothing come back as what went in
    out = str(tmp_path / "results.bin")
    with open(out, "wb") as f:
        for d in datas:
            for role, a in S.untouched(d).items():
                f.write(a.tobytes())
    for d, res in zip(datas, S.read_results(out, cases, datas)):
        assert all((res[k] == v).all() for k, v in S.untouched(d).items())


def test_probe_compiles_for_gfx950(tmp_path):
    import os
    obj = S.compile_probe(tmp_path)
    assert os.path.getsize(obj) > 0

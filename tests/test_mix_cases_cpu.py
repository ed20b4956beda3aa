"""CPU: the mix / prologue / commit probe's table proved without a GPU (tests/mix_cases.py, DESIGN.md "Mix, prologue and commit probe").

  * the table reaches every instantiation and branch it exists for, from the transcribed launch rule and the engine's planner (a g++-built driver
    of tests/cpp/mix_probe_plan.h) alone; each named (C, T) -> ksp / grid.x / apply tile is what the rule gives;
  * the lattice: headroom, the sensitivity of every (mix, W1 strip, 16-token tile, 32-k step) by enumeration, and an fp32 restatement that equals
    float64 in every bit in two summation orders, the lerp fused and unfused;
  * the general values: the fp32 restatement passes the very checks the GPU results face in both orders, fused and unfused; tau is 8 x the
    measured distance, and the bound with the tie budget stays within 10 x the base bound on every element;
  * the checks can fail: six mistakes, each stated as the kernel would make it and run on every case, are reported wherever they change a bit, and
    the cases they reach are the ones that exist for them; the four steps that must not split are each one condition away from splitting;
  * the case file and the result file round trip; the probe compiles for gfx950."""
import json
import os

import numpy as np
import pytest

from tests import mix_cases as M

CASES = M.all_cases()
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def carriers(tmp_path_factory):
    return M.carrier_plans(M.build_planner(tmp_path_factory.mktemp("mix_plan")), CASES)


def lines_of(carriers):
    return [M.plan_line(c, carriers.get(c.name)) for c in CASES]


def test_the_table_reaches_every_instantiation_and_branch(carriers):
    lines = lines_of(carriers)
    assert M.coverage_gaps(lines) == []
    by = {c.name: (c, l) for c, l in zip(CASES, lines)}
    for c, l in by.values():
        if "want_ksp" in c.o:
            assert (l["form"], l["ksp"]) == ("split", c.o["want_ksp"]), c.name
    # the named shapes
    gx = lambda n: by[n][1]["grid1"][0]
    assert gx("wide_c1536_t200_hilo_dm64_lattice") == 7 and gx("wide_c512_t500_hi_dm32_lattice") == 3 and gx("wide_c256_t65_hilo_dm64_general") == 8
    for n in ("wide_nosplit_t512_mg_null_hi_dm32_lattice", "wide_nosplit_t520_hilo_dm32_lattice", "wide_nosplit_t192_mp_null_hi_dm64_lattice", "wide_nosplit_t192_ksp_max1_hilo_dm64_lattice"):
        assert by[n][1]["form"] == "wide" and by[n][1]["split"] == 0, n
    assert by["split_c256_t512_hi_dm32_lattice"][1]["apply_nt"] == 1 and by["split_c2048_t512_hi_dm32_lattice"][1]["apply_nt"] == 2
    assert {l["apply_nt"] for c, l in by.values() if c.name.startswith("ksl_c4096_t256")} == {2}
    assert {l["apply_nt"] for c, l in by.values() if c.group == "mix_ksliced" and not c.name.startswith("ksl_c4096_t256")} == {1}
    # the batch tails of phase 1: k-steps per wave against the batch
    tails = {(M.mix_rule(c)["kst"], M.mix_rule(c)["KB"]) for c in CASES if c.name.startswith("dec_tail")}
    assert tails == {(6, 4), (6, 5), (11, 10)}
    # a small-K-eligible launch that carries a commit stays on the decode kernel, one extra block
    for c, l in by.values():
        if c.kind != M.K_MIX:
            assert l["carrier"]["path"] == "decode" and l["carrier"]["smallk_without_commit"] == 1 and l["launch_grid"] == l["carrier"]["grid"]
    assert [c.name for c in CASES if c.o.get("last") == -1] == ["commit_slot3_last_none"]
    # a statement about the table, not a constant
    assert M.coverage_gaps([l for l in lines if l.get("form") != "lnp"])
    assert M.coverage_gaps([l for l in lines if l.get("ksp") != 16])


def test_buffers_follow_the_probe_discipline():
    for c in CASES:
        d = M.make(c)
        P = c.p
        roles = {b.role: b for b in d["bufs"]}
        assert len(roles) == len(d["bufs"])
        for b in d["bufs"]:
            if b.flags & 2:
                assert b.flags & 1, f"{c.name}: {b.role} is written and never read back"
            else:
                s = M.SENT32 if b.esize == 4 else M.SENT16
                assert (b.image[:M.GUARD] == s).all() and (b.image[-M.GUARD:] == s).all() and b.image.size == b.n + 2 * M.GUARD
        assert all(("olo%d" % i in roles) == bool(P["hilo"] or P["carrier_hilo"]) for i in range(5)), c.name
        if c.kind == M.K_MIX and not P["lnp"]:
            z = M.unpack_opd(roles["zhi"].image[M.GUARD:-M.GUARD], M.ceil16(P["T"]), P["ldz"])
            assert (z[P["T"]:] == M.SENT16).all() and (z[:, P["C"]:] == M.SENT16).all()
        if "sx" in roles:
            sx = M.bits(d["sx"]).reshape(P["nslots"], -1)
            live = [] if c.kind == M.K_COMMIT else [d["slot"]]
            CC = P["commit_C"] or P["C"]
            assert P["sx_slot_stride"] > CC and all((sx[s] == M.SENT32).all() for s in range(P["nslots"]) if s not in live) and (sx[:, CC:] == M.SENT32).all()


@pytest.mark.parametrize("group", M.GROUPS)
def test_lattice_is_exact_and_sensitive(group, carriers):
    n = 0
    for c in CASES:
        if c.group != group or not c.lattice:
            continue
        d = M.make(c)
        line = M.plan_line(c, carriers.get(c.name))
        if c.kind != M.K_COMMIT:
            assert M.lattice_proof(c, d) == [], c.name
        want = M.emulate(c, d, F64)
        for order in (0, 1):
            for fused in (False, True):
                if c.p["T"] * c.p["C"] > 300000 and order != int(fused):
                    continue                                          # the largest cases: two of the four combinations
                res = M.emulate(c, d, F32, order, fused)
                assert all(np.array_equal(res[k], want[k]) for k in want if not k.startswith("cout")), f"{c.name}: the fp32 restatement differs from float64 (order {order}, fused {fused})"
                if (order, fused) in ((0, False), (1, True)):
                    assert M.check_case(c, d, res, line) == [], c.name
        if c.kind != M.K_MIX:                                         # the carrier's linear problems are exact too: headroom of what they read
            ops = [M.unpack_opd(want[f"ohi{i}"][M.GUARD:-M.GUARD], 16, c.p["ldh"])[:1, :c.p["C"]].view(np.float16).astype(F64) for i in range(5)] if c.kind == M.K_PAIR else \
                  [h.astype(F64) + (l.astype(F64) if d["clo"] else 0) for h, l in zip(d["chi"], d["clo"] or d["chi"])]
            for i in range(3):
                x = ops[M.CARRIER_MIX[i]]
                q = 1 / 32 if c.kind == M.K_COMMIT else 1 / 16        # eighths + thirty-seconds; the mix's outputs: sixteenths below 64, which f16 holds
                assert not ((x / q) % 1).any() and np.abs(x).max() < 64, c.name
                assert (np.abs(x) @ np.abs(d["cW"][i].astype(F64)).T).max() / q < M.HEADROOM, c.name
        n += 1
    assert n


@pytest.mark.parametrize("group", M.GROUPS[:-1])
def test_general_cases_are_well_conditioned(group, carriers, capsys):
    worst, dist, distz, cap = (0.0, ""), 0.0, 0.0, 0.0
    for c in CASES:
        if c.group != group or c.lattice:
            continue
        d = M.make(c)
        line = M.plan_line(c, carriers.get(c.name))
        e64 = M.evaluate(c, d)
        base = [M.ew_bound(M.f16_sat(e64["out"][i])) for i in range(5)]
        cap = max(cap, max(float(((b + t) / b).max()) for b, t in zip(base, M.tie_budget(c, d, e64, M.TAU[group], M.TAU_Z))))
        for order in (0, 1):
            for fused in (False, True):
                if c.p["T"] * c.p["C"] > 300000 and order != int(fused):
                    continue                                          # the largest cases: two of the four combinations
                ratios = []
                assert M.check_case(c, d, M.emulate(c, d, F32, order, fused), line, ratios) == [], c.name
                worst = max(worst, (ratios[-1][2], c.name))
            if not c.p["hilo"]:
                dm, dz = M.rounding_distance(c, d, e64, M.evaluate(c, d, F32, order, z_from=e64["z"] if c.p["lnp"] else None))
                dist, distz = max(dist, dm), max(distz, dz)
    assert cap <= M.BOUND_CAP, f"bound with the tie budget / base bound reaches {cap}"
    assert 0.9 * M.TAU[group] <= 8 * dist <= M.TAU[group], f"tau of {group}: measured {8 * dist}"
    if group == "mix_lnp":
        assert 0.9 * M.TAU_Z <= 8 * distz <= M.TAU_Z, f"tau_z: measured {8 * distz}"
    with capsys.disabled():
        print(f"\n{group}: fp32 restatement worst error / bound {worst[0]:.4f} ({worst[1]}), tau {M.TAU[group]:.2e} (8 x {dist:.3e}), largest bound / base bound {cap:.2f}")


BIG = {"mix_wide": "skip_strips", "mix_split": "tile16_index", "mix_ksliced": "slice_twice"}


@pytest.fixture(scope="module")
def reached(carriers):
    out = {mut: set() for mut in M.MUTATIONS}
    for c in CASES:
        if c.p["T"] * c.p["C"] > 300000 and not c.lattice:
            continue
        d = M.make(c)
        line = M.plan_line(c, carriers.get(c.name))
        good = M.emulate(c, d, F32)
        for mut in M.MUTATIONS:
            if c.kind == M.K_COMMIT and mut != "commit_row_slot":
                continue                                              # no mix launch in the case: nothing of it is computed
            if c.p["T"] * c.p["C"] > 300000 and mut not in ("tail_kstep", BIG[c.group]):
                continue                                              # the largest cases: phase 1's mistake and the one of their own form's code
            bad = M.emulate(c, d, F32, 0, False, mut)
            if all(np.array_equal(good[k], bad[k]) for k in good):
                continue                                              # the mistake does not reach this case: the buffers are the correct ones
            assert M.check_case(c, d, bad, line), f"{mut} changes {c.name} and goes unnoticed"
            out[mut].add(c.name)
    return out


def test_the_checks_can_fail(reached):
    """Each mistake is found in the cases that exist for it; where it is not found it changed no bit."""
    swept = [c for c in CASES if c.lattice or c.p["T"] * c.p["C"] <= 300000]
    rule = {c.name: M.mix_rule(c) for c in swept if c.kind != M.K_COMMIT}
    # a batch that is not full exists exactly where kst is no multiple of KB: the tail cases, and every C = 256 case (one k-step per wave)
    assert reached["tail_kstep"] == {n for n, r in rule.items() if r["kst"] % r["KB"]}
    assert {n for n in rule if n.startswith("dec_tail")} <= reached["tail_kstep"] and "split_c2048_t512_hi_dm64_lattice" not in reached["tail_kstep"]
    # five at a time with `<=`: slice ksp - 1 once more unless ksp is a multiple of 5
    sliced = {n for n, r in rule.items() if r["ksp"] > 1}
    assert reached["slice_twice"] == {n for n in sliced if "_ksp5_" not in n} and {k for k in (2, 3, 4, 6, 8, 16) if any(f"_ksp{k}_" in n for n in reached["slice_twice"])} == {2, 3, 4, 6, 8, 16}
    assert reached["prev_slot0"] == {n for n, r in rule.items() if r["form"] == "lnp" and "slot3" in n} and len(reached["prev_slot0"]) == 13
    assert reached["commit_row_slot"] == {"commit_slot3_hi", "commit_slot3_hilo", "commit_slot3_c4096", "pair_slot3"}
    assert {n.split("_t")[0] for n in reached["skip_strips"]} == {"wide_c1536", "wide_c512"} and all("nosplit" not in n for n in reached["skip_strips"])
    assert reached["tile16_index"] == {n for n in rule if n.startswith("split_c256_t512")} and len(reached["tile16_index"]) == 8


def test_steps_that_must_not_split_would_split_otherwise():
    """Each of the four is one condition away from the two-launch form: with that condition lifted the rule splits."""
    by = {c.name: c for c in CASES}
    split = lambda c, **kw: M.v6_split(**{**dict(T=c.p["T"], C=c.p["C"], hilo=bool(c.p["hilo"]), has_mg_hi=c.o["mg_hi"], has_mg_lo=c.o["mg_lo"], has_mp=c.o["mp"] > 0,
                                                ksp_min_t=c.p["ksp_min_t"], ksp_blocks=c.p["ksp_blocks"], ksp_max=c.p["ksp_max"]), **kw})
    for fam in ("lattice", "general"):
        for name, lifted, want in ((f"wide_nosplit_t512_mg_null_hi_dm32_{fam}", dict(has_mg_hi=True), 1), (f"wide_nosplit_t520_hilo_dm32_{fam}", dict(T=512), 1),
                                   (f"wide_nosplit_t192_mp_null_hi_dm64_{fam}", dict(has_mp=True), 2), (f"wide_nosplit_t192_ksp_max1_hilo_dm64_{fam}", dict(ksp_max=16), 2)):
            c = by[name]
            assert split(c) == 0 and M.mix_rule(c)["form"] == "wide", name
            assert split(c, **lifted) == want, name


def test_general_prologue_z_keeps_clear_of_rounding_ties():
    n = 0
    for c in CASES:
        if c.p["lnp"] and not c.lattice:
            z = M.evaluate(c, M.make(c))["zpre"]
            assert (M._tie_distance(z) >= 4 * M.TAU_Z * 0.99).all() and (np.abs(z) >= 0.125).all(), c.name
            n += 1
    assert n == 12


def test_case_file_round_trip(tmp_path, carriers):
    cases = [c for c in CASES if c.name in ("dec_c256_t17_hilo_dm32_lattice", "lnp_c256_np1_dm64_slot3_general", "commit_slot3_hilo", "pair_slot3")]
    datas = [M.make(c) for c in cases]
    M.write_cases(str(tmp_path / "cases.bin"), cases, datas)
    results = [M.emulate(c, d) for c, d in zip(cases, datas)]
    with open(tmp_path / "results.bin", "wb") as f:
        for d, r in zip(datas, results):
            for b in d["bufs"]:
                if b.flags & 1:
                    f.write(r[b.role].tobytes())
    back = M.read_results(str(tmp_path / "results.bin"), cases, datas)
    for c, d, r, b in zip(cases, datas, results, back):
        assert r.keys() == b.keys() and all(np.array_equal(r[k], b[k]) for k in r)
        line = json.loads(json.dumps(M.plan_line(c, carriers.get(c.name))))
        assert M.check_case(c, d, b, line) == []
    # the header the probe parses: magic, count, then the first case's name
    raw = open(tmp_path / "cases.bin", "rb").read(64)
    assert raw[:4] == b"MPRB" and int.from_bytes(raw[4:8], "little") == len(cases) and raw[12:12 + len(cases[0].name)] == cases[0].name.encode()


def test_probe_compiles_for_gfx950(tmp_path):
    obj = M.compile_probe(tmp_path)
    assert os.path.getsize(obj) > 0

"""CPU: the GEMM probe's case table (tests/gemm_cases.py) proved without a GPU — the lattice really is a fixed point of the quantisers, every
intermediate of every exact case really is representable in fp32, no 32-k step can cancel, the one-hot cases use every code, the operand
pack / unpack match the kernels' index function, the table reaches the coverage list through the engine's planner compiled with g++, the
checker accepts a correct result and names a damaged one, and the probe compiles for gfx950 (and links when the kernel objects are there)."""
import os

import numpy as np
import pytest

from oracle import rwkv_ref as R
from tests import gemm_cases as G

CASES = G.all_cases()
SMALL = [c for c in CASES if sum(p.rows * p.K for p in c.probs) * c.T <= 80 << 20]   # everything but the two large-grid cases


@pytest.fixture(scope="module")
def datas():
    return {c.name: G.make(c) for c in CASES}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = G.build_planner(tmp_path_factory.mktemp("plan"))
    return G.plan_cpu(exe, CASES)


def test_table_size_and_groups():
    assert 100 <= len(CASES) <= 300                                  # the low hundreds of launches
    assert {c.group for c in CASES} == set(G.GROUPS)
    for c in CASES:
        assert all(p.rows <= 400 and p.K <= 3072 for p in c.probs) or {"big_grid", "spb_unforced"} & set(c.tags), c.name


def test_lattice_is_a_fixed_point_of_the_quantisers(datas):
    for c in CASES:
        if c.family == "onehot":
            continue
        for p, W in zip(c.probs, datas[c.name]["W"]):
            assert np.array_equal(G.fake_quant(p, W).view(np.uint16), W.view(np.uint16)), (c.name, G.FMT_NAME[p.fmt])
            if p.fmt == G.INT8:                                       # a = 1/16 in every block, both ends of the code range present
                q, a, _ = R.quant_int8(W)
                assert (a == np.float16(1.0 / 16)).all() and (q.reshape(p.rows, -1, 128).min(axis=2) == 0).all() and (q.reshape(p.rows, -1, 128).max(axis=2) == 255).all()
            if p.fmt == G.NF4:                                        # absmax a power of two that varies, +-absmax in every block
                idx, am = R.quant_nf4(W)
                assert set(np.unique(idx)) == {0, 7, 15} and len(np.unique(am)) > 1 and (np.log2(am.astype(np.float64)) % 1 == 0).all()


def representable(v):
    return np.array_equal(v.astype(np.float32).astype(np.float64), v)


def test_headroom_and_exact_intermediates(datas):
    worst = 0.0
    for c in SMALL:
        if c.family == "onehot":
            continue
        d = datas[c.name]
        for i, p in enumerate(c.probs):
            h = G.headroom(c, d, i)
            worst = max(worst, h)
            assert h < G.HEADROOM, (c.name, i, h)
            stages = []
            G.reference(c, d, i, stages=stages)
            exact = stages if c.family == "lattice" else stages[:2]   # act family: the accumulator and accumulator + bias
            for s in exact:
                assert representable(s), (c.name, i, "an intermediate of the epilogue is not an fp32 value")
            if c.family == "lattice" and p.act == G.ACT_RELU2:
                assert np.abs(stages[1]).max() / (G.W_QUANTUM[p.fmt] * (0.25 if c.hilo else 1.0)) < 4096, (c.name, i, "the square needs more than 24 bits")
    print(f"worst sum |w||x| / quantum: 2^{np.log2(worst):.2f} (bound 2^20)")


def test_no_kstep_can_cancel(datas):
    """For every (16-row strip, 16-token tile, 32-k step) at least half of the partial sums are non-zero."""
    total = nz = 0
    for c in SMALL:
        if c.family != "lattice":
            continue
        d = datas[c.name]
        for i, p in enumerate(c.probs):
            s = G.kstep_sums(c, d, i) != 0                            # [T][rows][K / 32]
            for t0 in range(0, c.T, 16):
                blk = s[t0:t0 + 16].reshape(min(16, c.T - t0), p.rows // 16, 16, p.K // 32)
                frac = blk.mean(axis=(0, 2))                          # [strip][k-step]
                assert frac.min() >= 0.5, (c.name, i, t0, float(frac.min()))
            total += s.size
            nz += int(s.sum())
    print(f"non-zero 32-k partial sums: {100.0 * nz / total:.1f} %")
    assert nz / total > 0.9


def test_onehot_cases_use_every_code_and_every_column(datas):
    for fmt, ncode in ((G.INT8, 256), (G.NF4, 16)):
        cs = [c for c in CASES if c.family == "onehot" and c.probs[0].fmt == fmt]
        cols = set()
        for c in cs:
            d = datas[c.name]
            p, W = c.probs[0], d["W"][0]
            if fmt == G.INT8:
                q, a, b = R.quant_int8(W)
                assert (a == 0).any() and (np.log2(a[a > 0].astype(np.float64)) % 1 != 0).any(), c.name     # constant blocks; scales that are no powers of two
            else:
                q, am = R.quant_nf4(W)
                assert (am == 0).any() and (np.log2(am[am > 0].astype(np.float64)) % 1 != 0).any(), c.name
            assert len(np.unique(q)) == ncode, (c.name, len(np.unique(q)))
            assert len(set(d["perm"])) == c.T
            x = d["xhi"].astype(np.float64) + (d["xlo"].astype(np.float64) if c.hilo else 0.0)
            assert ((x != 0).sum(axis=1) == 1).all()
            want = G.fake_quant(p, W).astype(np.float64)[:, d["perm"]].T * x[np.arange(c.T), d["perm"]][:, None]
            assert np.array_equal(G.reference(c, d, 0), want) and representable(want)
            if c.mode == 2 and c.T == 64:
                cols |= set(d["perm"].tolist())
        assert cols == set(range(512)), "the decode launches of the family read back every column"
        assert {c.lo_mode for c in cs} == {"hi", "lo", "both"}


def test_operand_pack_and_unpack_match_opd_off():
    rng = np.random.default_rng(5)
    for T16, ld in ((16, 32), (48, 96), (32, 352)):
        x = rng.integers(0, 65536, (T16, ld)).astype(np.uint16)
        flat = G.pack_opd(x)
        assert np.array_equal(G.unpack_opd(flat, T16, ld), x)
        t, k = np.meshgrid(np.arange(T16), np.arange(ld), indexing="ij")
        off = G.opd_off(t, k, ld)
        assert sorted(off.reshape(-1).tolist()) == list(range(T16 * ld))
        assert np.array_equal(flat[off], x)


def test_tiled_layouts_follow_the_layout_comments():
    """Element by element from the sentences of rwkv_kernels.h / the load-time kernels' comments (not from the reshapes of gemm_cases)."""
    rng = np.random.default_rng(6)
    rows, K = 32, 512
    W = rng.integers(0, 65536, (rows, K)).astype(np.uint16)
    q = rng.integers(0, 256, (rows, K)).astype(np.uint8)
    idx = rng.integers(0, 16, (rows, K)).astype(np.uint8)
    t16 = G.tiled_f16(W)
    p8, _ = G.tiled_int8(q, np.zeros((rows, K // 128), np.float16), np.zeros((rows, K // 128), np.float16))
    p4, _ = G.tiled_nf4(idx, np.zeros((rows, K // 64), np.float16))
    for row, k in rng.integers(0, [rows, K], (400, 2)):
        strip, r = row // 16, row % 16
        lane = r + 16 * ((k % 32) // 8)
        assert t16[((strip * (K // 32) + k // 32) * 64 + lane) * 8 + k % 8] == W[row, k]
        assert p8[((strip * (K // 64) + k // 64) * 64 + lane) * 16 + (8 if k % 64 >= 32 else 0) + k % 8] == q[row, k]
        byte = p4[((strip * (K // 128) + k // 128) * 64 + lane) * 16 + (k % 128) // 32 * 4 + (k % 8) % 4]
        assert (byte >> 4 if k % 8 >= 4 else byte & 15) == idx[row, k]
    a = rng.integers(0, 65536, (rows, K // 128)).astype(np.uint16).view(np.float16)
    b = rng.integers(0, 65536, (rows, K // 128)).astype(np.uint16).view(np.float16)
    am = rng.integers(0, 65536, (rows, K // 64)).astype(np.uint16).view(np.float16)
    _, s8 = G.tiled_int8(q, a, b)
    _, s4 = G.tiled_nf4(idx, am)
    s8, s4 = s8.view(np.uint16), s4.view(np.uint16)
    for row in range(rows):
        for blk in range(K // 128):
            at = (((row // 16) * (K // 256) + blk // 2) * 16 + row % 16) * 2 + blk % 2
            assert (s8[2 * at], s8[2 * at + 1]) == (a.view(np.uint16)[row, blk], b.view(np.uint16)[row, blk])
        for blk in range(K // 64):
            assert s4[(((row // 16) * (K // 256) + blk // 4) * 16 + row % 16) * 4 + blk % 4] == am.view(np.uint16)[row, blk]


def test_table_reaches_the_coverage_list_through_the_planner(plans):
    refused = [(c.name, p) for c, p in zip(CASES, plans) if p["status"] != "ran"]
    assert not refused, refused
    gaps = G.coverage_gaps(CASES, plans)
    assert not gaps, gaps
    # the coverage check itself notices a missing family
    assert G.coverage_gaps([c for c in CASES if c.group != "smallk"], [p for c, p in zip(CASES, plans) if c.group != "smallk"])


def test_checker_accepts_the_reference_and_names_a_damaged_result(datas, plans):
    by = {c.name: (c, p) for c, p in zip(CASES, plans)}
    for name in ("dec-five-T18", "dec-partial-ksb4-int8-K1024", "tile12-kcopies3", "epi-exact-T20-hilo", "epi-saturate-T7", "smallk-T17", "onehot-nf4-dec2-both", "epi-act-T5-dec"):
        c, plan = by[name]
        d = datas[name]
        res = G.emulate(c, d, plan)
        assert G.check_case(c, d, res, plan) == [], name
        p = c.probs[0]
        if p.f32:                                                     # one element wrong by one k-step's sum; one stray write; one guard word
            body = res["out"][:c.nslab * c.T * c.ldo].reshape(c.nslab, c.T, c.ldo)
            t, row = c.T - 1, p.rows - 1
            keep = body[0, t, p.ocol + row]
            if c.family == "lattice" and p.act == G.ACT_NONE and p.post == G.POST_NONE and not p.bias and not p.partial:
                step = G.kstep_sums(c, d, 0)[t, row]
                j = int(np.flatnonzero(step)[0])
                body[0, t, p.ocol + row] = np.float32(G.f32_of(np.array([keep], np.uint32))[0] - step[j]).view(np.uint32)
                msgs = G.check_case(c, d, res, plan)
                assert len(msgs) == 1 and f"k-step {j} " in msgs[0] and "dropped" in msgs[0] and name in msgs[0] and f"(t {t}, row {row}" in msgs[0], msgs
                body[0, t, p.ocol + row] = keep
            body[c.nslab - 1, 0, c.ldo - 1] = 0
            assert any("outside what the launch owns" in m for m in G.check_case(c, d, res, plan)), name
            body[c.nslab - 1, 0, c.ldo - 1] = G.SENT32
            res["out"][-1] = 0
            assert any("guard band" in m for m in G.check_case(c, d, res, plan)), name
            res["out"][-1] = G.SENT32
        assert G.check_case(c, d, res, plan) == [], name
        res["pay"][0] = res["pay"][0].copy()
        res["pay"][0][3] ^= 1
        assert any("payload" in m for m in G.check_case(c, d, res, plan)), name
    c, plan = by["epi-exact-T7"]
    res = G.emulate(c, datas[c.name], plan)
    body = G.unpack_opd(res["ohi"][:16 * c.ldh], 16, c.ldh)
    body[c.T, c.probs[2].hcol] = 0                                     # a write into operand row T
    res["ohi"] = np.concatenate([G.pack_opd(body), res["ohi"][-G.GUARD:]])
    assert any("operand output hi outside what the launch owns" in m and "rows >= T" in m for m in G.check_case(c, datas[c.name], res, plan))


def test_case_files_round_trip(tmp_path, datas, plans):
    cs = [c for c in CASES if c.group == "smallk"]
    path = str(tmp_path / "cases.bin")
    G.write_cases(path, cs, [datas[c.name] for c in cs])
    raw = np.fromfile(path, np.uint8)
    want = 8
    for c in cs:
        T16 = (c.T + 15) // 16 * 16
        want += 14 * 4 + T16 * c.ldx * 2 * (2 if c.hilo else 1) + 2 * c.T * c.ldm * 4
        want += sum(12 * 4 + p.rows * p.K * 2 + (p.rows * 4 if p.bias else 0) for p in c.probs)
    assert raw.size == want
    out = str(tmp_path / "results.bin")
    with open(out, "wb") as f:
        for c, plan in zip(cs, [p for cc, p in zip(CASES, plans) if cc.group == "smallk"]):
            r = G.emulate(c, datas[c.name], plan)
            f.write(np.int32(0).tobytes() + r["out"].tobytes() + r["ohi"].tobytes() + r["olo"].tobytes())
            for a, b in zip(r["pay"], r["sc"]):
                f.write(a.tobytes() + b.tobytes())
    back = G.read_results(out, cs)
    for c, r, plan in zip(cs, back, [p for cc, p in zip(CASES, plans) if cc.group == "smallk"]):
        assert G.check_case(c, datas[c.name], r, plan) == []


def test_probe_compiles_for_gfx950_and_links_when_the_kernel_objects_are_there(tmp_path):
    from ai00_server_amd import build as B
    obj = G.compile_probe(tmp_path)
    assert os.path.getsize(obj) > 0
    if all(os.path.exists(p) for p in B.kernel_objects()) and not B.needs_build():
        exe = G.build_probe()
        assert os.access(exe, os.X_OK)

"""CPU: Quant::SF4 without a GPU — the code book against its derivation and its golden file, the quantiser arithmetic of tests/sf4_ref.py, the
planner's indifference between NF4 and SF4 on every recorded NF4 launch, the constant across the public surfaces, and the proof that the case
table of tests/sf4_cases.py is exact (the argument of tests/test_gemm_cases_cpu.py for the one-hot family)."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import rwkv_ref as R
from tests import gemm_cases as G
from tests import sf4_cases as SC
from tests import sf4_ref as S
from tests import test_gemm_plan_cpp as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = SC.cases()


@pytest.fixture(scope="module")
def datas():
    return {c.name: SC.make(c) for c in CASES}


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def test_table_matches_the_golden_file_and_the_construction():
    t32, bits = S.golden()
    assert np.array_equal(S.SF4_TABLE, t32)
    assert np.array_equal(S.SF4_TABLE_F16.view(np.uint16), bits)
    assert S.SF4_TABLE[0] == -1 and S.SF4_TABLE[7] == 0 and S.SF4_TABLE[15] == 1 and (np.diff(S.SF4_TABLE_F64) > 0).all()
    # the closed form is a CDF: 1/2 at 0, symmetric, and the quantile inverts it
    ppf = S.ppf_by_bisection(S.t5_cdf)
    for p in (0.5, 0.6, 0.9, S.DELTA, 0.999):
        assert abs(S.t5_cdf(ppf(p)) - p) < 1e-15 and abs(S.t5_cdf(-ppf(p)) - (1 - p)) < 1e-15


def test_the_construction_with_the_normal_ppf_is_nf4():
    """The same construction over the standard normal gives the oracle's NF4 table: identical fp16 code points, and the float32 table to
    one float32 ulp at 1 (2^-23; the published digits come from a float32 pipeline, this one rounds once from float64)."""
    nf = S.construct(S.ppf_by_bisection(S.normal_cdf))
    assert np.abs(nf - R.NF4_TABLE.astype(np.float64)).max() <= 2.0 ** -23
    assert np.array_equal(nf.astype(np.float32).astype(np.float16), R.NF4_TABLE_F16)


def test_table_against_scipy():
    st = pytest.importorskip("scipy.stats")
    assert np.abs(S.construct(lambda p: float(st.t.ppf(p, S.T_DOF))) - S.SF4_TABLE_F64).max() <= 1e-9
    assert np.abs(S.construct(lambda p: float(st.norm.ppf(p))) - S.construct(S.ppf_by_bisection(S.normal_cdf))).max() <= 1e-9


def test_fp16_code_points_are_strictly_increasing():
    t = S.SF4_TABLE_F16.astype(np.float64)
    assert (np.diff(t) > 0).all()
    assert (S.SF4_MID > S.SF4_TABLE[:-1]).all() and (S.SF4_MID < S.SF4_TABLE[1:]).all()
    assert not np.array_equal(S.SF4_TABLE_F16, R.NF4_TABLE_F16)


# ---- the quantiser --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v6-small", "v7-small", "v5-small"])
def test_fake_quant_is_idempotent_on_the_synthetic_checkpoints(name):
    t = R.synth_named(name)
    info = R.model_info(t)
    n = 0
    for l in range(info.num_layer):
        for m in R.quantised_matrix_names(int(info.version)):
            w = np.asarray(t[f"blocks.{l}.{m}"], np.float16)
            q = S.fake_quant_sf4(w)
            assert np.array_equal(S.fake_quant_sf4(q).view(np.uint16), q.view(np.uint16)), (name, l, m)
            n += 1
    assert n == info.num_layer * len(R.quantised_matrix_names(int(info.version)))


def test_zero_and_constant_blocks():
    w = np.zeros((16, 128), np.float16)
    w[:, 64:] = 0.37
    idx, am = S.quant_sf4(w)
    assert (am[:, 0] == 0).all() and (idx[:, :64] == 7).all()         # x / 1 = 0 lies above exactly the seven negative midpoints
    assert (am[:, 1] == np.float16(0.37)).all() and (idx[:, 64:] == 15).all()
    q = S.dequant_sf4(idx, am)
    assert np.array_equal(q.view(np.uint16), w.view(np.uint16))
    w[:, 64:] = -0.37
    assert np.array_equal(S.fake_quant_sf4(w).view(np.uint16), w.view(np.uint16)) and (S.quant_sf4(w)[0][:, 64:] == 0).all()


def test_prequantise_replaces_exactly_the_quantised_matrices():
    t = R.synth_named("v6-small")
    q = S.prequantise(t, 2)
    names = {f"blocks.{l}.{n}" for l in range(2) for n in R.quantised_matrix_names(6)}
    for k in t:
        same = np.array_equal(np.asarray(t[k]), np.asarray(q[k]))
        assert same != (k in names), k
    for k in names:
        assert q[k].dtype == np.float16 and np.array_equal(q[k], S.fake_quant_sf4(t[k]))
    # the SF4 model is neither the NF4 model nor the plain one
    k = "blocks.0.att.key.weight"
    assert not np.array_equal(q[k], R.fake_quant(np.asarray(t[k], np.float16), R.QUANT_NF4))


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def test_planner_gives_sf4_the_plan_of_nf4_on_every_recorded_nf4_launch(tmp_path):
    exe = str(tmp_path / "gemm_plan_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "gemm_plan_test.cpp"), "-o", exe])
    lines = [line for d, (line, _) in P.fixture_cases() if d["engine"].split("/")[1] == "nf4"]
    assert len(lines) >= 300

    def as_sf4(line):
        w = line.split()
        n = int(w[7])
        assert len(w) == 8 + 6 * n
        for i in range(n):
            if w[8 + 6 * i + 2] == "2":
                w[8 + 6 * i + 2] = "3"
        return " ".join(w)
    sf4 = [as_sf4(l) for l in lines]
    assert sum(a != b for a, b in zip(lines, sf4)) >= 300             # the launches do carry NF4 problems
    run = lambda ls: subprocess.run([exe], input="\n".join(ls) + "\n", capture_output=True, text=True, timeout=60)
    a, b = run(lines), run(sf4)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    pa, pb = a.stdout.splitlines(), b.stdout.splitlines()
    assert len(pa) == len(lines) == len(pb)
    differ = [(l, x, y) for l, x, y in zip(lines, pa, pb) if x != y]
    assert not differ, differ[:5]
    assert len({x.split()[0] for x in pa}) >= 2 and len({x.split()[1] for x in pa if x.startswith("tile")}) >= 3   # decode and tile launches, several shapes


# ---- the constant across the public surfaces ------------------------------------------------------------------------------------------
def test_sf4_is_3_on_every_public_surface():
    from ai00_server_amd import runtime as rt
    assert int(rt.Quant.SF4) == 3 == S.QUANT_SF4 == SC.SF4
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    assert re.search(r"RWKV_QUANT_SF4\s*=\s*3\b", read("include", "rwkv_abi.h"))
    assert re.search(r"SF4\s*=\s*RWKV_QUANT_SF4\b", read("include", "rwkv_runtime.hpp"))
    assert re.search(r"pub const RWKV_QUANT_SF4: i32 = 3;", read("integration", "rwkv-hip-sys", "src", "lib.rs"))
    assert re.search(r"pub enum QuantType \{[^}]*\bSF4 = 3\b", read("integration", "rwkv-hip", "src", "lib.rs"))
    assert re.search(r"Quant::SF4 => QuantType::SF4", read("integration", "rwkv-hip", "src", "compat.rs"))
    assert re.search(r"W_SF4 = 3\b", read("ai00_server_amd", "csrc", "rwkv_kernels.h"))
    # the kernels' byte table and the loader's float table are the golden ones
    t32, bits = S.golden()
    src = read("ai00_server_amd", "csrc", "rwkv_kernels.hip")
    m = re.search(r"nf4_f16_bits\[32\] = \{([^}]*)\}", src)
    words = [int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]{4})", m.group(1))]
    assert words[:16] == R.NF4_TABLE_F16.view(np.uint16).tolist() and words[16:] == bits.tolist()
    m = re.search(r"kSf4Table\[16\] = \{([^}]*)\}", src)
    assert np.array_equal(np.array([float(x) for x in re.findall(r"(-?\d+\.\d+)f", m.group(1))], np.float64).astype(np.float32), t32)


# ---- the case table is exact ----------------------------------------------------------------------------------------------------------
def representable(v):
    return np.array_equal(v.astype(np.float32).astype(np.float64), v)


def test_case_table_is_exact_and_uses_every_code_and_every_column(datas):
    assert {c.group for c in CASES} == set(SC.GROUPS)
    cols = set()
    for c in CASES:
        d = datas[c.name]
        x = d["xhi"].astype(np.float64) + (d["xlo"].astype(np.float64) if c.hilo else 0.0)
        assert ((x != 0).sum(axis=1) == 1).all() and len(set(d["perm"])) == c.T
        for i, p in enumerate(c.probs):
            W = d["W"][i]
            assert p.rows == 48 and p.K == 512 and W.shape == (48, 512)
            if p.fmt != SC.F16:
                q, am = S.quant_sf4(W) if p.fmt == SC.SF4 else R.quant_nf4(W)
                assert len(np.unique(q)) == 16, (c.name, i)
                assert (am == 0).any() and (np.log2(am[am > 0].astype(np.float64)) % 1 != 0).any(), c.name   # zero blocks; scales that are no powers of two
                assert (np.ptp(W.reshape(48, 8, 64), axis=2) == 0).any()                                       # constant blocks
            want = SC.fake_quant(p, W).astype(np.float64)[:, d["perm"]].T * x[np.arange(c.T), d["perm"]][:, None]
            assert np.array_equal(SC.reference(c, d, i), want) and representable(want), (c.name, i)
        if c.group == "onehot" and c.mode == 2 and c.T == 64:
            cols |= set(d["perm"].tolist())
    assert cols == set(range(512)), "the decode launches of the family read back every column"
    assert {c.lo_mode for c in CASES if c.group == "onehot"} == {"hi", "lo", "both"}
    assert {(c.tile_shape, c.T, c.hilo) for c in CASES if c.group == "onehot" and c.mode == 1} == {(4, 257, False), (7, 193, False), (11, 256, False), (12, 256, True)}


def test_mixed_cases_tell_the_two_code_books_apart(datas):
    mixed = [c for c in CASES if c.group == "mixed"]
    assert [(c.T, c.hilo, c.mode) for c in mixed] == [(20, True, 2), (193, False, 1)]
    for c in mixed:
        d = datas[c.name]
        assert [p.fmt for p in c.probs] == [SC.F16, SC.NF4, SC.SF4] and d["W"][1] is d["W"][2]
        assert np.array_equal(SC.fake_quant(c.probs[0], d["W"][0]), d["W"][0])
        a, b = SC.reference(c, d, 1), SC.reference(c, d, 2)
        assert (a != b).mean() > 0.5, c.name                          # the same raw weights through the other table: most outputs differ
        # NF4's side of the launch is the oracle's NF4, bit for bit
        assert np.array_equal(SC.fake_quant(c.probs[1], d["W"][1]), R.dequant_nf4(*R.quant_nf4(d["W"][1])))


def test_checker_accepts_a_correct_result_and_names_a_damaged_one(datas):
    plan = lambda c: {"status": "ran", "path": "decode" if c.mode == 2 else "tile", "shape": c.tile_shape if c.mode == 1 else -1, "hilo": int(c.hilo), "fmts": [p.fmt for p in c.probs]}
    plans = [plan(c) for c in CASES]
    assert SC.coverage_gaps(CASES, plans) == []
    assert SC.coverage_gaps(CASES[:-1], plans[:-1]) == [] and SC.coverage_gaps([c for c in CASES if c.tile_shape != 7], [p for c, p in zip(CASES, plans) if c.tile_shape != 7])
    for c in CASES:
        d = datas[c.name]
        good = SC.emulate(c, d)
        assert SC.check_case(c, d, good, plan(c)) == [], c.name
    c = next(c for c in CASES if c.group == "mixed")
    d = datas[c.name]
    # an SF4 problem run through NF4's table is found
    as_nf4 = SC.emulate(c, d)
    p = c.probs[2]
    body = as_nf4["out"][SC.IO.GUARD:SC.IO.GUARD + c.T * c.ldo].reshape(c.T, c.ldo)
    body[:, p.ocol:p.ocol + p.rows] = SC.reference(c, d, 1).astype(np.float32).view(np.uint32)
    msgs = SC.check_case(c, d, as_nf4, plan(c))
    assert len(msgs) == 1 and "problem 2 (sf4" in msgs[0]
    # a write outside the launch's columns, a damaged payload byte and a written guard band are found
    bad = SC.emulate(c, d)
    bad["out"][SC.IO.GUARD + c.probs[0].rows + 1] = 0
    bad["pay2"][SC.IO.GUARD + 5] ^= 0x0100
    bad["sc1"][-3] = 0
    msgs = SC.check_case(c, d, bad, plan(c))
    assert len(msgs) == 3 and any("outside what the launch owns" in m for m in msgs) and any("payload differs in 1 bytes" in m for m in msgs) and any("guard band of sc1" in m for m in msgs)


def test_case_file_round_trips(tmp_path, datas):
    path = str(tmp_path / "cases.bin")
    cs = [c for c in CASES if c.group == "mixed"]
    SC.write_cases(path, cs, [datas[c.name] for c in cs])
    back = SC.IO.read_cases(path, SC.MAGIC)
    assert [b[0] for b in back] == [c.name for c in cs]
    for c, (name, kind, par, bufs) in zip(cs, back):
        assert kind == 0 and par[:8] == (c.T, int(c.hilo), c.mode, c.force_spb, c.tile_shape, 3, c.ldx, c.ldo) and len(par) == 20
        assert [r for r, *_ in bufs] == [SC.ROLE_INDEX[b.role] for b in datas[c.name]["bufs"]]

"""CPU: the row / WKV / state probe's table proved without a GPU (tests/row_cases.py, DESIGN.md "Row and recurrence probe").

  * the exact grids: on every exact WKV case an fp32 restatement equals the float64 reference in every bit of the state, in two orders —
    token by token with sequential sums, and the packed form (V5 / V6: two tokens folded into one update; V7: pairwise tree sums);
  * every case is well conditioned: a plain fp32 numpy restatement (numpy's own summation order, partial slabs added in reverse) passes the
    very checks the GPU results face, and its worst error / bound per group is printed (`-s`) for DESIGN.md;
  * the checks can fail: a dropped token, a doubled token, a write to an unowned row and a swapped predecessor are each reported;
  * the table reaches every kernel it exists for, from the launcher arguments alone;
  * the probe compiles for gfx950."""
import os

import numpy as np
import pytest

from tests import row_cases as R

CASES = R.all_cases()
F32, F64 = np.float32, np.float64
_DATA = {}


def data(c):
    if c.name not in _DATA:
        _DATA[c.name] = R.make(c)
    return _DATA[c.name]


def test_the_table_reaches_every_kernel():
    lines = [R.plan_line(c) for c in CASES]
    assert R.coverage_gaps(lines) == []
    assert len(R.twins(CASES)) >= 4                                  # V5, V6 at both Dd, V7: the same data through CH = 8 and CH = 32
    for short, long_ in R.twins(CASES):
        assert R.kernel_of(R.plan_line(short)).endswith(",8>") and R.kernel_of(R.plan_line(long_)).endswith(",32>")
    # without any case of a group the proof must fail: it is a statement about the table, not a constant
    assert R.coverage_gaps([l for l in lines if l["launcher"] != "embed"])


def test_layout_leaves_unowned_rows_and_slots():
    for c in CASES:
        if c.kind in (R.K_WKV, R.K_WKV4):
            own = R.rows_of(c.o["seqs"])
            assert len(set(own)) == len(own) and len(own) < c.p["T"] and c.p["T"] % 16 != 0
            assert 2 not in [s for s, _, _ in c.o["seqs"]] or c.p["dense"]
            d = data(c)
            assert np.isnan(d["r"][[t for t in range(c.p["T"]) if t not in own]]).all() and np.isfinite(d["r"][own]).all()


@pytest.mark.parametrize("ver", [5, 6, 7])
def test_exact_grids_are_exact_in_fp32_in_two_orders(ver):
    n = 0
    for c in CASES:
        if c.kind != R.K_WKV or c.p["version"] != ver or not c.o["exact"]:
            continue
        d = data(c)
        own = R.rows_of(d["seqs"])
        if ver == 6:                                                # every row sum of the decay LoRA is in [0, 60] (w = 1) or in [205, 280] (w = 0)
            sums = d["td"][own].astype(F64) @ d["D2"].astype(F64).T
            assert (((sums >= 0) & (sums <= 60)) | ((sums >= 205) & (sums <= 280))).all() and (sums <= 60).any() and (sums >= 205).any()
            w32 = np.exp(-np.exp(F32(-200.0) + sums.astype(F32)))
            assert ((w32 == 0) | (w32 == 1)).all() and w32.dtype == F32
        if ver == 7:                                                # kappa = +-1/2 on four channels, or 0 on all 64 (the k == 0 token)
            kk = (d["k"][own] * d["k_k"]).reshape(len(own), -1, 64)
            nz = (kk != 0).sum(-1)
            assert set(np.unique(nz)) <= {0, 4} and (nz == 0).any()
            kn = kk / np.maximum(np.sqrt((kk * kk).sum(-1, dtype=F32, keepdims=True)), F32(1e-12))
            assert set(np.unique(np.abs(kn))) <= {0.0, 0.5}
        st64, _ = R.wkv_eval(c, d, F64)
        used = [s for s, _, _ in d["seqs"]]
        assert (st64[used].astype(F32).astype(F64) == st64[used]).all(), c.name
        for order in (0, 1):
            st32, _ = R.wkv_eval(c, d, F32, order)
            assert st32.dtype == F32
            assert (st32[used].astype(F64) == st64[used]).all(), f"{c.name}: order {order}"
        n += 1
    assert n >= 8


@pytest.mark.parametrize("group", R.GROUPS)
def test_fp32_restatement_passes_the_gpu_checks(group):
    ratios = []
    for c in CASES:
        if c.group != group:
            continue
        d = data(c)
        msgs = R.check_case(c, d, R.emulate(c, d, F32), R.plan_line(c), ratios)
        assert not msgs, "\n".join(msgs[:8])
        if group in ("ln_shift_512", "ln_shift_1024"):
            _DATA.pop(c.name)                                       # the wide ones are tens of megabytes
    if group != "state_pack":
        worst = max(ratios, key=lambda r: r[2])
        print(f"fp32 restatement, worst error / bound in {group}: {worst[2]:.4f} ({worst[1]})")
        assert worst[2] <= 1.0


def test_wkv4_cases_are_what_they_claim():
    for c in CASES:
        if c.kind != R.K_WKV4:
            continue
        d, C = data(c), c.p["C"]
        own = R.rows_of(d["seqs"])
        used = [s for s, _, _ in d["seqs"]]
        assert np.abs(d["k"][own]).max() >= 25.0                    # |k| up to several tens
        assert (d["state"][used, 2 * C] == F32(-1e30)).any() and (d["state"][used, 2 * C] > -100).any()      # fresh slots and running maxima
        assert d["wdec"].max() >= -0.01 and d["wdec"].min() <= -5.0  # wide decays
        for nm in ("k", "u", "wdec"):                                # the 2^-10 grid that makes pp + w and u + k exact
            v = d[nm][own] if nm == "k" else d[nm]
            assert (v * 1024 == np.round(v * 1024)).all()
        _, y64 = R.wkv4_eval(c, d, F64)
        assert (y64[own] > 65504).any() and (y64[own] < -65504).any() or len(own) == 4 and np.abs(y64[own]).max() > 65504


def _first(pred):
    return next(c for c in CASES if pred(c))


def test_the_checks_can_fail():
    # a token applied twice / dropped in an exact case: one k v^T too many or too few in one head's state
    for ver in (5, 7):
        c = _first(lambda c: c.kind == R.K_WKV and c.p["version"] == ver and c.o["exact"] and c.name.endswith("long_9-1-32-33_exact"))
        d = data(c)
        res = R.emulate(c, d, F32)
        slot, b, n = d["seqs"][2]
        H = c.p["H"]
        st = res["state"][R.GUARD:-R.GUARD].reshape(R.NSLOTS, -1)[slot, :H * 4096].view(F32).reshape(H, 64, 64)
        kv = np.outer(d["v"][b + n - 1, :64], d["k"][b + n - 1, :64])
        assert kv.any()
        for sign in (1, -1):
            bad = {k: v.copy() for k, v in res.items()}
            w = bad["state"][R.GUARD:-R.GUARD].reshape(R.NSLOTS, -1)
            w[slot, :4096] = R.bits((st[0] + sign * kv).astype(F32))
            msgs = R.check_case(c, d, bad, R.plan_line(c))
            assert any("exact grid" in m for m in msgs)
    # a y row written for a row of no sequence, a state tile of a slot outside the step, a guard band
    c = _first(lambda c: c.kind == R.K_WKV and not c.o["exact"])
    d = data(c)
    res = R.emulate(c, d, F32)
    for role, at in (("yhi", R.GUARD), ("state", R.GUARD + 2 * c.p["slot_stride"] + 5), ("state", R.GUARD + c.p["H"] * 4096 + 1), ("yhi", 3)):
        bad = {k: v.copy() for k, v in res.items()}
        bad[role][at] = 0
        assert R.check_case(c, d, bad, R.plan_line(c)), (role, at)
    # ln_shift: rows 65 and 66 swapped (what a banded numbering that is no bijection does to a step of 67 rows); one bit of x_out
    c = _first(lambda c: c.name == "ln_shift_c64_t67")
    d = data(c)
    res = R.emulate(c, d, F32)
    C = c.p["C"]
    for role in ("xx", "x_out"):
        if c.o[role]:
            bad = {k: v.copy() for k, v in res.items()}
            rows = bad[role][R.GUARD:-R.GUARD].reshape(-1, C)
            rows[[65, 66]] = rows[[66, 65]]
            assert R.check_case(c, d, bad, R.plan_line(c))
    assert c.o["x_out"]
    bad = {k: v.copy() for k, v in res.items()}
    bad["x_out"][R.GUARD + 11] ^= 1
    assert R.check_case(c, d, bad, R.plan_line(c))
    # state_pack: two elements exchanged
    c = _first(lambda c: c.kind == R.K_STATE_PACK and c.p["to_slab"] == 1)
    d = data(c)
    bad = {k: v.copy() for k, v in R.emulate(c, d).items()}
    s = bad["slab"][R.GUARD:-R.GUARD]
    s[[200, 201]] = s[[201, 200]]
    assert R.check_case(c, d, bad, R.plan_line(c))


def test_state_pack_round_trip_is_the_identity_of_the_table():
    pairs = 0
    for c in CASES:
        if c.kind == R.K_STATE_PACK and c.p["to_slab"] == 0:
            twin = _first(lambda t: t.kind == R.K_STATE_PACK and t.p["to_slab"] == 1 and t.o["seed"] == c.o["seed"])
            a, b = data(c), data(twin)
            assert (R.bits(a["slab"]) == R.bits(b["slab"])).all() and all((R.bits(x) == R.bits(y)).all() for x, y in zip(a["internal"], b["internal"]))
            which, src = R.sp_perm(c.p)
            for k in range(3):                                      # a permutation: no internal element is the image of two slab elements
                assert len(set(src[which == k].tolist())) == int((which == k).sum())
            pairs += 1
    assert pairs == 6


def test_write_then_read_round_trip(tmp_path):
    cases = [c for c in CASES if c.group == "embed_ln_out"][:3]
    datas = [data(c) for c in cases]
    R.write_cases(str(tmp_path / "cases.bin"), cases, datas)
    assert (tmp_path / "cases.bin").stat().st_size > 0
    with open(tmp_path / "results.bin", "wb") as f:
        for c, d in zip(cases, datas):
            res = R.emulate(c, d, F32)
            for b in d["bufs"]:
                if b.flags & 1:
                    f.write(res[b.role].tobytes())
    for c, d, res in zip(cases, datas, R.read_results(str(tmp_path / "results.bin"), cases, datas)):
        assert not R.check_case(c, d, res, R.plan_line(c))


def test_probe_compiles_for_gfx950(tmp_path):
    obj = R.compile_probe(tmp_path)
    assert os.path.getsize(obj) > 0

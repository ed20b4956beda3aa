"""The case table of tests/cpp/sf4_probe.hip, shared by tests/test_gpu_sf4.py (runs the probe on the GPU) and tests/test_sf4_cpu.py (proves the
table without one).  The one-hot family of tests/gemm_cases.py with W_SF4 problems: ARBITRARY fp16 weights, token t is one power of two at one
column, so the output row is fake_quant(W)[:, column] * x exactly — one product per output, nothing to sum, no tolerance.  The generators, the
operand and payload layouts and the Case / Prob records are those of tests/gemm_cases.py; what dispatches on the format there through the
oracle (which does not know SF4) is restated here over tests/sf4_ref.py.  A plain module, no fixtures."""
import numpy as np

from oracle import rwkv_ref as R
from tests import gemm_cases as G
from tests import probe_io as IO
from tests import sf4_ref as S

F16, NF4, SF4 = G.F16, G.NF4, 3
FMT_NAME = {F16: "f16", NF4: "nf4", SF4: "sf4"}
MAGIC = 0x42344653
ROLES = ["xhi", "xlo", "out", "w0", "w1", "w2", "pay0", "pay1", "pay2", "sc0", "sc1", "sc2"]
ROLE_INDEX = {r: i for i, r in enumerate(ROLES)}
ROWS, K = 48, 512
GROUPS = ("quant", "onehot", "mixed")


def cases():
    out = [G.Case("sf4-quant-bytes", "quant", 1, [G.Prob(ROWS, K, SF4)], mode=2, family="onehot", lo_mode="hi")]
    modes = ("hi", "lo", "both")
    for j in range(8):                                                # 8 x 64 tokens = every column of K = 512 (perm start differs per case)
        lm = modes[j % 3]
        out.append(G.Case(f"sf4-onehot-dec{j}-{lm}", "onehot", 64, [G.Prob(ROWS, K, SF4)], hilo=lm != "hi", mode=2, family="onehot", lo_mode=lm, perm_base=64 * j))
    out.append(G.Case("sf4-onehot-T1", "onehot", 1, [G.Prob(ROWS, K, SF4)], mode=2, family="onehot", lo_mode="hi"))
    # one forced tile shape per tile kind (gemm_plan.h kTileShapes): chunked through registers, chunked by LDS DMA, pipelined, pipelined hi + lo
    out.append(G.Case("sf4-onehot-tile4", "onehot", 257, [G.Prob(ROWS, K, SF4)], mode=1, tile_shape=4, ksplit=1, family="onehot", lo_mode="hi"))
    out.append(G.Case("sf4-onehot-tile7", "onehot", 193, [G.Prob(ROWS, K, SF4)], mode=1, tile_shape=7, ksplit=1, family="onehot", lo_mode="hi"))
    out.append(G.Case("sf4-onehot-tile11", "onehot", 256, [G.Prob(ROWS, K, SF4)], mode=1, tile_shape=11, ksplit=1, family="onehot", lo_mode="hi"))
    out.append(G.Case("sf4-onehot-tile12", "onehot", 256, [G.Prob(ROWS, K, SF4)], hilo=True, mode=1, tile_shape=12, ksplit=1, family="onehot", lo_mode="both", perm_base=256))
    # one launch, three code paths: an fp16 problem on the integer lattice, and the SAME raw weights once as NF4 and once as SF4
    three = lambda: [G.Prob(ROWS, K, F16), G.Prob(ROWS, K, NF4), G.Prob(ROWS, K, SF4)]
    out.append(G.Case("sf4-mixed-dec-T20-hilo", "mixed", 20, three(), hilo=True, mode=2, family="onehot", lo_mode="both", perm_base=100))
    out.append(G.Case("sf4-mixed-tile11-T193", "mixed", 193, three(), mode=1, tile_shape=11, ksplit=1, family="onehot", lo_mode="hi", perm_base=300))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return [c.layout() for c in out]


def fake_quant(p, W):
    return {F16: lambda w: w, NF4: lambda w: R.fake_quant(w, R.QUANT_NF4), SF4: S.fake_quant_sf4}[p.fmt](W)


def expected_payload(p, W):
    """(payload bytes, scale bytes) the load-time kernel must write: SF4 is tiled as NF4 is (gemm_cases.tiled_nf4)."""
    if p.fmt == F16:
        return G.tiled_f16(W).view(np.uint8), np.zeros(0, np.uint8)
    pay, sc = G.tiled_nf4(*(S.quant_sf4(W) if p.fmt == SF4 else R.quant_nf4(W)))
    return pay.view(np.uint8), sc.view(np.uint8)


def payload_sizes(p):
    n = p.rows * p.K
    return (n * 2, 0) if p.fmt == F16 else (n // 2, p.rows * (p.K // 64) * 2)


def make(case):
    """The inputs of gemm_cases.make (one-hot X, arbitrary weights); a mixed case's fp16 problem gets lattice weights and its NF4 and SF4
    problems share one raw matrix.  d["bufs"]: the probe's role buffers."""
    d = G.make(case)
    if len(case.probs) == 3:
        rng = np.random.default_rng(G.seed_of(case) + 1)
        d["W"][0] = G.lattice_weights(rng, case.probs[0])
        d["W"][2] = d["W"][1]
    bufs = [IO.b_in("xhi", G.padded_x(case, d["xhi"]))]
    if case.hilo:
        bufs.append(IO.b_in("xlo", G.padded_x(case, d["xlo"])))
    bufs.append(IO.b_out("out", case.T * case.ldo, 4))
    for i, (p, W) in enumerate(zip(case.probs, d["W"])):
        nb, ns = payload_sizes(p)
        bufs.append(IO.b_in(f"w{i}", np.ascontiguousarray(W)))
        bufs.append(IO.b_out(f"pay{i}", nb // 2, 2))
        if ns:
            bufs.append(IO.b_out(f"sc{i}", ns // 2, 2))
    d["bufs"] = bufs
    return d


class _Params:
    """The probe's parameter vector of a case, in its order, for probe_io.write_cases."""
    def __init__(self, case):
        self.name, self.kind = case.name, 0
        vals = [case.T, int(case.hilo), case.mode, case.force_spb, case.tile_shape, len(case.probs), case.ldx, case.ldo]
        for p in case.probs:
            vals += [p.rows, p.K, p.fmt, p.ocol]
        self.p = dict(enumerate(vals))


def write_cases(path, cases_, datas):
    IO.write_cases(path, MAGIC, [_Params(c) for c in cases_], datas, lambda c: sorted(c.p), ROLE_INDEX)


def read_results(path, cases_, datas):
    return IO.read_results(path, cases_, datas)


def reference(case, d, i):
    """[T][rows] of problem i, fp64."""
    p = case.probs[i]
    x = d["xhi"].astype(np.float64) + (d["xlo"].astype(np.float64) if case.hilo else 0.0)
    return x[:, :p.K] @ fake_quant(p, d["W"][i]).astype(np.float64).T


def emulate(case, d):
    """What a correct probe run returns, built from the reference (the CPU test runs check_case on it, and on a damaged copy)."""
    res = IO.untouched(d)
    out = res["out"].copy()
    body = out[IO.GUARD:IO.GUARD + case.T * case.ldo].reshape(case.T, case.ldo)
    for i, p in enumerate(case.probs):
        body[:, p.ocol:p.ocol + p.rows] = reference(case, d, i).astype(np.float32).view(np.uint32)
        pay, sc = expected_payload(p, d["W"][i])
        for role, a in ((f"pay{i}", pay), (f"sc{i}", sc)):
            if a.size:
                r = res[role].copy()
                r[IO.GUARD:IO.GUARD + a.size // 2] = a.view(np.uint16)
                res[role] = r
    res["out"] = out
    return res


def check_case(case, d, res, plan):
    """Every failure of one case as a list of messages (empty: the case passed)."""
    if plan.get("status") != "ran":
        return [f"{case.name}: the probe did not run the case: {plan}"]
    msgs = []
    bufs = {b.role: b for b in d["bufs"]}
    for role, b in bufs.items():
        if b.flags & 1:
            a, s = res[role], IO.SENT[b.esize]
            if (a[:IO.GUARD] != s).any() or (a[-IO.GUARD:] != s).any():
                msgs.append(f"{case.name}: a guard band of {role} was written; plan {plan}")
    for i, p in enumerate(case.probs):
        pay, sc = expected_payload(p, d["W"][i])
        got = IO.own(res, bufs[f"pay{i}"]).view(np.uint8)
        if not np.array_equal(got, pay):
            msgs.append(f"{case.name}: problem {i} ({FMT_NAME[p.fmt]}): tiled payload differs in {int((got != pay).sum())} bytes of {pay.size}")
        if sc.size:
            got = IO.own(res, bufs[f"sc{i}"]).view(np.uint8)
            if not np.array_equal(got, sc):
                msgs.append(f"{case.name}: problem {i} ({FMT_NAME[p.fmt]}): scales differ in {int((got != sc).sum())} bytes of {sc.size}")
    body = IO.own(res, bufs["out"]).reshape(case.T, case.ldo)
    owned = np.zeros(body.shape, bool)
    for i, p in enumerate(case.probs):
        owned[:, p.ocol:p.ocol + p.rows] = True
        got = body[:, p.ocol:p.ocol + p.rows].view(np.float32).astype(np.float64)
        want = reference(case, d, i)
        bad = ~(got == want)                                            # NaN never equals: a sentinel left in a valid output is a difference
        if bad.any():
            first = [f"(t {t}, row {r}, column {int(d['perm'][t])}, got {got[t, r]!r}, want {want[t, r]!r})" for t, r in np.argwhere(bad)[:4]]
            msgs.append(f"{case.name}: problem {i} ({FMT_NAME[p.fmt]} {p.rows}x{p.K}): {int(bad.sum())} of {got.size} outputs differ: {' '.join(first)}; plan {plan}")
    stray = ~owned & (body != IO.SENT32)
    if stray.any():
        msgs.append(f"{case.name}: {int(stray.sum())} fp32 elements outside what the launch owns were written, first (t, column) {np.argwhere(stray)[:4].tolist()}; plan {plan}")
    return msgs


def coverage_gaps(cases_, plans):
    """[] or what the plan lines do not show: every case ran on the path it was built for, every tile kind and the decode kernel ran."""
    gaps = []
    kinds = set()
    for c, p in zip(cases_, plans):
        want = "decode" if c.mode == 2 else "tile"
        if p.get("status") != "ran" or p.get("path") != want:
            gaps.append(f"{c.name}: planned {p}")
            continue
        if c.mode == 1:
            if p["shape"] != c.tile_shape or p["hilo"] != int(c.hilo):
                gaps.append(f"{c.name}: shape {p['shape']} hilo {p['hilo']}")
            if SF4 in p["fmts"]:
                kinds.add(G.TILE_KIND[p["shape"]])
        if p["fmts"] != [q.fmt for q in c.probs]:
            gaps.append(f"{c.name}: formats {p['fmts']}")
    if kinds != {0, 1, 2, 3}:
        gaps.append(f"tile kinds that ran an SF4 problem: {sorted(kinds)}")
    dec = [(c, p) for c, p in zip(cases_, plans) if c.mode == 2 and p.get("path") == "decode"]
    if {(c.T, int(c.hilo)) for c, _ in dec} < {(1, 0), (64, 0), (64, 1), (20, 1)}:
        gaps.append("decode step sizes")
    return gaps

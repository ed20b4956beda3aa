"""The mix / prologue / commit probe's case table, shared by tests/test_gpu_mix_exact.py (runs tests/cpp/mix_probe.hip on the GPU) and
tests/test_mix_cases_cpu.py (proves the table without one): one launch per case (DESIGN.md "Mix, prologue and commit probe").

What a launch computes:  z [T][C] (an f16 hi (+ lo) operand, or built by the LayerNorm prologue: xx = LN(x_in + P[0] + ..), prev = sx[slot],
z = xx + (prev - xx) mu_x, dx = prev - xx);  phase 1  m_c = tanh(W1_c z), W1 = [5 Dm][C];  phase 2  o_c = W2_c m_c, W2_c = [C][Dm];
out_c = xx + dx (mu_c + o_c), written as an f16 hi (+ lo) operand [ceil16(T)][ldh].  The hi-only forms round m (and the prologue's z) to f16.

  lattice   every output BIT FOR BIT.  tanh is exact only at 0 and in saturation, so phase 1 lands there: a 32-k step holds sixteen pairs of
            columns (p, 16 + p); a token owns the pairs of its class (t % 16, or t % T below 16 rows), z is non-zero only there with
            z[p] - z[16 + p] = rho_t u (u = 1/4 with hi + lo operands, 1 without; rho_t = +-1), and W1 carries (q n, -q n) on ONE owned pair per
            (row, k-step, class) (q = 64 / 16): the step contributes 16 n rho_t exactly, n = +-1 alternating over the k-steps plus one +-2 so
            that the whole sum is 16 eps rho_t, eps in {-1, 0, +1} per (row, class).  Every step matters: removing or doubling any k-step moves
            some sum of every (mix, strip, token tile) across 0 or +-16, and so does any slice of K on every fourth row, whose steps add up
            over 256-k chunks instead of cancelling (proved by enumeration, lattice_proof).  m = eps rho_t in {-1, 0, 1};
            W2 holds small integers, mu / xx / dx quarters: the lerp is exact in fp32, fused or not.
  general   random values against float64 numpy from the same input bits at the project's Fp32 bound 2e-5 * max(1, |ref|), plus, in the hi-only
            forms, the tie budget of the rounded entries (tie_budget).

A plain module, no fixtures."""
import json
import os
import subprocess
import zlib
from dataclasses import dataclass, field

import numpy as np

from tests.gemm_cases import F16 as W_F16, Prob, lattice_weights, pack_opd, split_hilo, unpack_opd   # the operand layout and the carrier's lattice: stated once, there
from tests.probe_io import GUARD, SENT16, SENT32, b_in, b_out, bits, read_results, write_cases as write_case_file   # the container: stated once, there
from tests.row_cases import Checker, ceil16, ew_bound, f16_sat, ln_eval, nan32, ulp16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
K_MIX, K_COMMIT, K_PAIR = range(3)
KIND_NAME = ("mix", "commit", "pair")
PARAMS = ("T", "C", "Dm", "hilo", "ldz", "ldh", "lnp", "np", "pstride", "sx_slot_stride", "dense", "nslots", "ksp_min_t", "ksp_blocks", "ksp_max",
          "Dd", "commit_C", "carrier_hilo", "ldo")
_ROLES = (["W1"] + [f"W2_{i}" for i in range(5)] + ["zhi", "zlo", "xx", "dx"] + [f"mu{i}" for i in range(5)] + ["mu_x"] + [f"ohi{i}" for i in range(5)]
          + [f"olo{i}" for i in range(5)] + ["mg_hi", "mg_lo", "mp", "x_in", "x_out", "P", "lnw", "lnb", "sx", "slot", "prev", "last", "xx_out"]
          + [f"cW{i}" for i in range(5)] + [f"cout{i}" for i in range(5)] + ["src"])
ROLE = {n: i for i, n in enumerate(_ROLES)}                        # the Role enum of mix_probe.hip
GROUPS = ("mix_decode", "mix_lnp", "mix_wide", "mix_split", "mix_ksliced", "commit")
NSLOTS, SLOT = 5, 3                                                # non-dense cases: the step's one row belongs to slot 3 of 5
NP_ALLOC = 5                                                       # slabs of P a prologue case allocates: those beyond np hold the pattern
CARRIER_ACT = ("none", "none", "none", "silu", "tanh")             # Wk, Wv, Wr, Wg, D1 (rwkv_engine.cpp, the V6 att launch)
CARRIER_MIX = (1, 2, 3, 4, 0)                                      # which mix operand (w, k, v, r, g) each of them reads
HEADROOM = 1 << 20
# tau: 8 x the largest absolute difference between the float64 pre-rounding value (m; TAU_Z: the prologue form's z) and the fp32 restatement of it in
# two summation orders, over the hi-only general cases of a group, rounded up to two digits (tie_budget says why it is absolute).  The prologue
# group's m is measured with the rounded z held fixed: what a flipped z does to m is in the budget by itself.  tests/test_mix_cases_cpu.py measures
# all of them again: the measurement must lie inside, and no further below than the rounding (a tau that only grew would widen the bound).
TAU = {"mix_decode": 3.8e-6, "mix_lnp": 2.7e-6, "mix_wide": 4.2e-6, "mix_split": 4.6e-6, "mix_ksliced": 4.7e-6, "commit": 0.0}
TAU_Z = 4.5e-6
BOUND_CAP = 10.0                                                   # base bound + tie budget <= 10 x base bound on every element (checked on the CPU)


@dataclass
class Case:
    name: str
    group: str
    kind: int
    p: dict
    o: dict = field(default_factory=dict)                          # family, which scratch buffers exist, row metadata

    @property
    def lattice(self):
        return self.o["family"] == "lattice"


def seed_of(case):
    return zlib.crc32(case.name.encode())


# ------------------------------------------------------------------------------------------------
# the launcher's rules, transcribed once (rwkv_kernels.hip v6_mix_split, launch_v6_mix); the probe prints what the product's own functions give
# ------------------------------------------------------------------------------------------------
def v6_split(T, C, hilo, has_mg_hi, has_mg_lo, has_mp, ksp_min_t, ksp_blocks, ksp_max):
    if T <= 32 or T % 32:
        return 0
    ntile = T // 32
    if has_mp and ksp_min_t <= T < 512:
        per_wave, best = (C >> 5) >> 3, 1
        for q in range(1, min(per_wave, ksp_max) + 1):
            if per_wave % q:
                continue
            best = q
            if 5 * ntile * q >= ksp_blocks:
                break
        if best > 1:
            return best
    return 1 if T >= 512 and has_mg_hi and (not hilo or has_mg_lo) else 0


def mix_rule(c):
    """form, NT, split, ksp, both grids, the apply launch's token tiles — and what the kernels derive from them (kst, KB)."""
    P, o = c.p, c.o
    T, C, Dm, hilo = P["T"], P["C"], P["Dm"], bool(P["hilo"])
    groups = (C // 16 + 7) // 8
    r = dict(form="decode", NT=1 if T <= 16 else 2, split=0, ksp=1, grid1=[groups, 5, 1], grid2=[0, 0], apply_nt=0)
    if T <= 32:
        r["form"] = "lnp" if P["lnp"] else "decode"
    else:
        ntile = (T + 31) // 32
        r["NT"] = 2
        r["split"] = v6_split(T, C, hilo, o.get("mg_hi", False), o.get("mg_lo", False), o.get("mp", 0) > 0, P["ksp_min_t"], P["ksp_blocks"], P["ksp_max"])
        if r["split"]:
            nt1 = groups * ntile < 256
            r.update(form="split", ksp=r["split"], grid1=[r["split"], 5, ntile], apply_nt=1 if nt1 else 2, grid2=[groups, (T + 15) // 16 if nt1 else ntile])
        else:
            r.update(form="wide", grid1=[max(1, min(8, 256 // (5 * ntile))), 5, ntile])
    DS = Dm // 16
    r["KB"] = (5 if hilo and r["NT"] == 2 else 10) if DS == 2 else 4
    r["kst"] = ((C >> 5) >> 3) // r["ksp"]
    return r


def plan_line(c, carrier=None):
    """The JSON line the probe prints for the case.  `carrier`: the carrier's plan object (carrier_plans) of a commit / pair case."""
    line = {"case": c.name, "kind": KIND_NAME[c.kind], **{k: int(c.p[k]) for k in PARAMS}}
    if c.kind != K_COMMIT:
        r = mix_rule(c)
        line.update({k: r[k] for k in ("form", "NT", "split", "ksp", "grid1", "grid2", "apply_nt")})
    if c.kind != K_MIX:
        line["carrier"] = carrier
        line["launch_grid"] = carrier["total_blocks"] + 1
    return line


def build_planner(out_dir):
    exe = os.path.join(str(out_dir), "mix_plan_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "mix_plan_test.cpp"), "-o", exe])
    return exe


def carrier_plans(exe, cases):
    """{case name: the carrier's plan} from the engine's planner on the CPU (tests/cpp/mix_plan_test.cpp)."""
    cc = [c for c in cases if c.kind != K_MIX]
    out = subprocess.run([exe], input="".join(f"{c.p['T']} {c.p['carrier_hilo']} {c.p['C']} {c.p['Dd']}\n" for c in cc), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    plans = [json.loads(l) for l in out.stdout.splitlines()]
    assert len(plans) == len(cc)
    return {c.name: p for c, p in zip(cc, plans)}


def compile_probe(out_dir):
    from ai00_server_amd import build as B
    return B.compile_probe("mix_probe", os.path.join(str(out_dir), "mix_probe.o"))


def build_probe():
    from ai00_server_amd import build as B
    return B.build_probe("mix_probe", verbose=False)


def write_cases(path, cases, datas):
    return write_case_file(path, 0x4252504D, cases, datas, lambda c: PARAMS, ROLE)


# ------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------
def rn16(x):
    """Round to f16 and back (values inside the f16 range)."""
    return np.asarray(x).astype(np.float16).astype(np.asarray(x).dtype)


def quarters(rng, shape, lo, hi):
    return (rng.integers(int(lo * 4), int(hi * 4) + 1, shape) / 4.0).astype(F32)


def _lattice_w1_z(rng, T, C, Dm, hilo):
    """(W1 [5 Dm][C] f16, z hi, z lo [T][C] f16, eps [G][5 Dm], rho [T]) of the saturated lattice."""
    KT, G, R = C // 32, min(16, T), 5 * Dm
    q = 64.0 if hilo else 16.0
    g, row, j = np.meshgrid(np.arange(G), np.arange(R), np.arange(KT), indexing="ij")
    cc, d = row // Dm, row % Dm
    eps = (((row * 7 + g * 3 + cc) % 5) % 3 - 1)                     # [G][R][KT], the same along j: -1, 0, +1
    sig = 1 - 2 * ((j + d + g) % 2)
    j0 = (3 * d + 5 * g + cc) % KT
    j0 = np.where(sig[np.arange(G)[:, None, None], row, j0] == eps, j0, (j0 + 1) % KT)        # a k-step whose sign is eps's
    n = np.where((eps != 0) & (j == j0), 2 * eps, sig)
    # every fourth row works on whole SLICES of K instead (alternating steps cancel inside any slice): one step per 256-k chunk carries +1, the last
    # chunk's -(chunks - 1): the sum is 0, and the sum of any aligned run of chunks that is not all of them is not
    nch = KT // 8
    if nch > 1:
        chunk = j // 8
        slow = (d % 4 == 3)
        at = j % 8 == (d + g + chunk) % 8
        n = np.where(slow, np.where(at, np.where(chunk == nch - 1, -(nch - 1), 1), 0), n)
        eps = np.where(slow, 0, eps)
    owned = [np.flatnonzero(np.arange(16) % G == k) for k in range(G)]
    pstar = np.empty((G, R, KT), int)
    for k in range(G):
        pstar[k] = owned[k][(j[k] + d[k] + cc[k]) % len(owned[k])]
    W1 = np.zeros((R, KT, 32), F64)
    W1[row, j, pstar] = q * n
    W1[row, j, 16 + pstar] = -q * n
    # z: class t % 16 % G, non-zero on the owned pairs only, z[p] - z[16 + p] = rho u
    rho = rng.choice([-1.0, 1.0], T)
    u = 0.25 if hilo else 1.0
    zb = rng.integers(-12, 13, (T, KT, 16)) / 4.0 if hilo else rng.integers(-3, 4, (T, KT, 16)).astype(F64)
    cls = (np.arange(T) % 16) % G
    own = (np.arange(16)[None, :] % G) == cls[:, None]               # [T][16]
    z = np.zeros((T, KT, 32), F64)
    z[:, :, :16] = np.where(own[:, None, :], zb + rho[:, None, None] * u, 0.0)
    z[:, :, 16:] = np.where(own[:, None, :], zb, 0.0)
    z = z.reshape(T, C)
    if hilo:                                                          # to the kernel lo is a second operand: deliberately not tiny
        hi = np.where(z != 0, np.round(z) + rng.integers(-1, 2, z.shape), 0.0)
        lo = z - hi
    else:
        hi, lo = z, np.zeros_like(z)
    return W1.reshape(R, C).astype(np.float16), hi.astype(np.float16), lo.astype(np.float16), eps[:, :, 0], rho


def make_mix(c):
    """Inputs and buffers of a mix (or pair) case."""
    P, o = c.p, c.o
    rng = np.random.default_rng(seed_of(c))
    T, C, Dm, hilo, lnp = P["T"], P["C"], P["Dm"], bool(P["hilo"]), bool(P["lnp"])
    T16, d = ceil16(T), {}
    if c.lattice:
        W1, zhi, zlo, d["eps"], d["rho"] = _lattice_w1_z(rng, T, C, Dm, hilo)
        W2 = [rng.integers(-2, 3, (C, Dm)).astype(np.float16) for _ in range(5)]
        mu = [quarters(rng, C, 0, 1) for _ in range(5)]
        xx, dx = quarters(rng, (T, C), -4, 4), quarters(rng, (T, C), -2, 2)
        if o.get("modest"):                                           # the pair case: what the carrier reads stays inside its own headroom
            W2 = [rng.integers(-1, 2, (C, Dm)).astype(np.float16) for _ in range(5)]
            xx, dx = quarters(rng, (T, C), -2, 2), quarters(rng, (T, C), -1, 1)
        elif not lnp:                                                 # beyond the f16 range, both signs
            xx[T // 2, 5], dx[T // 2, 5] = 70000.0, 0.0
            xx[T - 1, C - 3], dx[T - 1, C - 3] = -70000.0, 0.0
    else:
        W1 = (rng.normal(0, 1.0, (5 * Dm, C)) / np.sqrt(C)).astype(np.float16)
        W2 = [rng.uniform(-0.03, 0.03, (C, Dm)).astype(np.float16) for _ in range(5)]
        mu = [rng.uniform(0, 1, C).astype(F32) for _ in range(5)]
        zhi, zlo = split_hilo(rng.normal(0, 1, (T, C)).astype(F32))
        xx, dx = rng.normal(0, 1, (T, C)).astype(F32), rng.normal(0, 0.7, (T, C)).astype(F32)
        dx[0, 1], xx[0, 1] = 0.0, 70000.0
    d["W1"], d["W2"], d["mu"] = W1, W2, mu
    bufs = [b_in("W1", W1)] + [b_in(f"W2_{i}", W2[i]) for i in range(5)] + [b_in(f"mu{i}", mu[i]) for i in range(5)]
    if not lnp:
        d["zhi"], d["zlo"], d["xx"], d["dx"] = zhi, (zlo if hilo else None), xx, dx

        def padded(x):                                                # rows T .. and columns C .. hold NaN halfs: nothing of them may reach an output
            full = np.full((T16, P["ldz"]), SENT16, np.uint16)
            full[:T, :C] = x.view(np.uint16)
            return pack_opd(full)
        bufs += [b_in("zhi", padded(zhi))] + ([b_in("zlo", padded(zlo))] if hilo else []) + [b_in("xx", xx), b_in("dx", dx)]
    else:
        npar, dense = P["np"], bool(P["dense"])
        slot = 0 if dense else SLOT
        d["slot"] = slot
        d["x_in"] = (rng.normal(0, 1, (T, C)) + rng.normal(0, 0.5, (T, 1))).astype(F32)
        Pb = nan32((NP_ALLOC, P["pstride"]))
        Pb[:npar, :T * C] = rng.normal(0, 0.3, (npar, T * C))
        d["P"] = Pb
        sx = nan32((P["nslots"], P["sx_slot_stride"]))
        if c.lattice:                                                 # lnw = 0: xx = lnb whatever the statistics round to; z = the lattice's z exactly
            z = zhi.astype(F32)[0]
            mux = rng.choice([0.0, 0.5, 1.0], C).astype(F32)
            other = quarters(rng, C, -3, 3) if not o.get("modest") else quarters(rng, C, -1, 1)
            delta = quarters(rng, C, -2, 2) if not o.get("modest") else quarters(rng, C, -1, 1)
            lnb = np.where(mux == 0, z, np.where(mux == 1, other, z + delta)).astype(F32)
            sx[slot, :C] = np.where(mux == 0, other, np.where(mux == 1, z, z - delta))
            d["lnw"], d["lnb"], d["mu_x"] = np.zeros(C, F32), lnb, mux
        else:
            d["lnw"], d["lnb"], d["mu_x"] = rng.uniform(0.5, 1.5, C).astype(F32), rng.normal(0, 0.1, C).astype(F32), rng.uniform(0.1, 1, C).astype(F32)
            sx[slot, :C] = rng.normal(0, 1, C)
            # a z that flips in its f16 rounding moves EVERY m of the row by |W1| ulp(z), a good part of m's own f16 step, and the tie budget has to
            # assume the worst of all of them together: the state is chosen so that no z lies within 4 tau_z of a tie or below 1/8 (tie_budget)
            x = d["x_in"].copy()
            for j in range(npar):
                x = x + Pb[j, :T * C].reshape(T, C)
            xx = ln_eval(x.astype(F64), d["lnw"].astype(F64), d["lnb"].astype(F64), F64)[0]
            for _ in range(16):
                z = xx + (sx[slot, :C].astype(F64) - xx) * d["mu_x"].astype(F64)
                small, tie = np.abs(z) < 0.125, _tie_distance(z) < 4 * TAU_Z
                if not (small | tie).any():
                    break
                step = np.where(small, np.where(z < 0, -0.25, 0.25), np.where(tie, ulp16(z) / 4, 0.0))
                sx[slot, :C] = (sx[slot, :C].astype(F64) + step / d["mu_x"].astype(F64)).astype(F32)
        d["sx"] = sx
        bufs += [b_in("x_in", d["x_in"]), b_out("x_out", T * C, 4), b_in("P", Pb), b_in("lnw", d["lnw"]), b_in("lnb", d["lnb"]), b_in("mu_x", d["mu_x"]),
                 b_in("sx", sx, back=True), b_out("xx_out", T * C, 4)]
        if not dense:
            bufs += [b_in("slot", np.full(T, slot, np.int32)), b_in("prev", np.full(T, -1, np.int32))]
    for i in range(5):
        bufs.append(b_out(f"ohi{i}", T16 * P["ldh"], 2))
        if hilo:
            bufs.append(b_out(f"olo{i}", T16 * P["ldh"], 2))
    if o.get("mg_hi"):
        bufs.append(b_out("mg_hi", 5 * T * Dm, 2))
    if o.get("mg_lo"):
        bufs.append(b_out("mg_lo", 5 * T * Dm, 2))
    if o.get("mp", 0):
        bufs.append(b_out("mp", o["mp"] * 5 * T * Dm, 4))
    d["bufs"] = bufs
    return d


def add_carrier(c, d):
    """The carrier's weights and outputs, the commit's metadata; a commit case's own operands and source."""
    P, o = c.p, c.o
    rng = np.random.default_rng(seed_of(c) ^ 0x5A5A)
    T, C, Dd, CC, ch = P["T"], P["C"], P["Dd"], P["commit_C"], bool(P["carrier_hilo"])
    d["cW"] = [lattice_weights(rng, Prob(Dd if i == 4 else C, C, W_F16), small=True) for i in range(5)]
    bufs = [b_in(f"cW{i}", d["cW"][i]) for i in range(5)] + [b_out(f"cout{i}", T * P["ldo"], 4) for i in range(5)]
    dense = bool(P["dense"])
    d["cslot"] = np.arange(T, dtype=np.int32) if dense else np.full(T, SLOT, np.int32)
    d["clast"] = np.arange(T, dtype=np.int32) if dense else np.full(T, o.get("last", 0), np.int32)
    if c.kind == K_COMMIT:
        T16 = ceil16(T)
        d["chi"] = [(rng.integers(-1, 2, (T, C)) / 8.0).astype(np.float16) for _ in range(5)]       # the GEMM probe's `act` lattice: two problems end in a transcendental
        d["clo"] = [(rng.integers(-1, 2, (T, C)) / 32.0).astype(np.float16) for _ in range(5)] if ch else None

        def padded(x):
            full = np.full((T16, P["ldh"]), SENT16, np.uint16)
            full[:T, :C] = x.view(np.uint16)
            return pack_opd(full)
        bufs += [b_in(f"ohi{i}", padded(d["chi"][i]), back=True) for i in range(5)]
        if ch:
            bufs += [b_in(f"olo{i}", padded(d["clo"][i]), back=True) for i in range(5)]
        d["src"] = rng.normal(0, 1, (T, CC)).astype(F32)
        sx = nan32((P["nslots"], P["sx_slot_stride"]))
        bufs += [b_in("src", d["src"]), b_in("sx", sx, back=True)]
        d["sx"] = sx
    if not dense:
        have = {b.role for b in d.get("bufs", [])}
        bufs += [b_in("slot", d["cslot"])] if "slot" not in have else []
        bufs.append(b_in("last", d["clast"]))
    d["bufs"] = d.get("bufs", []) + bufs
    return d


def make(c):
    d = make_mix(c) if c.kind != K_COMMIT else {}
    return add_carrier(c, d) if c.kind != K_MIX else d


# ------------------------------------------------------------------------------------------------
# the computation, in float64 (the reference) or restated in fp32 in two summation orders, optionally with one mistake
# ------------------------------------------------------------------------------------------------
# One mistake each, stated as the kernel would make it and applied to EVERY case: which cases it reaches falls out of running it
#   tail_kstep       the last k-step of a batch that is not full is dropped (a wave's kst k-steps go in batches of KB)
#   slice_twice      `q0 + j <= ksp` in the five-at-a-time sum of the slice partials, whose loads are clamped to slice ksp - 1
#   prev_slot0       the prologue shifts from slot 0's state
#   commit_row_slot  the commit writes slot t, not slot[t]
#   skip_strips      the wide form's strip walk stops after its first round
#   tile16_index     the whole-K apply launch finds its m tile as if token tiles always had 32 rows
MUTATIONS = ("tail_kstep", "slice_twice", "prev_slot0", "commit_row_slot", "skip_strips", "tile16_index")


def _seq_sum(x, axis, rev):
    """Sequential sum along `axis` in x's dtype, ascending or descending."""
    idx = range(x.shape[axis])
    acc = np.zeros(np.delete(x.shape, axis), x.dtype)
    for i in (reversed(idx) if rev else idx):
        acc = acc + np.take(x, i, axis)
    return acc


def evaluate(c, d, ft=F64, order=0, fused=False, mut=None, z_from=None):
    """Everything a mix launch produces, as arrays of dtype `ft` (F64: the reference).  order 1 reverses every sum; fused: the lerp as one fma;
    z_from: the prologue's rounded z taken from another evaluation (to measure phase 1 on its own)."""
    P = c.p
    T, C, Dm, hilo = P["T"], P["C"], P["Dm"], bool(P["hilo"])
    r = mix_rule(c)
    rev = order == 1
    ev = {"rule": r}
    if P["lnp"]:
        x = d["x_in"].copy()
        for j in range(P["np"]):                                      # fp32, slab order: the bit-exact reference of x_out
            x = x + d["P"][j, :T * C].reshape(T, C)
        ev["x_out"] = x
        xs = x.astype(ft)
        if rev:                                                       # the other order: statistics from the reversed row
            xx = ln_eval(xs[:, ::-1], d["lnw"].astype(ft)[::-1], d["lnb"].astype(ft)[::-1], ft)[:, ::-1]
        else:
            xx = ln_eval(xs, d["lnw"].astype(ft), d["lnb"].astype(ft), ft)
        slot = 0 if mut == "prev_slot0" else d["slot"]
        prev = d["sx"][slot, :C].astype(ft)[None, :]
        dx = prev - xx
        zpre = xx + dx * d["mu_x"].astype(ft)
        with np.errstate(invalid="ignore"):
            z = rn16(f16_sat(zpre)) if z_from is None else z_from.astype(ft)
        ev.update(xx_out=xx, zpre=zpre)
    else:
        z = d["zhi"].astype(ft) + (d["zlo"].astype(ft) if hilo else 0)
        xx, dx = d["xx"].astype(ft), d["dx"].astype(ft)
    ev["z"] = z
    # ---- phase 1: per 32-k step, then per wave (kst steps), then the 8 waves of a slice, then the slices
    KT, ksp, kst, R = C // 32, r["ksp"], r["kst"], 5 * Dm
    W1 = d["W1"].astype(ft).reshape(R, KT, 32)
    ks = np.matmul(np.ascontiguousarray(z.reshape(T, KT, 32).transpose(1, 0, 2)), np.ascontiguousarray(W1.transpose(1, 2, 0)))      # [KT][T][R]
    ev["ksteps"] = ks
    ks = ks.reshape(ksp, 8, kst, T, R)
    if mut == "tail_kstep":
        KB = r["KB"]
        ks = ks[:, :, [k0 + j for k0 in range(0, kst, KB) for j in range(min(KB, kst - k0) - (kst - k0 < KB))]]
    mp = _seq_sum(_seq_sum(ks, 2, rev), 1, rev)                        # [ksp][T][R]
    ev["mp"] = mp
    s = _seq_sum(mp, 0, rev)
    if mut == "slice_twice" and ksp > 1:                               # the apply kernel's loop over the slice partials, five loads at a time
        s = np.zeros_like(mp[0])
        for q0 in range(0, ksp, 5):
            for j in range(5):
                if q0 + j <= ksp:
                    s = s + mp[min(q0 + j, ksp - 1)]
    with np.errstate(invalid="ignore"):
        mpre = np.tanh(s)                                             # [T][R]
    ev["mpre"] = mpre
    if hilo:
        if ft is F64 and not c.lattice:
            m = mpre
        else:                                                         # what the kernel keeps: the fp32 tanh as hi + lo (on the lattice exactly +-1 or 0: 1 - tanh(16) = 2.5e-14)
            h, l = split_hilo(mpre)
            m = h.astype(ft) + l.astype(ft)
    else:
        m = rn16(mpre)
    ev["m"] = m
    if mut == "tile16_index" and r["form"] == "split" and ksp == 1:
        t, rows = np.arange(T), 16 * r["apply_nt"]                    # the block of token tile t / rows reads the rows of m behind tile * 32
        m = m[((t // rows) * 32 + t % rows) % T]
    # ---- phase 2 and the lerp
    out = []
    for i in range(5):
        W2 = d["W2"][i].astype(ft).reshape(C, Dm // 32, 32)
        mi = m[:, i * Dm:(i + 1) * Dm].reshape(T, Dm // 32, 32)
        o = _seq_sum(np.einsum("tjd,rjd->jtr", mi, W2), 0, rev)
        a = d["mu"][i].astype(ft)[None, :] + o
        if fused and ft is F32:
            v = (xx.astype(F64) + dx.astype(F64) * a.astype(F64)).astype(F32)
        else:
            v = xx + dx * a
        out.append(v)
    ev["out"] = out
    ev["dx"] = dx
    if mut == "skip_strips" and r["form"] == "wide":
        ev["skip_from"] = 8 * r["grid1"][0] * 16                     # a round is 8 strips per block of grid.x: the columns of later rounds are never written
    return ev


def _tie_distance(v):
    """Absolute distance of every value to the nearest f16 rounding tie (the midpoint between two neighbouring f16 values)."""
    u = ulp16(v)
    return np.abs(v / u - np.floor(v / u) - 0.5) * u


def tie_budget(c, d, ev, tau, tau_z):
    """[5][T][C]: the first-order effect on each output of a one-step flip of every rounded m within tau of an f16 rounding tie (hi-only forms).
    tau is an ABSOLUTE distance (8 x the largest |float64 - fp32 restatement| of the pre-rounding values): relative to the value it has no bound at
    entries near zero, where a flip is worth nothing anyway — such an entry always counts as near a tie and costs its own tiny step.
    The prologue form rounds z first, and a flipped z moves every m of the row by |W1| ulp16(z), a good part of m's own step: no useful budget
    covers that, so the general prologue cases keep every z at least tau_z from a tie (make_mix), and a case that does not is refused here."""
    P = c.p
    T, C, Dm = P["T"], P["C"], P["Dm"]
    if P["hilo"]:
        return [np.zeros((T, C)) for _ in range(5)]
    if P["lnp"]:
        assert (_tie_distance(ev["zpre"]) >= tau_z).all(), f"{c.name}: a z of the prologue lies within tau_z of an f16 rounding tie"
    mpre = ev["mpre"]
    dm = (_tie_distance(mpre) < tau) * ulp16(mpre)
    return [np.abs(ev["dx"]) * (dm[:, i * Dm:(i + 1) * Dm] @ np.abs(d["W2"][i].astype(F64)).T) for i in range(5)]


def rounding_distance(c, d, ev64, ev32):
    """Largest absolute difference between the float64 pre-rounding values and a restatement's: (m, z)."""
    dm = float(np.max(np.abs(ev64["mpre"] - ev32["mpre"].astype(F64))))
    dz = float(np.max(np.abs(ev64["zpre"] - ev32["zpre"].astype(F64)))) if c.p["lnp"] else 0.0
    return dm, dz


def carrier_ref(c, d, x_hi, x_lo):
    """float64 outputs [5][T][rows] of the carrier from operand values [5][T][C]."""
    outs = []
    for i in range(5):
        x = x_hi[CARRIER_MIX[i]].astype(F64) + (x_lo[CARRIER_MIX[i]].astype(F64) if x_lo is not None else 0.0)
        v = x @ d["cW"][i].astype(F64).T
        outs.append(v / (1.0 + np.exp(-v)) if CARRIER_ACT[i] == "silu" else np.tanh(v) if CARRIER_ACT[i] == "tanh" else v)
    return outs


# ------------------------------------------------------------------------------------------------
# a correct launch's result buffers (and a mistaken one's), and the checks
# ------------------------------------------------------------------------------------------------
def emulate(c, d, ft=F32, order=0, fused=False, mut=None):
    """The result buffers of the restatement in `ft`: what check_case must accept (mut: with one of MUTATIONS, which it must report wherever the
    mistake changes a buffer)."""
    P = c.p
    T, C, Dm, hilo = P["T"], P["C"], P["Dm"], bool(P["hilo"])
    res = {}
    for b in d["bufs"]:
        if b.flags & 1:
            res[b.role] = (np.full(b.n + 2 * GUARD, SENT32 if b.esize == 4 else SENT16, np.uint32 if b.esize == 4 else np.uint16) if b.flags & 2 else b.image.copy())
    pay = lambda role: res[role][GUARD:-GUARD]
    T16 = ceil16(T)
    ohi = olo = None
    if c.kind != K_COMMIT:
        ev = evaluate(c, d, ft, order, fused, mut)
        r = ev["rule"]
        ohi, olo = [], []
        for i in range(5):
            h, l = split_hilo(ev["out"][i].astype(F32))
            ohi.append(h), olo.append(l)
            ncol = min(C, ev.get("skip_from", C))
            for role, part in ((f"ohi{i}", h), (f"olo{i}", l)):
                if role in res:
                    a = unpack_opd(pay(role).copy(), T16, P["ldh"])
                    a[:T, :ncol] = part.view(np.uint16)[:, :ncol]
                    pay(role)[:] = pack_opd(a)
        if r["form"] == "split":
            if r["ksp"] > 1:
                pay("mp")[:r["ksp"] * 5 * T * Dm] = bits(np.ascontiguousarray(ev["mp"].astype(F32).reshape(r["ksp"], T, 5, Dm).transpose(0, 2, 1, 3)))
            else:
                h, l = split_hilo(ev["mpre"].astype(F32))
                pay("mg_hi")[:] = bits(np.ascontiguousarray(h.reshape(T, 5, Dm).transpose(1, 0, 2)))
                if hilo:
                    pay("mg_lo")[:] = bits(np.ascontiguousarray(l.reshape(T, 5, Dm).transpose(1, 0, 2)))
        if P["lnp"]:
            pay("x_out")[:] = bits(ev["x_out"])
            pay("xx_out")[:] = bits(ev["xx_out"].astype(F32))
    if c.kind != K_MIX:
        CC = P["commit_C"]
        if c.kind == K_PAIR:
            xh, xl, src = ohi, None, ev["xx_out"].astype(F32)
        else:
            xh, xl, src = d["chi"], d["clo"], d["src"]
        for i, v in enumerate(carrier_ref(c, d, xh, xl)):
            a = pay(f"cout{i}").reshape(T, P["ldo"])
            a[:, :v.shape[1]] = bits(v.astype(F32)).reshape(v.shape)
        sx = pay("sx").reshape(P["nslots"], -1)
        for t in range(T):
            if d["clast"][t] >= 0:
                sx[t if mut == "commit_row_slot" else d["cslot"][t], :CC] = bits(src[d["clast"][t]])
    return res


def _opd_exact(ck, what, res, role, T, ld, C, want16):
    """An operand [ceil16(T)][ld] bit for bit: rows < T, columns < C hold want16's bits, everything else the pattern."""
    T16 = ceil16(T)
    exp = np.full((T16, ld), SENT16, np.uint16)
    exp[:T, :C] = want16.view(np.uint16)
    ck.same_bits(what, unpack_opd(res[role][GUARD:-GUARD], T16, ld), exp)


def check_case(c, d, res, line, ratios=None, carrier=None):
    """[] or messages; appends (group, case, worst error / bound) to ratios."""
    ck = Checker(c, ratios)
    P = c.p
    T, C, Dm, hilo = P["T"], P["C"], P["Dm"], bool(P["hilo"])
    want_line = plan_line(c, carrier if carrier is not None else line.get("carrier"))
    if line != want_line:
        ck.msgs.append(f"{c.name}: the probe printed {line}, the table says {want_line}")
    ck.guards(res)
    ohi_bits = None
    if c.kind != K_COMMIT:
        ev = evaluate(c, d, F64)
        r = ev["rule"]
        budget = None if c.lattice else tie_budget(c, d, ev, TAU[c.group], TAU_Z)
        for i in range(5):
            want = ev["out"][i]
            if c.lattice:
                assert np.array_equal(want, want.astype(F32)), "lattice outputs are fp32 values"
                h, l = split_hilo(want.astype(F32))
                _opd_exact(ck, f"mix {i} hi (lattice)", res, f"ohi{i}", T, P["ldh"], C, h)
                if hilo:
                    _opd_exact(ck, f"mix {i} lo (lattice)", res, f"olo{i}", T, P["ldh"], C, l)
            else:
                ck.operand(f"mix {i}", res, f"ohi{i}", f"olo{i}" if hilo else None, T, P["ldh"], {t: t for t in range(T)}, C, want, ew_bound(f16_sat(want)) + budget[i])
        if c.kind == K_PAIR:
            ohi_bits = [unpack_opd(res[f"ohi{i}"][GUARD:-GUARD], ceil16(T), P["ldh"])[:T, :C].view(np.float16) for i in range(5)]
        # scratch: used by the split form, whole otherwise
        used_mp = r["ksp"] * 5 * T * Dm if r["form"] == "split" and r["ksp"] > 1 else 0
        if "mp" in res:
            body = res["mp"][GUARD:-GUARD]
            ck.same_bits("mp beyond the slices of the launch", body[used_mp:], np.full(body.size - used_mp, SENT32, np.uint32))
            if used_mp:
                got = body[:used_mp].view(F32).reshape(r["ksp"], 5, T, Dm).astype(F64)
                want = ev["mp"].reshape(r["ksp"], T, 5, Dm).transpose(0, 2, 1, 3)
                for q in range(r["ksp"]):
                    if c.lattice:
                        ck.exact(f"mp slice {q} (k {q * C // r['ksp']}..{(q + 1) * C // r['ksp'] - 1})", got[q].astype(F32), want[q])
                    else:
                        ck.close(f"mp slice {q}", got[q], want[q], ew_bound(want[q]))
        whole_k = r["form"] == "split" and r["ksp"] == 1
        mpre = ev["mpre"].reshape(T, 5, Dm).transpose(1, 0, 2)
        for role in ("mg_hi", "mg_lo"):
            if role not in res:
                continue
            body = res[role][GUARD:-GUARD]
            if not whole_k or (role == "mg_lo" and not hilo):
                ck.same_bits(f"{role}, not used by the {r['form']} form", body, np.full(body.size, SENT16, np.uint16))
            elif c.lattice:
                h, l = split_hilo(mpre.astype(F32))
                ck.same_bits(f"{role} (lattice)", body, bits(np.ascontiguousarray(h if role == "mg_hi" else l)))
        if whole_k and not c.lattice:
            gh = res["mg_hi"][GUARD:-GUARD].view(np.float16).reshape(5, T, Dm).astype(F64)
            ck.close("mg_hi", gh, mpre, ew_bound(mpre), 0.5 * ulp16(mpre))
            if hilo:
                ck.close("mg_hi + mg_lo", gh + res["mg_lo"][GUARD:-GUARD].view(np.float16).reshape(5, T, Dm).astype(F64), mpre, ew_bound(mpre))
        if P["lnp"]:
            ck.same_bits("x_out against the fp32 sum in the order j = 0 .. np-1", res["x_out"][GUARD:-GUARD], bits(ev["x_out"]))
            got = res["xx_out"][GUARD:-GUARD].view(F32).reshape(T, C)
            if c.lattice:
                ck.exact("xx_out (lattice: lnb)", got, ev["xx_out"])
            else:
                ck.close("xx_out", got.astype(F64), ev["xx_out"], ew_bound(ev["xx_out"]))
            if c.kind == K_MIX:
                ck.same_bits("sx (the prologue reads it, the commit writes it)", res["sx"], b_in("sx", d["sx"]).image)
    if c.kind != K_MIX:
        CC = P["commit_C"]
        if c.kind == K_PAIR:
            xh, xl, src = ohi_bits, None, res["xx_out"][GUARD:-GUARD].view(F32).reshape(T, CC)
        else:
            xh, xl, src = d["chi"], d["clo"], d["src"]
            for i in range(5):                                        # the carrier's operands are inputs
                for role in (f"ohi{i}",) + ((f"olo{i}",) if xl is not None else ()):
                    ck.same_bits(f"{role} (an input)", res[role], next(b for b in d["bufs"] if b.role == role).image)
        with np.errstate(all="ignore"):
            wants = carrier_ref(c, d, xh, xl)
        for i, want in enumerate(wants):
            body = res[f"cout{i}"][GUARD:-GUARD].reshape(T, P["ldo"])
            rows = want.shape[1]
            ck.same_bits(f"carrier output {i}, columns beyond its rows", body[:, rows:], np.full((T, P["ldo"] - rows), SENT32, np.uint32))
            got = body[:, :rows].view(F32)
            if CARRIER_ACT[i] == "none":
                ck.exact(f"carrier output {i}", got, want)
            else:
                ck.close(f"carrier output {i} ({CARRIER_ACT[i]})", got.astype(F64), want, ew_bound(want))
        exp = bits(d["sx"]).reshape(P["nslots"], -1).copy()
        for t in range(T):
            if d["clast"][t] >= 0:
                exp[d["cslot"][t], :CC] = bits(src[d["clast"][t]])
        ck.same_bits("sx after the commit (the committed slot is the source row, everything else holds the pattern)", res["sx"][GUARD:-GUARD].reshape(P["nslots"], -1), exp)
    if ratios is not None:
        ratios.append((c.group, c.name, ck.worst))
    return ck.msgs


# ------------------------------------------------------------------------------------------------
# proofs that need no GPU (tests/test_mix_cases_cpu.py)
# ------------------------------------------------------------------------------------------------
def lattice_proof(c, d):
    """[] or what the lattice does not deliver: headroom, saturation, and the sensitivity of every (mix, W1 strip, 16-token tile, 32-k step)."""
    P = c.p
    T, C, Dm, hilo = P["T"], P["C"], P["Dm"], bool(P["hilo"])
    ev = evaluate(c, d, F64)
    msgs = []
    z = ev["z"]
    quantum = 16.0
    if P["lnp"]:
        if not np.array_equal(ev["zpre"], ev["z"]) or not np.array_equal(ev["zpre"][0], d_z(c, d)):
            msgs.append("the prologue's z is not the lattice's z exactly")
        if not np.array_equal(ev["xx_out"][0], d["lnb"].astype(F64)):
            msgs.append("xx != lnb")
    absz = np.abs(d["zhi"].astype(F64)) + (np.abs(d["zlo"].astype(F64)) if hilo else 0) if not P["lnp"] else np.abs(z)
    head = float((absz @ np.abs(d["W1"].astype(F64)).T).max() / quantum)
    if not head < HEADROOM:
        msgs.append(f"phase 1 headroom {head}")
    ks = ev["ksteps"]                                                  # [KT][T][R]
    if (ks % 16).any():
        msgs.append("a k-step's contribution is no multiple of 16")
    S = ks.sum(0)
    if not np.isin(S, (-16.0, 0.0, 16.0)).all() or not np.array_equal(ev["mpre"].astype(F32), np.sign(S).astype(F32)):
        msgs.append("a phase-1 sum is not in {-16, 0, 16}, or the fp32 value nearest to tanh of it is not its sign")
    KT, R = C // 32, 5 * Dm
    sgn = np.sign(S)[None]
    gone = (np.sign(S[None] - ks) != sgn).reshape(KT, T, R // 16, 16)   # removing the step changes m here
    twice = (np.sign(S[None] + ks) != sgn).reshape(KT, T, R // 16, 16)  # doubling it does
    for what, ch in (("removing", gone), ("doubling", twice)):
        for t0 in range(0, T, 16):
            ok = ch[:, t0:t0 + 16].any(axis=(1, 3))                    # [KT][strip]
            if not ok.all():
                msgs.append(f"{what} a k-step changes no m of its tile: (k-step, strip) {np.argwhere(~ok)[:3].tolist()} at tokens {t0}..")
    ksp = ev["rule"]["ksp"]
    if ksp > 1:                                                       # the same for whole slices of K
        sl = ks.reshape(ksp, KT // ksp, T, R).sum(1)
        for what, ch in (("removing", np.sign(S[None] - sl) != sgn), ("doubling", np.sign(S[None] + sl) != sgn)):
            ch = ch.reshape(ksp, T, R // 16, 16)
            for t0 in range(0, T, 16):
                ok = ch[:, t0:t0 + 16].any(axis=(1, 3))
                if not ok.all():
                    msgs.append(f"{what} a K slice changes no m of its tile: (slice, strip) {np.argwhere(~ok)[:3].tolist()} at tokens {t0}..")
    # phase 2: exact in fp32 whatever the order, and at least half of the per-k-step partial sums non-zero
    m = ev["m"]
    for i in range(5):
        W2 = d["W2"][i].astype(F64)
        mi = m[:, i * Dm:(i + 1) * Dm]
        part = np.einsum("tjd,rjd->jtr", mi.reshape(T, Dm // 32, 32), W2.reshape(C, Dm // 32, 32))
        for t0 in range(0, T, 16):
            nz = (part[:, t0:t0 + 16] != 0).reshape(Dm // 32, -1, C // 16, 16).mean(axis=(1, 3))
            if (nz < 0.5).any():
                msgs.append(f"mix {i}: fewer than half of the phase-2 partial sums of a (strip, token tile, k-step) are non-zero at tokens {t0}..")
        a = np.abs(d["mu"][i].astype(F64))[None] + np.abs(mi) @ np.abs(W2).T
        xx = np.abs(ev["xx_out"]) if P["lnp"] else np.abs(d["xx"].astype(F64))
        big = float(((np.abs(ev["dx"]) * a + xx) * 16).max())          # the lerp lives on sixteenths
        if not big < (1 << 23):
            msgs.append(f"mix {i}: lerp headroom {big}")
    return msgs


def d_z(c, d):
    """The lattice's z of a prologue case, rebuilt from the case alone."""
    _, zhi, _, _, _ = _lattice_w1_z(np.random.default_rng(seed_of(c)), c.p["T"], c.p["C"], c.p["Dm"], False)
    return zhi.astype(F64)[0]


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------
def _mix(name, group, T, C, Dm, hilo, family, lnp=False, npar=0, dense=True, mg=True, mp=2, pad=None, kind=K_MIX, **kw):
    i = zlib.crc32(name.encode())
    pad = (i % 3 != 0) if pad is None else pad                        # ldz, ldh > C in about two of three cases (and in at least one of every form: all_cases)
    ld = C + (64 if pad else 0)
    p = dict(T=T, C=C, Dm=Dm, hilo=int(hilo), ldz=0 if lnp else ld, ldh=C + (32 if pad else 0), lnp=int(lnp), np=npar, pstride=T * C + 96 if lnp else 0,
             sx_slot_stride=C + 64 if lnp else 0, dense=int(dense), nslots=NSLOTS if lnp else 0, ksp_min_t=192, ksp_blocks=kw.pop("ksp_blocks", 160),
             ksp_max=kw.pop("ksp_max", 16), Dd=0, commit_C=0, carrier_hilo=0, ldo=0)
    o = dict(family=family, mg_hi=bool(mg), mg_lo=bool(mg) and hilo and kw.pop("mg_lo", True), mp=mp, **kw)
    return Case(name, group, kind, p, o)


def _both(out, name, *a, **kw):
    for fam in ("lattice", "general"):
        out.append(_mix(f"{name}_{fam}", *a, family=fam, **kw))


def mix_cases():
    out = []
    hd = lambda hilo, Dm: f"{'hilo' if hilo else 'hi'}_dm{Dm}"
    # (1) decode form: every T edge, both Dm, both operand forms; (2) the batch tail of phase 1
    for T in (1, 15, 16, 17, 31, 32):
        for Dm in (32, 64):
            for hilo in (False, True):
                _both(out, f"dec_c256_t{T}_{hd(hilo, Dm)}", "mix_decode", T, 256, Dm, hilo)
    for C, T, Dm, hilo in ((1536, 5, 64, False), (1536, 20, 64, True), (1536, 20, 32, True), (2816, 3, 32, False)):
        _both(out, f"dec_tail_c{C}_t{T}_{hd(hilo, Dm)}", "mix_decode", T, C, Dm, hilo)
    # (3) prologue form
    for C, npar in ((256, 1), (2304, 3), (4096, 5)):
        for Dm in (32, 64):
            for dense in (True, False):
                _both(out, f"lnp_c{C}_np{npar}_dm{Dm}_{'dense' if dense else 'slot3'}", "mix_lnp", 1, C, Dm, False, lnp=True, npar=npar, dense=dense)
    # (4) - (7) wide form, one launch
    for T, (hilo, Dm) in zip((33, 48, 64, 65), ((False, 32), (True, 32), (False, 64), (True, 64))):
        _both(out, f"wide_c256_t{T}_{hd(hilo, Dm)}", "mix_wide", T, 256, Dm, hilo)
    for C, T in ((1536, 200), (512, 500)):
        for hilo, Dm in ((True, 64), (False, 32)):
            _both(out, f"wide_c{C}_t{T}_{hd(hilo, Dm)}", "mix_wide", T, C, Dm, hilo)
    _both(out, "wide_nosplit_t512_mg_null_hi_dm32", "mix_wide", 512, 256, 32, False, mg=False)
    _both(out, "wide_nosplit_t520_hilo_dm32", "mix_wide", 520, 256, 32, True)
    _both(out, "wide_nosplit_t192_mp_null_hi_dm64", "mix_wide", 192, 512, 64, False, mp=0)
    _both(out, "wide_nosplit_t192_ksp_max1_hilo_dm64", "mix_wide", 192, 512, 64, True, ksp_max=1)
    # (8) split, whole K
    for C in (256, 2048):
        for Dm in (32, 64):
            for hilo in (False, True):
                _both(out, f"split_c{C}_t512_{hd(hilo, Dm)}", "mix_split", 512, C, Dm, hilo, mp=1)
    # (9) split, K-sliced: (C, T) -> ksp
    forms = ((False, 32), (True, 64), (True, 32), (False, 64))
    for i, (C, T, ksp, blocks) in enumerate(((512, 192, 2, 160), (768, 256, 3, 160), (1280, 192, 5, 160), (1536, 192, 6, 160), (2048, 192, 8, 160), (4096, 192, 16, 100000))):
        hilo, Dm = forms[i % 4]
        _both(out, f"ksl_c{C}_t{T}_ksp{ksp}_{hd(hilo, Dm)}", "mix_ksliced", T, C, Dm, hilo, mp=ksp + 1, ksp_blocks=blocks, want_ksp=ksp)
    for hilo, Dm in forms:
        _both(out, f"ksl_c4096_t256_ksp4_{hd(hilo, Dm)}", "mix_ksliced", 256, 4096, Dm, hilo, mp=5, want_ksp=4)
    return out


def commit_cases():
    out = []

    def carrier(p, o, CC, ch, dense, last=0):
        p.update(Dd=64, commit_C=CC, carrier_hilo=int(ch), ldo=p["C"] + 8, dense=int(dense), nslots=NSLOTS, sx_slot_stride=CC + 64)
        o["last"] = last
    for name, ch, dense, CC, last in (("commit_dense_hi", False, True, 256, 0), ("commit_slot3_hi", False, False, 256, 0), ("commit_dense_hilo", True, True, 256, 0),
                                      ("commit_slot3_hilo", True, False, 256, 0), ("commit_slot3_last_none", False, False, 256, -1), ("commit_slot3_c4096", False, False, 4096, 0)):
        p = dict(T=1, C=256, Dm=32, hilo=0, ldz=0, ldh=256 + 32, lnp=0, np=0, pstride=0, sx_slot_stride=0, dense=0, nslots=0, ksp_min_t=192, ksp_blocks=160, ksp_max=16,
                 Dd=0, commit_C=0, carrier_hilo=0, ldo=0)
        o = dict(family="lattice")
        carrier(p, o, CC, ch, dense, last)
        out.append(Case(name, "commit", K_COMMIT, p, o))
    for dense in (True, False):
        c = _mix(f"pair_{'dense' if dense else 'slot3'}", "commit", 1, 256, 32, False, "lattice", lnp=True, npar=2, dense=dense, kind=K_PAIR, modest=True, pad=True)
        carrier(c.p, c.o, 256, False, dense)
        out.append(c)
    return out


def all_cases():
    cases = mix_cases() + commit_cases()
    assert len({c.name for c in cases}) == len(cases)
    assert {c.group for c in cases} == set(GROUPS)
    return cases


def coverage_gaps(lines):
    """[] or what of the coverage list of DESIGN.md "Mix, prologue and commit probe" the lines do not reach."""
    gaps = []
    mix = [l for l in lines if l["kind"] != "commit"]
    fam = lambda l: l["case"].rsplit("_", 1)[-1]
    need = lambda what, ok: None if ok else gaps.append(what)

    def both(what, sel):
        got = {fam(l) for l in mix if sel(l)}
        if not {"lattice", "general"} <= got and not what.startswith("pair"):
            gaps.append(f"{what}: families {sorted(got)}")
    for hilo in (0, 1):
        for Dm in (32, 64):
            for nt in (1, 2):
                both(f"v6_mix_kernel<{nt}, {hilo}, {Dm // 16}> decode", lambda l: (l["form"], l["NT"], l["hilo"], l["Dm"]) == ("decode", nt, hilo, Dm))
            both(f"v6_mix_kernel<2, {hilo}, {Dm // 16}, wide>", lambda l: (l["form"], l["hilo"], l["Dm"]) == ("wide", hilo, Dm))
            for sliced in (0, 1):
                both(f"v6_mix_kernel<2, {hilo}, {Dm // 16}, P1ONLY> sliced {sliced}", lambda l: l["form"] == "split" and (l["hilo"], l["Dm"], int(l["ksp"] > 1)) == (hilo, Dm, sliced))
                for ant in (1, 2):
                    both(f"v6_mix_apply_kernel<{hilo}, {Dm // 16}, {ant}> sliced {sliced}",
                         lambda l: l["form"] == "split" and (l["hilo"], l["Dm"], int(l["ksp"] > 1), l["apply_nt"]) == (hilo, Dm, sliced, ant))
    for Dm in (32, 64):
        for dense in (0, 1):
            both(f"v6_mix_kernel<1, 0, {Dm // 16}, LNP> dense {dense}", lambda l: (l["form"], l["Dm"], l["dense"]) == ("lnp", Dm, dense))
    dec = [l for l in mix if l["form"] == "decode"]
    need("decode T in {1, 15, 16, 17, 31, 32}", {1, 15, 16, 17, 31, 32} <= {l["T"] for l in dec})
    tails = {(l["C"], l["Dm"], l["hilo"], l["NT"]) for l in dec}
    need("decode batch tails 4 + 2, 5 + 1, 10 + 1", any(t[0] == 1536 and t[1] == 64 for t in tails) and (1536, 32, 1, 2) in tails and any(t[0] == 2816 and t[1] == 32 and not (t[2] and t[3] == 2) for t in tails))
    need("prologue (C, np) in {(256, 1), (2304, 3), (4096, 5)}", {(256, 1), (2304, 3), (4096, 5)} <= {(l["C"], l["np"]) for l in mix if l["form"] == "lnp"})
    wide = [l for l in mix if l["form"] == "wide"]
    need("wide T in {33, 48, 64, 65} with grid.x = 8", {33, 48, 64, 65} <= {l["T"] for l in wide if l["grid1"][0] == 8 and l["C"] == 256})
    need("wide grid.x = 7 in two rounds", any(l["grid1"][0] == 7 and l["C"] // 16 > 56 and l["T"] % 32 for l in wide))
    need("wide grid.x = 3 in rounds of unequal length", any(l["grid1"][0] == 3 and 24 < l["C"] // 16 < 48 for l in wide))
    need("steps that would split but must not", {512, 520, 192} <= {l["T"] for l in wide} and any(l["T"] == 192 and l["ksp_max"] == 1 for l in wide))
    need("whole-K split with the apply launch on 16- and on 32-token tiles", {1, 2} <= {l["apply_nt"] for l in mix if l["form"] == "split" and l["ksp"] == 1})
    ksl = {(l["C"], l["T"], l["ksp"]) for l in mix if l["form"] == "split" and l["ksp"] > 1}
    need("slice counts", {(512, 192, 2), (768, 256, 3), (1280, 192, 5), (1536, 192, 6), (2048, 192, 8), (4096, 192, 16), (4096, 256, 4)} <= ksl)
    need("ld > C in every form", all(any(l["ldh"] > l["C"] and (l["form"] == "lnp" or l["ldz"] > l["C"]) for l in mix if l["form"] == f) for f in ("decode", "lnp", "wide", "split")))
    com = [l for l in lines if l["kind"] != "mix"]
    need("commit dense / slot 3, hi-only / hi + lo", {(d, h) for d in (0, 1) for h in (0, 1)} <= {(l["dense"], l["carrier_hilo"]) for l in com if l["kind"] == "commit"})
    need("commit.C = 4096", any(l["commit_C"] == 4096 for l in com))
    need("pair dense and slot 3", {0, 1} <= {l["dense"] for l in com if l["kind"] == "pair"})
    need("the carrier stays on the decode kernel with one extra block", all(l["carrier"]["path"] == "decode" and l["carrier"]["smallk_without_commit"] == 1
                                                                          and l["launch_grid"] == l["carrier"]["total_blocks"] + 1 for l in com) and bool(com))
    return gaps

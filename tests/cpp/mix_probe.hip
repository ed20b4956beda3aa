// mix_probe.hip — stand-alone driver of the V6 mix kernels, the LayerNorm prologue and the token-shift commit block for
// tests/test_gpu_mix_exact.py (DESIGN.md "Mix, prologue and commit probe").  Not part of librwkv_hip.so: it links the kernel objects the build
// leaves in ai00_server_amd/csrc and calls only launch_tile_f16 (the weights arrive raw), launch_v6_mix, v6_mix_split, the v6_mix_*supported
// predicates and launch_gemm.  ONE launch per case; a `pair` case makes two (prologue launch, then the carrier that commits what it published).
//
//   mix_probe <cases.bin> <results.bin>        one JSON line per case on stdout: the arguments that went in, `split` / `ksp` as the product's
//                                              v6_mix_split gives them, and form, NT, both grids and the apply tile by the launcher's rule RESTATED
//                                              here (mix_plan): launch_v6_mix returns nothing, so these fields say what the rule gives, not what
//                                              was launched — that is constrained by the outputs alone
//
// The case file, the result file, the patterns and the order of work per case are those of every role-buffer probe: DESIGN.md "Probe container"
// (tests/cpp/probe_case.h, probe_common.h).  Here: elements of 2 | 4 bytes, `off` a multiple of 256, and the validation of every case BEFORE the
// GPU is touched: the supported-predicate of its form holds and every index the kernels form from its fields lies inside the buffer allocated
// for it; a refused case ends the process with its name.
#include "mix_probe_plan.h"
#include "probe_common.h"

using namespace rwkv;

enum Kind { K_MIX = 0, K_COMMIT, K_PAIR, K_COUNT };
enum Role {
    R_W1 = 0, R_W2_0, R_ZHI = R_W2_0 + 5, R_ZLO, R_XX, R_DX, R_MU0, R_MUX = R_MU0 + 5, R_OHI0, R_OLO0 = R_OHI0 + 5, R_MGHI = R_OLO0 + 5, R_MGLO, R_MP,
    R_XIN, R_XOUT, R_P, R_LNW, R_LNB, R_SX, R_SLOT, R_PREV, R_LAST, R_XXOUT, R_CW0, R_COUT0 = R_CW0 + 5, R_SRC = R_COUT0 + 5, R_COUNT
};
enum Param { P_T = 0, P_C, P_DM, P_HILO, P_LDZ, P_LDH, P_LNP, P_NP, P_PSTRIDE, P_SXSTRIDE, P_DENSE, P_NSLOTS, P_KSP_MIN_T, P_KSP_BLOCKS, P_KSP_MAX,
             P_DD, P_COMMIT_C, P_CARRIER_HILO, P_LDO, P_COUNT };
static const char *const PARAMS[P_COUNT] = {"T", "C", "Dm", "hilo", "ldz", "ldh", "lnp", "np", "pstride", "sx_slot_stride", "dense", "nslots", "ksp_min_t",
                                            "ksp_blocks", "ksp_max", "Dd", "commit_C", "carrier_hilo", "ldo"};
static const char *const KIND_NAME[K_COUNT] = {"mix", "commit", "pair"};

struct MixPlan { int form = 0, NT = 0, split = 0, ksp = 1, g1[3] = {0, 0, 0}, g2[2] = {0, 0}, apply_nt = 0; };   // form: 0 decode, 1 prologue, 2 wide, 3 split
static const char *const FORM_NAME[4] = {"decode", "lnp", "wide", "split"};
struct MixCase : Case {
    MixPlan mp;
    CarrierPlan cp;
    std::vector<void *> tiled;                                        // device: W1, W2_0..4, carrier W0..4 after launch_tile_f16
    int P(int i) const { return (int)p[i]; }
};

static V6MixArgs mix_args(const MixCase &c, bool device) {
    V6MixArgs a{};
    a.T = c.P(P_T); a.C = c.P(P_C); a.Dm = c.P(P_DM); a.ldz = c.P(P_LDZ); a.ldh = c.P(P_LDH);
    a.ksp_min_t = c.P(P_KSP_MIN_T); a.ksp_blocks = c.P(P_KSP_BLOCKS); a.ksp_max = c.P(P_KSP_MAX);
    // v6_mix_split looks at mg_hi / mg_lo / mp for null only: before the buffers exist on the device, presence stands in for the pointer
    static _Float16 dummy_h;
    static float dummy_f;
    a.mg_hi = device ? c.ptr<_Float16>(R_MGHI) : (c.find(R_MGHI) ? &dummy_h : nullptr);
    a.mg_lo = device ? c.ptr<_Float16>(R_MGLO) : (c.find(R_MGLO) ? &dummy_h : nullptr);
    a.mp = device ? c.ptr<float>(R_MP) : (c.find(R_MP) ? &dummy_f : nullptr);
    if (!device) return a;
    a.W1 = c.tiled[0];
    for (int m = 0; m < 5; ++m) {
        a.W2[m] = c.tiled[1 + m]; a.mu[m] = c.ptr<float>(R_MU0 + m);
        a.ohi[m] = c.ptr<_Float16>(R_OHI0 + m); a.olo[m] = c.ptr<_Float16>(R_OLO0 + m);
    }
    a.zhi = c.ptr<_Float16>(R_ZHI); a.zlo = c.ptr<_Float16>(R_ZLO); a.xx = c.ptr<float>(R_XX); a.dx = c.ptr<float>(R_DX);
    a.mu_x = c.ptr<float>(R_MUX);
    if (c.P(P_LNP)) {
        LnProArgs &l = a.lnp;
        l.x_in = c.ptr<float>(R_XIN); l.x_out = c.ptr<float>(R_XOUT); l.P = c.ptr<float>(R_P); l.np = c.P(P_NP); l.pstride = c.p[P_PSTRIDE];
        l.lnw = c.ptr<float>(R_LNW); l.lnb = c.ptr<float>(R_LNB); l.sx = c.ptr<float>(R_SX); l.sx_slot_stride = c.p[P_SXSTRIDE];
        l.rm = RowMeta{nullptr, c.ptr<int>(R_SLOT), c.ptr<int>(R_PREV), c.ptr<int>(R_LAST), c.P(P_DENSE)};
        l.mode = 1; l.xx_out = c.ptr<float>(R_XXOUT); l.C = a.C;
    }
    return a;
}

// the launcher's rules restated beside v6_mix_split (the product's own): form, token tiles per block, both grids, the apply launch's tile
static MixPlan mix_plan(const MixCase &c) {
    const V6MixArgs a = mix_args(c, false);
    const bool hilo = c.P(P_HILO) != 0;
    MixPlan m;
    const int groups = (a.C / 16 + 7) / 8;
    if (a.T <= 32) {
        m.form = c.P(P_LNP) ? 1 : 0; m.NT = a.T <= 16 ? 1 : 2;
        m.g1[0] = groups; m.g1[1] = 5; m.g1[2] = 1;
        return m;
    }
    const int ntile = (a.T + 31) / 32;
    m.NT = 2; m.split = v6_mix_split(a, hilo);
    if (m.split > 0) {
        m.form = 3; m.ksp = m.split;
        m.g1[0] = m.ksp; m.g1[1] = 5; m.g1[2] = ntile;
        const bool nt1 = (long)groups * ntile < 256;
        m.apply_nt = nt1 ? 1 : 2;
        m.g2[0] = groups; m.g2[1] = nt1 ? (a.T + 15) / 16 : ntile;
        return m;
    }
    m.form = 2;
    m.g1[0] = std::max(1, std::min(8, 256 / (5 * ntile))); m.g1[1] = 5; m.g1[2] = ntile;
    return m;
}

static void validate_mix(MixCase &c) {
    const int T = c.P(P_T), C = c.P(P_C), Dm = c.P(P_DM), hilo = c.P(P_HILO), ldz = c.P(P_LDZ), ldh = c.P(P_LDH), lnp = c.P(P_LNP);
    REQUIRE(c, T >= 1 && T <= 4096 && C >= 256 && C <= 8192 && (hilo == 0 || hilo == 1) && (lnp == 0 || lnp == 1));
    REQUIRE(c, ldh % 32 == 0 && ldh >= C);
    REQUIRE(c, c.P(P_KSP_MIN_T) >= 1 && c.P(P_KSP_BLOCKS) >= 1 && c.P(P_KSP_MAX) >= 1);
    if (lnp) REQUIRE(c, v6_mix_ln_supported(T, C, Dm, hilo != 0, c.P(P_NP)));
    else if (T <= 32) REQUIRE(c, v6_mix_supported(T, C, Dm));
    else REQUIRE(c, v6_mix_wide_supported(T, C, Dm));
    need(c, R_W1, 5LL * Dm * C, 2);
    for (int m = 0; m < 5; ++m) {
        need(c, R_W2_0 + m, (int64_t)C * Dm, 2); need(c, R_MU0 + m, C, 4);
        need(c, R_OHI0 + m, ceil16(T) * ldh, 2);
        if (hilo) need(c, R_OLO0 + m, ceil16(T) * ldh, 2); else REQUIRE(c, !c.find(R_OLO0 + m));      // olo is null exactly when the case is hi-only
    }
    if (!lnp) {
        REQUIRE(c, ldz % 32 == 0 && ldz >= C);
        need(c, R_ZHI, ceil16(T) * ldz, 2);
        if (hilo) need(c, R_ZLO, ceil16(T) * ldz, 2);
        need(c, R_XX, (int64_t)T * C, 4); need(c, R_DX, (int64_t)T * C, 4);
    } else {
        const int np = c.P(P_NP), dense = c.P(P_DENSE), nslots = c.P(P_NSLOTS);
        const int64_t pstride = c.p[P_PSTRIDE], stride = c.p[P_SXSTRIDE];
        REQUIRE(c, T <= LNP_MAX_T && np >= 1 && pstride >= 0 && pstride % 4 == 0 && stride >= C && stride % 4 == 0 && nslots >= 1 && (dense == 0 || dense == 1));
        need(c, R_XIN, (int64_t)T * C, 4); need(c, R_XOUT, (int64_t)T * C, 4); need(c, R_XXOUT, (int64_t)T * C, 4);
        need(c, R_P, (int64_t)(np - 1) * pstride + (int64_t)T * C, 4);
        need(c, R_LNW, C, 4); need(c, R_LNB, C, 4); need(c, R_MUX, C, 4);
        need(c, R_SX, (int64_t)(nslots - 1) * stride + C, 4);
        if (dense) REQUIRE(c, T <= nslots);
        else {
            need(c, R_SLOT, T, 4); need(c, R_PREV, T, 4);
            for (int t = 0; t < T; ++t) REQUIRE(c, c.host<int>(R_SLOT)[t] >= 0 && c.host<int>(R_SLOT)[t] < nslots && c.host<int>(R_PREV)[t] == -1);   // one row per slot: no row to shift from
        }
        REQUIRE(c, (size_t)8 * 4 * 64 * 16 + (size_t)2 * 16 * (Dm + 8) * 2 + lnp_lds_bytes(LNP_MAX_T, C, false) <= 160 * 1024);
    }
    c.mp = mix_plan(c);
    if (c.mp.form == 3) {
        REQUIRE(c, T % 32 == 0 && ((C >> 5) >> 3) % c.mp.ksp == 0);
        if (c.mp.ksp > 1) need(c, R_MP, (int64_t)c.mp.ksp * 5 * T * Dm, 4);
        else { need(c, R_MGHI, 5LL * T * Dm, 2); if (hilo) need(c, R_MGLO, 5LL * T * Dm, 2); }
    }
    REQUIRE(c, c.mp.g1[0] >= 1 && (long)c.mp.g1[0] * c.mp.g1[1] * c.mp.g1[2] <= (1 << 16));
}

static void validate_commit(MixCase &c, bool pair) {
    const int T = c.P(P_T), C = c.P(P_C), ldh = c.P(P_LDH), Dd = c.P(P_DD), CC = c.P(P_COMMIT_C), ch = c.P(P_CARRIER_HILO), ldo = c.P(P_LDO);
    const int dense = c.P(P_DENSE), nslots = c.P(P_NSLOTS);
    const int64_t stride = c.p[P_SXSTRIDE];
    REQUIRE(c, T >= 1 && T <= 64 && C >= 32 && C % 32 == 0 && ldh % 32 == 0 && ldh >= C && (ch == 0 || ch == 1) && ldo % 4 == 0 && ldo >= C && ldo >= Dd);
    REQUIRE(c, CC >= 4 && CC % 4 == 0 && stride >= CC && stride % 4 == 0 && nslots >= 1 && (dense == 0 || dense == 1));
    if (pair) REQUIRE(c, CC == C && !ch);
    carrier_plan(T, ch != 0, C, Dd, c.cp);
    if (c.cp.why) refuse(c, c.cp.why);
    for (int i = 0; i < CARRIER_NPROB; ++i) {
        need(c, R_CW0 + i, (int64_t)(i == 4 ? Dd : C) * C, 2);
        need(c, R_COUT0 + i, (int64_t)T * ldo, 4);
        need(c, R_OHI0 + i, ceil16(T) * ldh, 2);
        if (ch) need(c, R_OLO0 + i, ceil16(T) * ldh, 2);
    }
    need(c, pair ? R_XXOUT : R_SRC, (int64_t)T * CC, 4);
    need(c, R_SX, (int64_t)(nslots - 1) * stride + CC, 4);
    if (dense) { REQUIRE(c, T <= nslots); return; }
    need(c, R_SLOT, T, 4); need(c, R_LAST, T, 4);
    std::vector<int> writers(nslots, 0);
    for (int t = 0; t < T; ++t) {
        const int sl = c.host<int>(R_SLOT)[t], la = c.host<int>(R_LAST)[t];
        REQUIRE(c, sl >= 0 && sl < nslots && la >= -1 && la < T);
        if (la >= 0) REQUIRE(c, ++writers[sl] == 1);
    }
}

static void validate(MixCase &c) {
    REQUIRE(c, (int)c.p.size() == P_COUNT);
    for (const Buf &x : c.b) {
        REQUIRE(c, x.role >= 0 && x.role < R_COUNT && (x.esize == 2 || x.esize == 4) && x.off >= 0 && x.off % 256 == 0 && x.off <= x.nbytes);
        REQUIRE(c, x.nbytes < (int64_t)1 << 31);                       // activation accessors form 32-bit byte offsets
        int same = 0;
        for (const Buf &y : c.b) same += y.role == x.role;
        REQUIRE(c, same == 1);
    }
    if (c.kind == K_MIX || c.kind == K_PAIR) validate_mix(c);
    if (c.kind == K_PAIR) REQUIRE(c, c.P(P_LNP) == 1);
    if (c.kind == K_COMMIT || c.kind == K_PAIR) validate_commit(c, c.kind == K_PAIR);
}

// raw fp16 [rows][K] of `role` -> a tiled device buffer, by the product's load-time kernel
static void *tile(const MixCase &c, int role, int rows, int K, hipStream_t s) {
    void *out = nullptr;
    HIP_OK(hipMalloc(&out, (size_t)rows * K * 2));
    launch_tile_f16(c.ptr<_Float16>(role), rows, rows, K, out, s);
    HIP_OK(hipGetLastError());
    return out;
}

static void launch_carrier(MixCase &c, hipStream_t s) {
    const int T = c.P(P_T), C = c.P(P_C), Dd = c.P(P_DD), ldh = c.P(P_LDH), ldo = c.P(P_LDO);
    const bool ch = c.P(P_CARRIER_HILO) != 0;
    DMat mats[CARRIER_NPROB];
    for (int i = 0; i < CARRIER_NPROB; ++i) {
        mats[i].fmt = W_F16; mats[i].rows = i == 4 ? Dd : C; mats[i].K = C; mats[i].data = c.tiled[6 + i]; mats[i].bytes = (uint64_t)mats[i].rows * C * 2;
        ProbSpec ps;
        ps.W = &mats[i];
        ps.x = Opd{c.ptr<_Float16>(R_OHI0 + kCarrierMix[i]), ch ? c.ptr<_Float16>(R_OLO0 + kCarrierMix[i]) : nullptr, ldh};
        ps.act = kCarrierAct[i]; ps.out = c.ptr<float>(R_COUT0 + i); ps.ldo = ldo;
        fill_prob(c.cp.Lh.p[i], ps, (long)T * ldo);
    }
    ShiftCommit cm{};
    cm.src = c.kind == K_PAIR ? c.ptr<float>(R_XXOUT) : c.ptr<float>(R_SRC);
    cm.sx = c.ptr<float>(R_SX); cm.sx_slot_stride = c.p[P_SXSTRIDE];
    cm.rm = RowMeta{nullptr, c.ptr<int>(R_SLOT), c.ptr<int>(R_PREV), c.ptr<int>(R_LAST), c.P(P_DENSE)};
    cm.T = T; cm.C = c.P(P_COMMIT_C);
    c.cp.Lh.commit = cm;
    launch_gemm(c.cp.Lh, ch, s);
    launched(s);
}

// the weights tiled by the product's load-time kernel, then the mix launch, the carrier, or both in that order
static void launch(MixCase &c, hipStream_t s) {
    const int C = c.P(P_C), Dm = c.P(P_DM);
    c.tiled.assign(11, nullptr);
    if (c.kind != K_COMMIT) {
        c.tiled[0] = tile(c, R_W1, 5 * Dm, C, s);
        for (int m = 0; m < 5; ++m) c.tiled[1 + m] = tile(c, R_W2_0 + m, C, Dm, s);
    }
    if (c.kind != K_MIX)
        for (int i = 0; i < CARRIER_NPROB; ++i) c.tiled[6 + i] = tile(c, R_CW0 + i, i == 4 ? c.P(P_DD) : C, C, s);
    HIP_OK(hipStreamSynchronize(s));
    if (c.kind != K_COMMIT) {
        launch_v6_mix(mix_args(c, true), c.P(P_HILO) != 0, s);
        launched(s);
    }
    if (c.kind != K_MIX) launch_carrier(c, s);
    for (void *p : c.tiled) if (p) HIP_OK(hipFree(p));
}

static void fields(const MixCase &c) {
    std::printf(", \"kind\": \"%s\"", KIND_NAME[c.kind]);
    for (int i = 0; i < P_COUNT; ++i) std::printf(", \"%s\": %lld", PARAMS[i], (long long)c.p[i]);
    if (c.kind != K_COMMIT) {
        const MixPlan &m = c.mp;
        std::printf(", \"form\": \"%s\", \"NT\": %d, \"split\": %d, \"ksp\": %d, \"grid1\": [%d, %d, %d], \"grid2\": [%d, %d], \"apply_nt\": %d",
                    FORM_NAME[m.form], m.NT, m.split, m.ksp, m.g1[0], m.g1[1], m.g1[2], m.g2[0], m.g2[1], m.apply_nt);
    }
    if (c.kind != K_MIX) {
        std::printf(", \"carrier\": ");
        carrier_print(stdout, c.cp);
        std::printf(", \"launch_grid\": %d", c.cp.Lh.total_blocks + 1);
    }
}

int main(int argc, char **argv) {
    return probe_main<MixCase>(argc, argv, ProbeSpec{"mix_probe", 0x4252504D, K_COUNT, 32, R_COUNT, 2}, validate, launch, fields);
}


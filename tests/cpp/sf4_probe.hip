// sf4_probe.hip — stand-alone driver of the GEMM kernels on W_SF4 problems, alone and beside fp16 and NF4 problems in one launch, for
// tests/test_gpu_sf4.py.  Not part of librwkv_hip.so: it links the kernel objects the build leaves in ai00_server_amd/csrc, runs
// the product's load-time kernels (launch_tile_f16 / launch_quant_nf4 / launch_quant_sf4) on raw weights, plans with the engine's own planner
// and launches through launch_gemm_tile / launch_gemm, ONE launch per case.
//
//   sf4_probe <cases.bin> <results.bin>        one JSON line per case on stdout: the plan that ran
//
// The case file, the result file, the patterns and the order of work per case are those of every role-buffer probe: DESIGN.md "Probe container"
// (tests/cpp/probe_case.h, probe_common.h; tests/sf4_cases.py writes the cases through tests/probe_io.py).  Elements of 2 | 4 bytes.
//   params: T hilo mode force_spb tile_shape nprob ldx ldo, then per problem: rows K fmt ocol
//           mode 2: plan_decode(force_spb); 1: tile_geometry(tile_shape, one K copy)
//   roles:  xhi, xlo  f16 [ceil16(T) * ldx] in B-fragment order;  out  f32 [T * ldo];  per problem i: w_i  raw f16 [rows * K],
//           pay_i / sc_i  the tiled payload and the scales the load-time kernel writes (as 2-byte elements; no sc_i for fp16)
// Every problem has a plain epilogue (no activation, bias or post-op), xoff 0, fp32 output at column ocol, and is not partial.
// Every case is validated and planned BEFORE anything is launched: every index the kernels form from the case's fields lies inside the
// buffer allocated for it.  A W_SF4 shape must plan exactly as the same shape with W_NF4 does, or the case is refused.
#include "gemm_probe_plan.h"
#include "probe_common.h"

using namespace rwkv;

enum Kind { K_GEMM = 0, K_COUNT };
constexpr int MAXN = 3;
enum Role { R_XHI = 0, R_XLO, R_OUT, R_W0, R_PAY0 = R_W0 + MAXN, R_SC0 = R_PAY0 + MAXN, R_COUNT = R_SC0 + MAXN };

struct SfCase : Case {
    ProbePlan plan;
    ProbeReq req{};
};

static size_t payload_bytes(int fmt, int rows, int K) { return fmt == W_F16 ? (size_t)rows * K * 2 : (size_t)rows * K / 2; }
static size_t scale_bytes(int fmt, int rows, int K) { return fmt == W_F16 ? 0 : (size_t)rows * (K / 64) * 2; }

static void plan_with(const ProbeReq &q, const ProbShape *sh, GemmLaunch &Lh, GemmPlan &pl) {
    if (q.mode == 2) {
        const int np = plan_decode(Lh, sh, q.nprob, q.T, q.hilo != 0, q.force_spb);
        pl = {GEMM_DECODE, Lh.single_shot, Lh.total_blocks, Lh.threads, np};
    } else {
        const TilePlan tp = tile_geometry(Lh, sh, q.nprob, q.T, q.tile_shape, 1);
        pl = {GEMM_TILE, tp.shape, Lh.total_blocks, tp.threads, tp.ksplit};
    }
}

static void validate(SfCase &c) {
    const std::vector<int64_t> &p = c.p;
    for (const Buf &x : c.b) {
        REQUIRE(c, x.role >= 0 && x.role < R_COUNT && (x.esize == 2 || x.esize == 4) && x.off >= 0 && x.off % 256 == 0 && x.off <= x.nbytes);
        int same = 0;
        for (const Buf &y : c.b) same += y.role == x.role;
        REQUIRE(c, same == 1);
    }
    REQUIRE(c, c.kind == K_GEMM && p.size() >= 8);
    const int T = p[0], hilo = p[1], mode = p[2], force_spb = p[3], tile_shape = p[4], n = p[5], ldx = p[6], ldo = p[7];
    REQUIRE(c, T >= 1 && T <= 4096 && (hilo == 0 || hilo == 1) && (mode == 1 || mode == 2) && n >= 1 && n <= MAXN && (int)p.size() == 8 + 4 * n);
    REQUIRE(c, ldx >= 32 && ldx % 32 == 0 && ldx <= 65536 && ldo >= 16 && ldo % 4 == 0 && ldo <= 65536);
    need(c, R_XHI, ceil16(T) * ldx, 2);
    if (hilo) need(c, R_XLO, ceil16(T) * ldx, 2);
    need(c, R_OUT, (int64_t)T * ldo, 4);
    ProbShape real[MAXN], as_nf4[MAXN];
    for (int i = 0; i < n; ++i) {
        const int rows = p[8 + 4 * i], K = p[9 + 4 * i], fmt = p[10 + 4 * i], ocol = p[11 + 4 * i];
        REQUIRE(c, rows >= 16 && rows % 16 == 0 && rows <= 4096 && K >= 32 && K <= ldx);
        REQUIRE(c, fmt == W_F16 || fmt == W_NF4 || fmt == W_SF4);
        REQUIRE(c, K % (fmt == W_F16 ? 32 : 256) == 0);
        REQUIRE(c, ocol >= 0 && ocol % 4 == 0 && ocol + rows <= ldo);
        need(c, R_W0 + i, (int64_t)rows * K, 2);
        need(c, R_PAY0 + i, (int64_t)payload_bytes(fmt, rows, K) / 2, 2);
        if (fmt != W_F16) need(c, R_SC0 + i, (int64_t)scale_bytes(fmt, rows, K) / 2, 2);
        // gemm_plan.h shape_of of a plain, non-partial problem with fp32 output and xoff 0
        real[i] = ProbShape{rows, K, fmt, false, true, true};
        as_nf4[i] = real[i];
        if (fmt == W_SF4) as_nf4[i].fmt = W_NF4;
    }
    // the plan of the same launch with NF4 in SF4's place, through the checks every GEMM probe case goes through (gemm_probe_plan.h) ...
    c.req = ProbeReq{T, hilo, mode, force_spb, tile_shape, mode == 1 ? 1 : 0, -1, n, 1};
    probe_plan(c.req, as_nf4, c.plan);
    if (!c.plan.why.empty()) refuse(c, c.plan.why);
    REQUIRE(c, c.plan.pl.path == (mode == 2 ? GEMM_DECODE : GEMM_TILE) && c.plan.pl.ksplit == 1);
    // ... and the plan the engine makes for the formats as they are: it must be the same one, field for field
    GemmLaunch Lh{};
    GemmPlan pl{GEMM_DECODE, 0, 0, 0, 1};
    plan_with(c.req, real, Lh, pl);
    const GemmLaunch &A = c.plan.Lh;
    REQUIRE(c, pl.path == c.plan.pl.path && pl.variant == c.plan.pl.variant && pl.grid == c.plan.pl.grid && pl.threads == c.plan.pl.threads && pl.ksplit == c.plan.pl.ksplit);
    REQUIRE(c, Lh.total_blocks == A.total_blocks && Lh.threads == A.threads && Lh.single_shot == A.single_shot && Lh.tail == A.tail && Lh.lds_items == A.lds_items &&
                   Lh.T == A.T && Lh.nprob == A.nprob && Lh.xcd_map == A.xcd_map);
    for (int i = 0; i < n; ++i) {
        const GemmProb &g = Lh.p[i], &h = A.p[i];
        REQUIRE(c, g.spb == h.spb && g.nw == h.nw && g.ksb == h.ksb && g.Kb == h.Kb && g.nslice == h.nslice && g.nblk_strip == h.nblk_strip && g.block_begin == h.block_begin);
        REQUIRE(c, g.ksb == 1);                                        // one slab: the fp32 buffer has room for no other
    }
    c.plan.Lh = Lh;
}

static void launch(SfCase &c, hipStream_t s) {
    const std::vector<int64_t> &p = c.p;
    const int T = p[0], n = p[5], ldx = p[6], ldo = p[7];
    const bool hilo = p[1] != 0;
    DMat mats[MAXN];
    ProbSpec ps[MAXN];
    for (int i = 0; i < n; ++i) {
        const int rows = p[8 + 4 * i], K = p[9 + 4 * i], fmt = p[10 + 4 * i], ocol = p[11 + 4 * i];
        const _Float16 *raw = c.ptr<_Float16>(R_W0 + i);
        void *pay = c.ptr<unsigned char>(R_PAY0 + i), *sc = fmt == W_F16 ? nullptr : c.ptr<unsigned char>(R_SC0 + i);
        if (fmt == W_F16) launch_tile_f16(raw, rows, rows, K, pay, s);
        else if (fmt == W_NF4) launch_quant_nf4(raw, rows, K, pay, sc, s);
        else launch_quant_sf4(raw, rows, K, pay, sc, s);
        launched(s);
        mats[i].data = pay; mats[i].scales = sc; mats[i].fmt = fmt; mats[i].rows = rows; mats[i].K = K;
        mats[i].bytes = payload_bytes(fmt, rows, K) + scale_bytes(fmt, rows, K);
        ps[i].W = &mats[i];
        ps[i].x.hi = c.ptr<_Float16>(R_XHI); ps[i].x.lo = hilo ? c.ptr<_Float16>(R_XLO) : nullptr; ps[i].x.ld = ldx;
        ps[i].out = c.ptr<float>(R_OUT) + ocol; ps[i].ldo = ldo;
    }
    GemmLaunch &Lh = c.plan.Lh;
    for (int i = 0; i < n; ++i) fill_prob(Lh.p[i], ps[i], (long)T * ldo);
    if (c.plan.pl.path == GEMM_TILE) launch_gemm_tile(Lh, c.plan.pl.variant, hilo, s);
    else launch_gemm(Lh, hilo, s);
    launched(s);
}

static void fields(const SfCase &c) {
    const GemmPlan &pl = c.plan.pl;
    const bool tile = pl.path == GEMM_TILE;
    std::printf(", \"status\": \"ran\", \"path\": \"%s\", \"T\": %d, \"hilo\": %d, \"shape\": %d, \"NT\": %d, \"single_shot\": %d, \"total_blocks\": %d, \"threads\": %d, \"fmts\": [",
                kGemmPathNames[pl.path], c.req.T, c.req.hilo, tile ? pl.variant : -1, c.plan.NT, tile ? -1 : c.plan.Lh.single_shot, c.plan.Lh.total_blocks, pl.threads);
    for (int i = 0; i < c.req.nprob; ++i) std::printf("%s%d", i ? ", " : "", c.plan.Lh.p[i].fmt);
    std::printf("]");
}

int main(int argc, char **argv) {
    return probe_main<SfCase>(argc, argv, ProbeSpec{"sf4_probe", 0x42344653, K_COUNT, 8 + 4 * MAXN, R_COUNT, 2}, validate, launch, fields);
}

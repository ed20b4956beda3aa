// gemm_probe_plan.h — how a case of tests/gemm_cases.py becomes a plan: shared by tests/cpp/gemm_probe.hip (which then launches it on the
// GPU) and tests/cpp/gemm_plan_test.cpp (argument "probe": the same plan line from a plain host compiler, for the coverage proof of
// tests/test_gemm_cases_cpu.py).  Host-only: the engine's planner (gemm_plan.h) decides, this file only picks which of its entry points a
// case asks for, refuses what the kernels cannot take, and prints what was planned.
#pragma once
#include "../../ai00_server_amd/csrc/gemm_plan.h"
#include <cstdio>
#include <string>

namespace rwkv {

struct ProbeReq {
    int T, hilo;
    int mode;                        // -1: plan_gemm decides (tile_shape / xcd_map >= 0 and ksplit == 1 go into its Knobs); 2: plan_decode(force_spb); 1: tile_geometry(tile_shape, ksplit)
    int force_spb, tile_shape, ksplit, xcd_map, nprob;
    int nslab;                       // partial slabs the caller's fp32 buffer has room for
};
struct ProbePlan {
    GemmLaunch Lh;
    GemmPlan pl{GEMM_DECODE, 0, 0, 0, 1};
    int NT = 0;
    std::string why;                 // not empty: unsupported, nothing may be launched
};

inline void probe_plan(const ProbeReq &q, const ProbShape *sh, ProbePlan &r) {
    auto need = [&](bool ok, const char *what) { if (!ok && r.why.empty()) r.why = what; };
    const int n = q.nprob, T = q.T;
    const bool hilo = q.hilo != 0;
    need(T >= 1 && n >= 1 && n <= GEMM_MAXP, "T >= 1, 1 .. GEMM_MAXP problems");
    need(q.mode == -1 || q.mode == 1 || q.mode == 2, "mode");
    need(q.xcd_map >= -1 && q.xcd_map <= 2, "xcd_map");
    need(q.force_spb >= 0 && q.force_spb <= 8, "force_spb");
    if (!r.why.empty()) return;
    for (int i = 0; i < n; ++i) {
        need(sh[i].rows >= 16 && sh[i].rows % 16 == 0, "rows % 16");
        need(sh[i].fmt == W_F16 || sh[i].fmt == W_INT8 || sh[i].fmt == W_NF4, "fmt");
        need(sh[i].K >= 32 && sh[i].K % (sh[i].fmt == W_F16 ? 32 : 256) == 0, "K alignment of the format");
    }
    if (!r.why.empty()) return;
    Knobs kn;
    kn.tile_shape = q.tile_shape; kn.tile_xcd = q.xcd_map;
    if (q.ksplit == 1 && q.mode == -1) kn.tile_ksplit = 0;
    if (q.mode == 2) {
        const int np = plan_decode(r.Lh, sh, n, T, hilo, q.force_spb);
        r.pl = {GEMM_DECODE, r.Lh.single_shot, r.Lh.total_blocks, r.Lh.threads, np};
    } else if (q.mode == 1) {
        need(T >= GEMM_TILE_MIN_T, "tile launches start at GEMM_TILE_MIN_T rows");
        need(q.tile_shape >= 0 && q.tile_shape < GEMM_TILE_SHAPES, "tile shape");
        need(q.ksplit >= 1 && q.ksplit <= 4, "tile K copies");
        if (!r.why.empty()) return;
        for (int i = 0; i < n; ++i) {
            need(gemm_tile_shape_supported(q.tile_shape, hilo, sh[i].K), "gemm_tile_shape_supported");
            const int kc = kTileShapes[q.tile_shape].kc;
            const int units = gemm_tile_pipelined(q.tile_shape) ? sh[i].K / 128 : (sh[i].K + kc - 1) / kc;
            need(q.ksplit == 1 || (sh[i].partial && sh[i].kcopies && units >= q.ksplit), "K copies need a linear problem and one chunk per copy");
        }
        if (!r.why.empty()) return;
        const TilePlan tp = tile_geometry(r.Lh, sh, n, T, q.tile_shape, q.ksplit);
        if (q.xcd_map >= 0) r.Lh.xcd_map = q.xcd_map;
        r.pl = {GEMM_TILE, tp.shape, r.Lh.total_blocks, tp.threads, tp.ksplit};
    } else {
        r.pl = plan_gemm(r.Lh, sh, n, T, hilo, false, kn);
    }
    need(r.pl.ksplit >= 1, "plan == 0: a linear problem's K cannot be split");
    need(r.pl.ksplit <= q.nslab, "more partial slabs than the case has room for");
    need(r.Lh.total_blocks >= 1 && r.Lh.total_blocks <= (1 << 20), "grid");
    if (!r.why.empty()) return;
    if (r.pl.path == GEMM_TILE)
        for (int i = 0; i < n; ++i) need(gemm_tile_shape_supported(r.pl.variant, hilo, sh[i].K), "gemm_tile_shape_supported");
    if (r.pl.path == GEMM_DECODE) {
        int KSW;
        gemm_variant(T, hilo, r.NT, KSW);
        need(r.Lh.threads <= gemm_variant_max_waves(r.NT, KSW, hilo) * 64 && r.Lh.lds_items * r.NT <= 160, "decode block shape");
    }
}

// one JSON line: everything needed to say which code ran
inline void probe_print(FILE *f, int ci, const ProbeReq &q, const ProbePlan &r) {
    if (!r.why.empty()) {
        std::fprintf(f, "{\"case\": %d, \"status\": \"unsupported\", \"why\": \"%s\"}\n", ci, r.why.c_str());
        return;
    }
    const bool tile = r.pl.path == GEMM_TILE, dec = r.pl.path == GEMM_DECODE;
    std::fprintf(f, "{\"case\": %d, \"status\": \"ran\", \"path\": \"%s\", \"T\": %d, \"hilo\": %d, \"shape\": %d, \"NT\": %d, \"single_shot\": %d, \"tail\": %d, "
                    "\"total_blocks\": %d, \"grid\": %d, \"threads\": %d, \"xcd_map\": %d, \"ksplit\": %d, \"probs\": [",
                 ci, kGemmPathNames[r.pl.path], q.T, q.hilo ? 1 : 0, tile ? r.pl.variant : -1, r.NT, dec ? r.Lh.single_shot : -1, dec ? r.Lh.tail : -1,
                 r.Lh.total_blocks, r.pl.grid, r.pl.threads, tile ? r.Lh.xcd_map : -1, r.pl.ksplit);
    for (int i = 0; i < q.nprob; ++i) {
        const GemmProb &g = r.Lh.p[i];
        std::fprintf(f, "%s{\"spb\": %d, \"nw\": %d, \"ksb\": %d, \"Kb\": %d, \"nslice\": %d, \"nblk_strip\": %d, \"block_begin\": %d}",
                     i ? ", " : "", g.spb, g.nw, g.ksb, tile ? 0 : g.Kb, tile ? 0 : g.nslice, g.nblk_strip, g.block_begin);
    }
    std::fprintf(f, "]}\n");
}

}  // namespace rwkv

// mix_probe_plan.h — the commit carrier of tests/mix_cases.py as a plan: shared by tests/cpp/mix_probe.hip (which launches it on the GPU) and
// tests/cpp/mix_plan_test.cpp (the same line from a plain host compiler, for tests/test_mix_cases_cpu.py).  Host-only.  The carrier is the
// V6 att launch of rwkv_engine.cpp in small: Wk, Wv, Wr (linear), Wg (SiLU), all [C][C], and the decay LoRA's first stage D1 [Dd][C] (tanh), each
// reading its own operand, planned by the engine's plan_gemm with has_commit = true.
#pragma once
#include "../../ai00_server_amd/csrc/gemm_plan.h"
#include <cstdio>

namespace rwkv {

constexpr int CARRIER_NPROB = 5;
constexpr int kCarrierAct[CARRIER_NPROB] = {ACT_NONE, ACT_NONE, ACT_NONE, ACT_SILU, ACT_TANH};
constexpr int kCarrierMix[CARRIER_NPROB] = {1, 2, 3, 4, 0};        // which of the five mix operands (w, k, v, r, g) a problem reads

inline void carrier_shapes(int C, int Dd, ProbShape *sh) {
    // what shape_of gives for these problems: fp32 output only, no bias, no post-op, no column offset
    for (int i = 0; i < CARRIER_NPROB; ++i) sh[i] = {i == 4 ? Dd : C, C, W_F16, false, kCarrierAct[i] == ACT_NONE, true};
}

struct CarrierPlan {
    GemmLaunch Lh;
    GemmPlan pl{GEMM_DECODE, 0, 0, 0, 1};
    int NT = 0;
    bool smallk_without_commit = false;
    const char *why = nullptr;       // not null: nothing may be launched
};

inline void carrier_plan(int T, bool hilo, int C, int Dd, CarrierPlan &r) {
    if (T < 1 || T > 64 || C < 32 || C % 32 || Dd < 16 || Dd % 16) { r.why = "carrier shape"; return; }
    ProbShape sh[CARRIER_NPROB];
    carrier_shapes(C, Dd, sh);
    r.smallk_without_commit = smallk_eligible(sh, CARRIER_NPROB, T, false);
    r.pl = plan_gemm(r.Lh, sh, CARRIER_NPROB, T, hilo, true, Knobs{});
    if (r.pl.path != GEMM_DECODE) { r.why = "a launch with a commit must stay on the decode kernel"; return; }
    if (r.pl.ksplit != 1) { r.why = "the carrier writes no partial slabs"; return; }
    int KSW;
    gemm_variant(T, hilo, r.NT, KSW);
    if (r.Lh.total_blocks < 1 || r.Lh.total_blocks > (1 << 16) || r.Lh.threads > gemm_variant_max_waves(r.NT, KSW, hilo) * 64 || r.Lh.lds_items * r.NT > 160)
        r.why = "decode block shape";
}

// the carrier's part of a case's JSON line (an object)
inline void carrier_print(FILE *f, const CarrierPlan &r) {
    std::fprintf(f, "{\"path\": \"%s\", \"smallk_without_commit\": %d, \"NT\": %d, \"single_shot\": %d, \"tail\": %d, \"total_blocks\": %d, \"grid\": %d, \"threads\": %d, \"probs\": [",
                 kGemmPathNames[r.pl.path], r.smallk_without_commit ? 1 : 0, r.NT, r.Lh.single_shot, r.Lh.tail, r.Lh.total_blocks, r.pl.grid, r.pl.threads);
    for (int i = 0; i < CARRIER_NPROB; ++i) {
        const GemmProb &g = r.Lh.p[i];
        std::fprintf(f, "%s{\"spb\": %d, \"nw\": %d, \"ksb\": %d, \"block_begin\": %d}", i ? ", " : "", g.spb, g.nw, g.ksb, g.block_begin);
    }
    std::fprintf(f, "]}");
}

}  // namespace rwkv

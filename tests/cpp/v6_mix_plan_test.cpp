// v6_mix_plan_test.cpp — the geometry of the one-launch forms of v6_mix_kernel without a GPU (tests/test_v6_mix_plan_cpu.py).
//   v6_mix_plan_test     stdin: one line "T C Dm" per launch; stdout: one JSON object per line — the plan, and the ownership of every
//                        (mix, token tile, strip) counted by walking the grid with the kernel's own strip rule
// Build: g++ -std=c++17 tests/cpp/v6_mix_plan_test.cpp   (host-only: may be built with -fsanitize=address,undefined)
#include "../../ai00_server_amd/csrc/gemm_plan.h"
#include <cstdio>
#include <vector>

int main() {
    int T, C, Dm;
    while (std::scanf("%d %d %d", &T, &C, &Dm) == 3) {
        const rwkv::V6MixPlan p = rwkv::v6_mix_plan(T, C, Dm, 0);
        const int S = C / 16, tiles = (T + p.NT * 16 - 1) / (p.NT * 16);
        if (p.gx < 1 || p.gz < 1 || p.sq < 0 || p.sr < 0) { std::fprintf(stderr, "v6_mix_plan_test: plan out of range\n"); return 1; }
        std::vector<int> owners((size_t)5 * p.gz * S, 0);
        int beyond = 0, max_group = 0;                    // strips a block would own past C/16 or past its 8 waves
        for (int c = 0; c < 5; ++c)
            for (int tz = 0; tz < p.gz; ++tz)
                for (int sg = 0; sg < p.gx; ++sg) {
                    const int n = p.sq + (sg < p.sr ? 1 : 0), s0 = sg * p.sq + std::min(sg, p.sr);     // v6_mix_kernel: strip = s0 + wave, wave < n
                    max_group = std::max(max_group, n);
                    for (int w = 0; w < n; ++w) {
                        if (w >= 8 || s0 + w >= S) { ++beyond; continue; }
                        ++owners[((size_t)c * p.gz + tz) * S + s0 + w];
                    }
                }
        int lo = 1 << 30, hi = 0;
        for (int o : owners) { lo = std::min(lo, o); hi = std::max(hi, o); }
        std::printf("{\"T\": %d, \"C\": %d, \"Dm\": %d, \"NT\": %d, \"grid\": [%d, 5, %d], \"sq\": %d, \"sr\": %d, \"lds\": %zu, \"token_tiles\": %d, "
                    "\"owners_min\": %d, \"owners_max\": %d, \"beyond\": %d, \"max_group\": %d}\n",
                    T, C, Dm, p.NT, p.gx, p.gz, p.sq, p.sr, p.lds, tiles, lo, hi, beyond, max_group);
    }
    return 0;
}

// CPU driver of ai00_server_amd/csrc/gemm_plan.h for tests/test_gemm_plan_cpp.py: plans the launches it reads, prints what the engine would log.
//   stdin, one launch per line:  T hilo commit no_tile tile_shape tile_ksplit tile_xcd nprob {rows K fmt partial kcopies smallk}...
//   stdout, one line per launch: kind variant grid threads ksplit
// Compiled with a plain host compiler: no HIP, no library of the project.
#include "../../ai00_server_amd/csrc/gemm_plan.h"
#include <cstdio>

int main() {
    using namespace rwkv;
    int T, hilo, commit, n;
    Knobs kn;
    while (std::scanf("%d %d %d %d %d %d %d %d", &T, &hilo, &commit, &kn.no_tile, &kn.tile_shape, &kn.tile_ksplit, &kn.tile_xcd, &n) == 8) {
        if (n < 1 || n > GEMM_MAXP) return 2;
        ProbShape ps[GEMM_MAXP];
        for (int i = 0; i < n; ++i) {
            int partial, kcopies, smallk;
            if (std::scanf("%d %d %d %d %d %d", &ps[i].rows, &ps[i].K, &ps[i].fmt, &partial, &kcopies, &smallk) != 6) return 2;
            ps[i].partial = partial != 0; ps[i].kcopies = kcopies != 0; ps[i].smallk = smallk != 0;
        }
        GemmLaunch Lh;
        const GemmPlan pl = plan_gemm(Lh, ps, n, T, hilo != 0, commit != 0, kn);
        std::printf("%s %d %d %d %d\n", kGemmPathNames[pl.path], pl.variant, pl.grid, pl.threads, pl.ksplit);
    }
    return 0;
}

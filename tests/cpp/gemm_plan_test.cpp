// CPU driver of ai00_server_amd/csrc/gemm_plan.h for tests/test_gemm_plan_cpp.py: plans the launches it reads, prints what the engine would log.
//   stdin, one launch per line:  T hilo commit no_tile tile_shape tile_ksplit tile_xcd nprob {rows K fmt partial kcopies smallk}...
//   stdout, one line per launch: kind variant grid threads ksplit
//   with the argument "geometry" the line goes on with what the kernels of that launch index by:
//     total_blocks strips_per_tile_block tokens_per_tile_block nprob {Kb ksb nslice nblk_strip spb nw block_begin tile_blocks}...
//   (tile_blocks: gemm_tile_blocks of the problem on the planned shape, 0 on the other paths; the two per-block figures are 0 there too)
//   with the argument "probe" it reads the launches of tests/gemm_cases.py instead and prints the plan line tests/cpp/gemm_probe.hip prints for
//   them on the GPU (gemm_probe_plan.h: NT, tail and the per-problem geometry too):
//     T hilo mode force_spb tile_shape ksplit xcd_map nslab nprob {rows K fmt partial kcopies smallk}...
// Compiled with a plain host compiler: no HIP, no library of the project.
#include "gemm_probe_plan.h"
#include <cstdio>
#include <cstring>

int main(int argc, char **argv) {
    const bool geometry = argc > 1 && !std::strcmp(argv[1], "geometry");
    using namespace rwkv;
    if (argc > 1 && !std::strcmp(argv[1], "probe")) {
        ProbeReq q;
        for (int ci = 0; std::scanf("%d %d %d %d %d %d %d %d %d", &q.T, &q.hilo, &q.mode, &q.force_spb, &q.tile_shape, &q.ksplit, &q.xcd_map, &q.nslab, &q.nprob) == 9; ++ci) {
            if (q.nprob < 1 || q.nprob > GEMM_MAXP) return 2;
            ProbShape ps[GEMM_MAXP];
            for (int i = 0; i < q.nprob; ++i) {
                int partial, kcopies, smallk;
                if (std::scanf("%d %d %d %d %d %d", &ps[i].rows, &ps[i].K, &ps[i].fmt, &partial, &kcopies, &smallk) != 6) return 2;
                ps[i].partial = partial != 0; ps[i].kcopies = kcopies != 0; ps[i].smallk = smallk != 0;
            }
            ProbePlan r;
            probe_plan(q, ps, r);
            probe_print(stdout, ci, q, r);
        }
        return 0;
    }
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
        std::printf("%s %d %d %d %d", kGemmPathNames[pl.path], pl.variant, pl.grid, pl.threads, pl.ksplit);
        if (geometry) {
            const bool tile = pl.path == GEMM_TILE;
            const TileShape ts = kTileShapes[tile ? pl.variant : 0];
            std::printf(" %d %d %d %d", Lh.total_blocks, tile ? ts.waves * ts.spw : 0, tile ? ts.ntl * 16 : 0, n);
            for (int i = 0; i < n; ++i) {
                const GemmProb &g = Lh.p[i];
                std::printf(" %d %d %d %d %d %d %d %d", g.Kb, g.ksb, g.nslice, g.nblk_strip, g.spb, g.nw, g.block_begin,
                            tile ? gemm_tile_blocks(pl.variant, ps[i].rows, T) : 0);
            }
        }
        std::printf("\n");
    }
    return 0;
}

// gemm_plan.h — GEMM launch planning (DESIGN.md "GEMM planning"): which kernel family runs a launch (small-K, prefill tile, decode), with
// which tile shape, K split, strips and waves per block.  Host-only integer arithmetic on the SHAPE of a launch — no HIP runtime call, no
// pointer is looked at — so that every rule is pinned without a GPU (tests/cpp/gemm_plan_test.cpp, tests/test_gemm_plan_cpp.py).
// The facts about the kernels that the rules depend on are defined here, once; the launchers in rwkv_kernels.hip read them from here.
#pragma once
#include "rwkv_kernels.h"
#include <algorithm>

namespace rwkv {

struct Opd {                        // f16 hi/lo activation operand, B-tiled (rwkv_kernels.hip opd_off): ceil16(Tmax) x ld
    _Float16 *hi = nullptr, *lo = nullptr;
    int ld = 0;
};

struct ProbSpec {                   // one problem of a launch as the engine states it
    const DMat *W = nullptr;
    Opd x;
    int xoff = 0;                   // column offset into x (multiple of 32)
    int act = ACT_NONE, post = POST_NONE;
    const float *bias = nullptr, *m0 = nullptr, *m1 = nullptr;
    int ldm = 0;
    float *out = nullptr;
    int ldo = 0;
    bool partial = false;           // out = partial-sum buffer, K may be split across blocks
    Opd oh;                         // optional operand output
};

// What the rules may look at.
struct ProbShape {
    int rows, K, fmt;
    bool partial;
    bool kcopies;                   // the epilogue lets a prefill launch run K copies into partial slabs: no activation, bias, POST_MIX or operand output
    bool smallk;                    // the epilogue the small-K kernel has: fp32 output only, no post-op, no column offset into X
};
inline ProbShape shape_of(const ProbSpec &s) {
    return {s.W->rows, s.W->K, s.W->fmt, s.partial, s.post != POST_MIX && s.act == ACT_NONE && !s.bias && !s.oh.hi,
            s.xoff == 0 && s.out && !s.oh.hi && s.post == POST_NONE};
}

// Operands and epilogue of one problem; the geometry fields are the planner's.
inline void fill_prob(GemmProb &g, const ProbSpec &s, long pstride) {
    g.W = s.W->data; g.S = s.W->scales; g.fmt = s.W->fmt; g.rows = s.W->rows; g.K = s.W->K;
    g.xhi = s.x.hi + (s.xoff >> 5) * 512; g.xlo = s.x.lo ? s.x.lo + (s.xoff >> 5) * 512 : nullptr; g.ldx = s.x.ld;   // column offset = whole k-tiles
    g.act = s.act; g.post = s.post; g.bias = s.bias; g.m0 = s.m0; g.m1 = s.m1; g.ldm = s.ldm;
    g.out_f32 = s.out; g.ldo = s.ldo; g.partial_stride = pstride;
    g.out_hi = s.oh.hi; g.out_lo = s.oh.lo; g.ldh = s.oh.ld;
}

// ------------------------------------------------------------------------------------------------
// kernel facts
// ------------------------------------------------------------------------------------------------
// decode GEMM (gemm_kernel<NT, KSW, HILO, SHOT, TAIL>): token tiles per pass and 32-k steps per wave for a step of T rows
inline void gemm_variant(int T, bool hilo, int &NT, int &KSW) {
    // Every variant runs 256-k waves (ten per block at K = 2560): a wave's loads return in order and what a CU can pull from HBM grows with
    // its waves, not with the loads each keeps in flight (profiles/r3_exp_stream_waves_x_loads.log: 27 MB over 256 workgroups: 5 waves
    // 8.6-10.8 us, 10 waves 6.9-8.0, 16 waves 6.8-7.1 whatever the depth).  (The 512-k form and its LayerNorm-prologue launch lost that
    // A/B in round 3 and were removed in round 5.)
    KSW = 8;
    // hi + lo operands (Precision::Fp32, or a promoted launch): 17+ rows run two token tiles per pass in 512-thread blocks (128 X registers, the
    // register shape of the four-tile variant) — one pass over the weights for up to 32 rows instead of one per 16
    if (hilo) NT = T <= 16 ? 1 : 2;
    else if (T <= 16) NT = 1;
    else if (T <= 32) NT = 2;
    else NT = 4;                                                  // 33..64 rows in ONE pass over the weights (128 X registers)
}
inline int gemm_variant_max_waves(int NT, int, bool hilo = false) { return (NT == 4 || (NT == 2 && hilo)) ? GEMM_MAX_WAVES_K16 : GEMM_MAX_WAVES; }
// rounds of 256 k a wave can hold at once (single shot): X registers vs the VGPR budget
inline int gemm_max_rounds(int fmt, int NT, bool hilo) { return (NT == 4 || (NT == 2 && hilo)) ? 2 : (fmt == W_F16 ? 2 : ((NT == 2 || hilo) ? 3 : 4)); }

constexpr int SK_KMAX = 320;                              // small-K kernel (smallk_kernel): the longest K a wave keeps in registers

// Prefill tile shapes, largest first: X(waves, strips per wave, n-tiles of 16 tokens, k per chunk, kind, shape number).
// kind 0: gemm_tile_kernel, X tiles through registers; 1: gemm_tile_kernel, X tiles by global_load_lds.
#define GEMM_TILE_CHUNKED(X) X(8, 2, 8, 128, 0, 0) X(8, 1, 8, 128, 0, 1) X(4, 1, 8, 128, 0, 2) X(4, 1, 4, 128, 0, 3) X(4, 1, 4, 256, 0, 4) \
                             X(8, 1, 8, 256, 0, 5) X(4, 1, 4, 256, 1, 6) X(4, 2, 4, 128, 1, 7) X(4, 2, 8, 128, 1, 8) X(8, 2, 8, 128, 1, 9)
// kind 2: the software-pipelined kernel (gemm_tile3_kernel<n-tiles>), plain operands; 3: the same for hi + lo operands (gemm_tile4_kernel)
#define GEMM_TILE_PIPELINED(X) X(4, 2, 8, 128, 2, 10) X(4, 2, 4, 128, 2, 11) X(4, 2, 4, 128, 3, 12)
struct TileShape { int waves, spw, ntl, kc, kind; };
#define GEMM_TILE_ROW(w, p, n, k, kind, i) {w, p, n, k, kind},
constexpr TileShape kTileShapes[] = {GEMM_TILE_CHUNKED(GEMM_TILE_ROW) GEMM_TILE_PIPELINED(GEMM_TILE_ROW)};
#undef GEMM_TILE_ROW
constexpr int GEMM_TILE_SHAPES = (int)(sizeof(kTileShapes) / sizeof(kTileShapes[0]));
constexpr int GEMM_TILE_MIN_T = 193;                     // measured crossover (V6-3B Int8): up to 192 rows the decode kernel's 64-row passes win or tie
constexpr int GEMM_TILE3 = 10;                            // the pipelined 128x128 kernel (non-hi/lo operands, K % 128 == 0)
constexpr int GEMM_TILE3_64 = 11;                         // the same pipeline on 128 rows x 64 tokens (steps of a few hundred rows)
constexpr int GEMM_TILE4_HILO = 12;                       // the software-pipelined kernel for hi + lo operands on 128 rows x 64 tokens (round 6; K % 128 == 0)
inline int gemm_tile_blocks(int shape, int rows, int T) {
    const int strips = kTileShapes[shape].waves * kTileShapes[shape].spw, bt = kTileShapes[shape].ntl * 16;
    return ((rows / 16 + strips - 1) / strips) * ((T + bt - 1) / bt);
}
inline bool gemm_tile_pipelined(int shape) { return kTileShapes[shape].kind >= 2; }
inline bool gemm_tile3_supported(bool hilo, int K) { return !hilo && K % 128 == 0; }
inline bool gemm_tile4_supported(bool hilo, int K) { return hilo && K % 128 == 0; }
inline bool gemm_tile_shape_supported(int shape, bool hilo, int K) {
    if (shape == 5 && hilo) return false;                // 128 tokens x 256-k chunks, double-buffered, hi + lo: 256 KiB of LDS
    return shape == GEMM_TILE4_HILO ? gemm_tile4_supported(hilo, K) : (shape >= GEMM_TILE3 ? gemm_tile3_supported(hilo, K) : true);
}

inline void begin_launch(GemmLaunch &Lh, int n, int T) { Lh = GemmLaunch{}; Lh.nprob = n; Lh.T = T; }

// ------------------------------------------------------------------------------------------------
// small-K launches
// ------------------------------------------------------------------------------------------------
// Launches whose every matrix is short in K (V7's second LoRA stage): the output-stationary small-K kernel, one wave per (problem, strip).
// (A launch that has to carry a token-shift commit keeps the decode kernel: the commit rides on its extra block.)
// Decode-shaped steps only: at 32 rows 6.4 -> ~5.5 us (V7-2.9B: -1.0 / -1.7 / -1.7 % per step at 32 / 8 / 1 slots); at 256 and 2048 rows
// the tile kernels, which share X through LDS, are as fast (profiles/r5_exp_smallk_ab.log).
inline bool smallk_eligible(const ProbShape *ps, int n, int T, bool has_commit) {
    if (T > 64 || has_commit) return false;
    for (int i = 0; i < n; ++i)
        if (ps[i].partial || !ps[i].smallk || ps[i].fmt != W_F16 || ps[i].K > SK_KMAX || ps[i].K % 32 || ps[i].rows % 16) return false;
    return true;
}
// block_begin = first (problem, strip) item of a problem, total_blocks = items in all (launch_smallk packs four to a block)
inline void plan_smallk(GemmLaunch &Lh, const ProbShape *ps, int n, int T) {
    begin_launch(Lh, n, T);
    for (int i = 0; i < n; ++i) {
        GemmProb &g = Lh.p[i];
        g.spb = 1; g.nw = 1; g.ksb = 1; g.Kb = ps[i].K; g.nslice = 1; g.nblk_strip = ps[i].rows / 16;
        g.block_begin = Lh.total_blocks;
        Lh.total_blocks += ps[i].rows / 16;
    }
}

// ------------------------------------------------------------------------------------------------
// decode launches
// ------------------------------------------------------------------------------------------------
// Decomposition of one launch: every wave owns KW = KSW*32 k of the block's K range; linear ("partial") problems may split K across `ksb`
// blocks (the consumer row kernel sums the partials); a block walks `spb` strips.  Aim: >= ~1.5 blocks per CU in flight, whole matrix in
// flight at once.  Returns the number of partial slabs the launch writes (1: none), 0 when a linear problem's K cannot be split.
inline int plan_decode(GemmLaunch &Lh, const ProbShape *ps, int n, int T, bool hilo, int force_spb = 0) {
    begin_launch(Lh, n, T);
    int NT, KSW;
    gemm_variant(T, hilo, NT, KSW);
    const int KW = KSW * 32;
    long total_strips = 0;
    for (int i = 0; i < n; ++i) total_strips += ps[i].rows / 16;
    int np = 1, max_nw = 1, lds_items = 1;
    bool shot = true, tail = false;
    for (int i = 0; i < n; ++i) {
        const ProbShape &s = ps[i];
        GemmProb &g = Lh.p[i];
        const int K = s.K, strips = s.rows / 16;
        const int align = s.fmt == W_F16 ? 32 : 256;
        // K split across blocks: mandatory when the range needs more than 16 waves, optional (linear epilogues)
        // to spread small matrices over more CUs
        int ksb = 1;
        auto valid = [&](int b) { return K % b == 0 && (K / b) % align == 0; };
        if (s.partial) {
            // smallest split that gives >= 1.5 blocks per CU (one strip per block), else the largest valid one <= 8
            int best = 0;
            // (round 6: capping the split at 1 or 2 — one or two partial slabs for the next row kernel to sum instead of five — costs 5 % of a 32-slot
            // step: 2.274 -> 2.395 / 2.385 ms, profiles/r6_exp_decode_ab.log)
            for (int b = 1; b <= 8; ++b) {
                if (!valid(b)) continue;
                best = b;
                if ((long)strips * b >= 384) break;
            }
            if (!best) return 0;
            ksb = best;
        }
        const int Kb = K / ksb;
        const int nslice = (Kb + KW - 1) / KW;                 // balanced: every wave owns the same number of slices
        const int maxw = gemm_variant_max_waves(NT, KSW, hilo), per_wave = (nslice + maxw - 1) / maxw;
        int nw = (nslice + per_wave - 1) / per_wave;
        // two-tile hi + lo launches run 512-thread blocks (8 waves): ten 256-k slices balance as five waves with two slices each, but what a CU
        // pulls from HBM grows with its waves — eight waves, two of them with a second slice, stream the first 80 % of the block's bytes at once
        // (Precision::Fp32 at 32 slots 2.587 -> 2.490 ms per step, Fp16 + RWKV_PROMOTE=1 2.307 -> 2.256)
        if (hilo && NT == 2 && per_wave > 1) nw = std::min(maxw, nslice);
        // (Round 6: the two slices beyond the eight waves dealt out as six (slice, strip) items — one strip of a slice per wave instead of two waves
        // walking a whole second slice — is SLOWER: every item pulls its slice's whole operand for a third of the work; 32-slot step 2.274 -> 2.30 ms,
        // Fp32 2.51 -> 2.59, V7 2.38 -> 2.41; profiles/r6_exp_hilo_ragged_items.log.  Not kept.)
        // strips per block: the whole grid should be resident at once (~164 VGPRs -> 12 waves per CU), and a wave's
        // rounds should fit in registers so that every load is issued up-front (single shot); the head matrix is too
        // big for that and runs 8 strips per block, software-pipelined.
        const int sub = KSW / 8, maxr = gemm_max_rounds(s.fmt, NT, hilo);
        const long cap = 256L * std::max(1, 8 / nw);           // measured: 5-wave blocks are resident one per CU
        int spb = (int)((total_strips * ksb + cap - 1) / cap);
        if ((total_strips * ksb + spb - 1) / spb > 1024) spb = 8;            // huge matrices (head): long pipelined blocks
        else if (spb * sub > maxr && strips * ksb <= 64) spb = std::max(1, maxr / sub);   // tiny member of a group
        spb = std::max(1, std::min(spb, 8));
        if (force_spb) spb = force_spb;
        spb = std::min(spb, std::max(1, 150 / (nw * NT)));                     // LDS: spb*nw*NT KiB <= 150 KiB
        g.spb = spb; g.nw = nw; g.ksb = ksb;
        g.Kb = Kb; g.nslice = nslice;
        g.nblk_strip = (strips + spb - 1) / spb;
        g.block_begin = Lh.total_blocks;
        Lh.total_blocks += g.nblk_strip * ksb;
        max_nw = std::max(max_nw, nw);
        if (spb * sub > maxr) shot = false;
        if (Kb % 256) tail = true;
        lds_items = std::max(lds_items, spb * nw);
        if (s.partial) np = ksb;
    }
    Lh.threads = max_nw * 64;
    Lh.lds_items = lds_items;
    // 17..32-row steps over quantised weights: a ring of two rounds in flight per wave instead of every load issued up-front.  A wave that
    // has issued its 16 operand tiles and 12 weight tiles sits in the issue queue for ~3 us (profiles/r4_trace_gemm_timeline_t1_t32.log)
    // and only then starts on a strip that landed long ago; with the ring its dequantisation starts a round earlier: r/k/v/g Int8 at
    // T = 32 10.07 -> 9.74 us, Fk / Fr 10.70 -> 10.48, fp16 and T <= 16 unchanged or slower (profiles/r4_exp_gemm_ring_vs_shot.log).
    bool all_quant = true;
    for (int i = 0; i < n; ++i) all_quant = all_quant && (ps[i].fmt != W_F16 || ps[i].rows <= 256);   // (the decay LoRA's 64 fp16 rows ride along)
    if (NT == 2 && all_quant && !hilo) shot = false;
    Lh.single_shot = shot ? 1 : 0;
    Lh.tail = tail ? 1 : 0;
    return np;
}

// ------------------------------------------------------------------------------------------------
// prefill launches (T >= GEMM_TILE_MIN_T): LDS-tiled MFMA GEMM
// ------------------------------------------------------------------------------------------------
struct TilePlan { int shape, ksplit, threads; };          // threads: block size of the shape (the profile joins the launch log on it)

// Geometry of a tile launch of one shape with `ksplit` copies of the grid over K (the kernels read block_begin, ksb, total_blocks, xcd_map)
inline TilePlan tile_geometry(GemmLaunch &Lh, const ProbShape *ps, int n, int T, int shape, int ksplit) {
    begin_launch(Lh, n, T);
    for (int i = 0; i < n; ++i) {
        GemmProb &g = Lh.p[i];
        g.spb = 16; g.nw = 8; g.ksb = ksplit; g.nblk_strip = 0;
        g.block_begin = Lh.total_blocks;
        Lh.total_blocks += gemm_tile_blocks(shape, ps[i].rows, T) * ksplit;
    }
    Lh.xcd_map = 1;                                             // XCD-banded tile numbering, row-tile-major (rwkv_kernels.hip tg_body)
    return {shape, ksplit, kTileShapes[shape].waves * 64};
}

// Tile shape and K copies of a prefill launch.  kn.tile_shape (RWKV_TILE_SHAPE=0..12) forces a shape where the launch supports it (the parity
// tests force every shape, one engine per shape), kn.tile_ksplit = 0 turns the K copies off, kn.tile_xcd overrides the band order.
inline TilePlan plan_tile(GemmLaunch &Lh, const ProbShape *ps, int n, int T, bool hilo, const Knobs &kn) {
    // 64x64 tiles measured best everywhere (tile_bench): with 256-k chunks while the launch is latency-bound
    // (few blocks: one L2 round trip per chunk dominates), with 128-k chunks (more blocks per CU) once it is
    // throughput-bound.
    const int f_shape = kn.tile_shape;
    long tot64 = 0, t3 = 0;                                      // tiles of the launch on the 64x64 shapes / on the pipelined 128x128 shape
    int maxK = 0;
    bool all_f16 = true, all_nf4 = true, ok3 = true, ok4 = hilo, big_f16 = false, big_not_nf4 = false;
    for (int i = 0; i < n; ++i) {
        const ProbShape &s = ps[i];
        tot64 += gemm_tile_blocks(3, s.rows, T); t3 += gemm_tile_blocks(GEMM_TILE3, s.rows, T);
        maxK = std::max(maxK, s.K);
        all_f16 = all_f16 && s.fmt == W_F16; all_nf4 = all_nf4 && fmt_is_4bit(s.fmt);   // (SF4 is NF4 to every rule: the same bytes, the same instructions)
        ok3 = ok3 && gemm_tile3_supported(hilo, s.K); ok4 = ok4 && gemm_tile4_supported(hilo, s.K);
        if (s.rows <= 512) continue;                            // (the fp16 LoRA stages — V6's decay, V7's w / a / g / v: 64..320 rows — ride along)
        big_f16 = big_f16 || s.fmt == W_F16; big_not_nf4 = big_not_nf4 || !fmt_is_4bit(s.fmt);
    }
    int shape = tot64 <= 1536 ? 4 : 3;
    // fp16 weights fill a wave's registers twice as fast as Int8: the 128-k chunks (more blocks per CU) win at every grid size
    // since the LDS image is in fragment order (rkvg fp16 T = 512: 489 -> 534 TFLOP/s, T = 256: 374 -> 456)
    if (all_f16) shape = 3;
    // NF4 sits in between (a quarter of the bytes per weight, the most dequantisation work): the 128-k chunks win from ~500 tiles
    // (isolated, 3 B width, 256 rows: r/k/v/g 42.0 -> 40.2 us, Fk + Fr 50.8 -> 47.4; Wo / Fv with 160 tiles lose 40 %),
    // profiles/r3_exp_tile_128x64.log
    if (all_nf4 && tot64 >= 512) shape = 3;
    // the direct-to-LDS 128x64 shape (7: two strips per wave, X tiles by global_load_lds) pays only for very large
    // grids: 7B fp16 prefill at chunk 1024 25.9 -> 27.5 k tok/s, but 21.3 -> 17.8 k at chunk 512; the 256x128
    // GLDS shape (9) wins isolated large fp16 GEMMs (404 -> 536 TFLOP/s) and loses the model (small matrices starve)
    // (not for launches whose matrices are all short in K — V7's second-stage LoRA, K = 64..320, four [T][C] outputs: 88 us on that
    // shape at 2048 rows; on the 64x64 shapes V7-2.9B NF4 prefill 74.4 -> 76.5 k tok/s, 64.7 -> 66.5 k at 1024; profiles/r3_exp_shape7_by_k.log)
    if (T >= 1024 && tot64 >= 2500 && maxK >= 1024) shape = 7;
    // The pipelined 128x128 kernel (shape 10) keeps two blocks per CU resident, 512 tiles a round, and runs ~820 TFLOP/s on
    // whole rounds against ~540 for the 64x64 shapes whatever the grid (scripts/tile_bench2.py); a partial last round costs
    // a whole one (blocks left alone on a CU are latency-bound), so it is used when its rounds are at least 60 % full and it has
    // at least 300 tiles: V6-3B chunk 2048 60.8 -> 69.5 k prefill tok/s, V6-7B chunk 1024 30.4 -> 32.7 k.  (Round 3 moved the bar
    // from 65 % / 400 tiles: Wo of the 3 B models at 2048 rows — 320 tiles, 62.5 % of a round — is 75 us on 64x64 tiles and one
    // round of this kernel, ~64 us: 76.4 -> 78.3 k, V7-2.9B NF4 69.2 -> 71.8 k; profiles/r3_exp_tile3_thresholds.log.)
    const long fill_min = 60, rounds = (t3 + 511) / 512;
    if (ok3 && t3 >= 300 && t3 * 100 >= fill_min * rounds * 512) shape = GEMM_TILE3;
    // The pipelined kernel on 128 x 64 tiles (shape 11, round 4) for the NON-linear launches of steps the 128-token tile cannot fill:
    // at 256 rows a 10304-row launch is 160 tiles of 128 x 128 (fewer than CUs) but 324 of 128 x 64, each prefetching four stages
    // ahead where the 64 x 64 shapes prefetch one chunk: r/k/v/g/decay 49.7 -> 40.8 us, Fk / Fr 45.7 -> 40.0 (Int8, 256 rows).
    // Where it pays, measured after the epilogue rewrite (profiles/r4_exp_tile3_128x64.log, last section; V6-3B Int8 / fp16, V7-2.9B
    // NF4, V6-7B fp16): quantised launches at 256 rows (Int8 +5.8 %, NF4 even) and NF4 at 1024 rows (+2.7 %); fp16 at 512 rows (7 B
    // +8 %, 3 B +1 %); everywhere else the 64 x 64 shapes or the 128 x 128 tile are as fast or faster (fp16 at 1024 rows -3 %).
    // The linear launches (Wo, Fv) stay on K copies of 64 x 64 tiles (22 us at 256 rows against 30).
    // ("big": the matrices of more than 512 rows decide)
    const bool linear_launch = n == 1 && ps[0].partial;
    const bool in_range = big_f16 ? (T > 320 && T <= 768) : (T <= 320 || (!big_not_nf4 && T > 768 && T <= 1280));
    if (ok3 && !linear_launch && in_range) shape = GEMM_TILE3_64;
    // hi + lo operands (Precision::Fp32, and the launch classes Precision::Fp16 promotes): the software-pipelined 128 x 64 kernel whenever
    // every K is a multiple of 128 — it fetches and dequantises a weight once for both operand halves: r/k/v/g Int8 46.8 us against 76.5 on
    // the 64x64 shape at 256 rows, 262 against 547 at 2048 (profiles/r6_exp_tile4.log).  (V7's second-stage LoRAs, K = 64..320, stay on 64x64.)
    if (ok4) shape = GEMM_TILE4_HILO;
    if (f_shape >= 0 && f_shape < GEMM_TILE_SHAPES) {
        bool okf = true;
        for (int i = 0; i < n; ++i) okf = okf && gemm_tile_shape_supported(f_shape, hilo, ps[i].K);
        if (okf) shape = f_shape;
        else if (gemm_tile_pipelined(f_shape) && ok4) shape = GEMM_TILE4_HILO;      // a forced pipelined shape means "the pipelined kernel of this operand form"
        else shape = 4;                                                              // (also shape 5 with hi + lo operands: its LDS image does not fit)
    }
    const bool wide_tile = shape == GEMM_TILE3;                                      // 128 x 128 pipelined tiles
    const bool narrow_tile = shape == GEMM_TILE3_64 || shape == GEMM_TILE4_HILO;    // 128 x 64
    // K split of a linear launch on the pipelined kernel (Wo, Fv: one `partial` problem whose output the next row kernel sums
    // anyway): a grid of fewer than 512 tiles costs a whole round of the kernel, so the tiles are replicated over `ksb` K ranges
    // until the rounds are full — 3 x 320 tiles (V6-3B at 2048 rows) fill 94 % of two rounds a third as long (tg3_body).
    int ksplit = 1;
    if ((ok3 || ok4) && kn.tile_ksplit && linear_launch && ps[0].kcopies && (f_shape < 0 || gemm_tile_pipelined(f_shape))) {
        const int K = ps[0].K, G = K / 128;
        double best = wide_tile ? (double)t3 / (((t3 + 511) / 512) * 512) : 0.0;
        if (t3 >= 128 && ok3) {
            // a copy must keep >= 2048 k: the pipeline's ramp and the fp32 slab a tile writes are fixed costs per copy — measured
            // (V6-3B Int8, 2048 rows): Fv (K = 8960) in three copies 200 -> 173 us, Wo (K = 2560) in three copies 67 -> 86 us
            for (int b = 2; b <= 4 && G / b >= 16; ++b) {
                const double fill = (double)(t3 * b) / (((t3 * b + 511) / 512) * 512);
                if (fill > best + 0.10 && fill >= 0.80) { best = fill; ksplit = b; }
            }
        }
        if (narrow_tile) {
            // copies over K until the launch has about one block per CU, a copy keeping >= 768 k
            const long t11 = gemm_tile_blocks(GEMM_TILE3_64, ps[0].rows, T);
            ksplit = 1;
            for (int b = 2; b <= 4 && K / b >= 768 && t11 * (b - 1) < 224; ++b) ksplit = b;
        } else if (ksplit > 1) shape = GEMM_TILE3;
        else if (!wide_tile) {
            // the 64x64 shapes on a step of a few hundred rows: Wo / Fv have fewer tiles than the chip has CUs (160 at 256 rows of
            // the 3 B model); copies over K fill it
            const long t64 = gemm_tile_blocks(shape, ps[0].rows, T);
            // (only below one tile per CU: at 320 tiles — 512 rows — the copies cost more in slabs than they fill: 49.6 -> 47.1 k tok/s)
            if (t64 < 256) for (int b = 2; b <= 4 && K / b >= 768 && t64 * (b - 1) < 448; ++b) ksplit = b;
        }
    }
    const TilePlan tp = tile_geometry(Lh, ps, n, T, shape, ksplit);
    // Order of the XCD bands (round 6, profiles/r6_exp_tile5_and_xcd_order.log).  Row-tile-major (1): every weight byte is fetched by ONE XCD, which walks
    // all token tiles for it.  Token-tile-major (2): an XCD keeps its own token tiles' X rows in its L2 and streams the weights past them.  An
    // estimate by bytes says (2) from ~640 rows on; measured, the blocks of an XCD walk K in near lock-step, so X streams through the L2 once either
    // way: no change for plain operands (r/k/v/g Int8 at 2048 rows 144.5 / 145.8 us), worse with fp16 weights (149 -> 155), and -8 % only where
    // the operand is doubled — hi + lo launches of 2048-row steps (258 -> 238 us).
    if (hilo && T >= 2048 && shape == GEMM_TILE4_HILO) Lh.xcd_map = 2;
    if (kn.tile_xcd >= 0) Lh.xcd_map = kn.tile_xcd;
    return tp;
}

// ------------------------------------------------------------------------------------------------
// one launch: small-K first, then the prefill tiles, then the decode kernel
// ------------------------------------------------------------------------------------------------
enum GemmPath : int { GEMM_SMALLK = 0, GEMM_TILE = 1, GEMM_DECODE = 2 };
constexpr const char *kGemmPathNames[3] = {"smallk", "tile", "decode"};
struct GemmPlan {
    GemmPath path;
    int variant;                    // tile: the shape; decode: 1 = single shot, 0 = ring
    int grid, threads;
    int ksplit;                     // partial slabs the launch writes (1: none); 0: a linear problem's K cannot be split
};
// Fills the geometry of Lh (fill_prob adds the operands); has_commit: the launch carries a token-shift commit (one extra block)
inline GemmPlan plan_gemm(GemmLaunch &Lh, const ProbShape *ps, int n, int T, bool hilo, bool has_commit, const Knobs &kn) {
    if (smallk_eligible(ps, n, T, has_commit)) {
        plan_smallk(Lh, ps, n, T);
        return {GEMM_SMALLK, 0, (Lh.total_blocks + 3) / 4, 256, 1};
    }
    if (T >= GEMM_TILE_MIN_T && !kn.no_tile) {
        const TilePlan tp = plan_tile(Lh, ps, n, T, hilo, kn);
        return {GEMM_TILE, tp.shape, Lh.total_blocks, tp.threads, tp.ksplit};
    }
    const int np = plan_decode(Lh, ps, n, T, hilo);
    return {GEMM_DECODE, Lh.single_shot, Lh.total_blocks + (has_commit ? 1 : 0), Lh.threads, np};
}

}  // namespace rwkv

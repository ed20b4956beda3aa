// sample_probe.hip — stand-alone driver of the sampling and vocabulary-row kernels for tests/test_gpu_sample_exact.py (DESIGN.md "Sampling
// and vocabulary-row probe").  Not part of librwkv_hip.so: it links the kernel objects the build leaves in ai00_server_amd/csrc and calls
// only the public launchers launch_nucleus, launch_softmax, launch_score_rows, launch_argmax, launch_logit_adjust and launch_logit_mask,
// ONE launch per case — a sampler case is launched a second time into a second pair of output buffers (the two must agree in every bit).
//
//   sample_probe <cases.bin> <results.bin>     one JSON line per case on stdout: the launcher arguments that went in
//
// cases.bin (little-endian), tests/sample_cases.py write_cases:
//   i32 magic 'SPRB', i32 ncases, then per case
//     i32 name_len, char name[name_len], i32 kind (K_*), i32 nparam, i64 param[nparam] (the order of PARAMS below), i32 nbuf, then per buffer
//       i32 role (R_*), i32 esize (1 | 4), i32 flags (1: copied back, 2: no bytes follow, the probe fills the pattern of esize),
//       i64 nbytes (the whole allocation, guard bands and spare rows included), i64 off (byte offset of the pointer the launcher gets, a
//       multiple of 4; of 16 for logits and allow), u8 image[nbytes] unless flags & 2
//   A role that is absent is a null pointer.
// results.bin: per case, every buffer with flags & 1, WHOLE, in the order of the case file.
// Patterns: 0x7FC0DEAD (4-byte elements: a NaN as a float, an impossible token as an int) / 0xAD (bytes).  Every case is validated BEFORE
// anything is launched: every index the kernels form from the case's fields lies inside the buffer allocated for it, every logits block has
// a spare row on both sides, and a sampler row holds at least one finite entry and neither +inf nor NaN (anything else is outside the
// engine's contract: refused with the case's name).  Every HIP call is checked; the first error ends the process with a non-zero status.
#include "../../ai00_server_amd/csrc/rwkv_kernels.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace rwkv;

#define HIP_OK(call)                                                                                        \
    do {                                                                                                    \
        const hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                             \
            std::fprintf(stderr, "sample_probe: %s -> %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            std::fflush(stdout);                                                                            \
            std::exit(3);                                                                                   \
        }                                                                                                   \
    } while (0)

constexpr uint32_t SENT32 = 0x7FC0DEADu;
constexpr uint8_t SENT8 = 0xADu;
constexpr int64_t GUARD = 256;                                         // elements on both sides of every buffer

enum Kind { K_NUCLEUS = 0, K_SOFTMAX, K_SCORE, K_ARGMAX, K_ADJUST, K_MASK, K_COUNT };
enum Role { R_LOGITS = 0, R_SP, R_OUT_TOK, R_OUT_PROB, R_OUT_TOK2, R_OUT_PROB2, R_OUT, R_TARGETS, R_SCRATCH_V, R_SCRATCH_I, R_ROWS, R_TOKS, R_VALS, R_ALLOW, R_COUNT };
static const char *const PARAMS[K_COUNT][8] = {
    {"n_rows", "V", "any_nucleus_typical", "any_mirostat", "any_wide", nullptr},
    {"n_rows", "V", nullptr},
    {"n_rows", "V", nullptr},
    {"n_rows", "V", nullptr},
    {"n_rows", "V", "n", nullptr},
    {"n_rows", "V", "n", nullptr},
};
static const int NPARAM[K_COUNT] = {5, 2, 2, 2, 3, 3};
static const char *const KIND_NAME[K_COUNT] = {"nucleus", "softmax", "score_rows", "argmax", "logit_adjust", "logit_mask"};
static_assert(sizeof(SampleRow) == 24, "the case file carries SampleRow as six 4-byte words");

struct Buf {
    int role = 0, esize = 0, flags = 0;
    int64_t nbytes = 0, off = 0;
    std::vector<uint8_t> host;
    void *dev = nullptr;
};
struct Case {
    std::string name;
    int kind = 0;
    std::vector<int64_t> p;
    std::vector<Buf> b;
    const Buf *find(int role) const {
        for (const Buf &x : b) if (x.role == role) return &x;
        return nullptr;
    }
    template <class T> T *ptr(int role) const { const Buf *x = find(role); return x ? (T *)((char *)x->dev + x->off) : nullptr; }
    template <class T> const T *host(int role) const { const Buf *x = find(role); return x ? (const T *)(x->host.data() + x->off) : nullptr; }
};

struct Reader {
    FILE *f;
    void get(void *dst, size_t bytes) {
        if (bytes && std::fread(dst, 1, bytes, f) != bytes) { std::fprintf(stderr, "sample_probe: case file ends early\n"); std::exit(2); }
    }
    int32_t i32() { int32_t v; get(&v, 4); return v; }
    int64_t i64() { int64_t v; get(&v, 8); return v; }
};

[[noreturn]] static void refuse(const Case &c, const std::string &why) {
    std::fprintf(stderr, "sample_probe: case %s refused before any launch: %s\n", c.name.c_str(), why.c_str());
    std::exit(4);
}
#define REQUIRE(c, cond) do { if (!(cond)) refuse(c, #cond); } while (0)

// `n` elements of `esize` bytes are reachable from the pointer of `role` with a guard band behind them (the role must exist unless optional)
static void need(const Case &c, int role, int64_t n, int esize, bool optional = false) {
    const Buf *x = c.find(role);
    if (!x) { if (optional) return; refuse(c, "missing buffer, role " + std::to_string(role)); }
    if (x->esize != esize || n < 0 || x->off < GUARD * esize || x->off + (n + GUARD) * esize > x->nbytes)
        refuse(c, "buffer of role " + std::to_string(role) + " is too small for " + std::to_string(n) + " elements between guard bands");
}
// a block of `rows` rows of `w` elements with one spare row before and one behind, inside the guard bands
static void need_block(const Case &c, int role, int64_t rows, int64_t w, int esize) {
    const Buf *x = c.find(role);
    if (!x) refuse(c, "missing buffer, role " + std::to_string(role));
    if (x->esize != esize || rows < 1 || w < 1 || x->off < (GUARD + w) * esize || x->off + ((rows + 1) * w + GUARD) * esize > x->nbytes)
        refuse(c, "block of role " + std::to_string(role) + " has no spare row on both sides of " + std::to_string(rows) + " rows");
}

static void validate(const Case &c) {
    const std::vector<int64_t> &p = c.p;
    for (const Buf &x : c.b) {
        REQUIRE(c, x.role >= 0 && x.role < R_COUNT && (x.esize == 1 || x.esize == 4) && x.off >= 0 && x.off % 4 == 0 && x.off <= x.nbytes);
        if (x.role == R_LOGITS || x.role == R_ALLOW) REQUIRE(c, x.off % 16 == 0);   // read 16 bytes (score_rows, the mask) and 4 bytes (allow) at a time
        int same = 0;
        for (const Buf &y : c.b) same += y.role == x.role;
        REQUIRE(c, same == 1);
    }
    REQUIRE(c, (int)p.size() == NPARAM[c.kind]);
    const int64_t n_rows = p[0], V = p[1];
    REQUIRE(c, n_rows >= 1 && n_rows <= 4096 && V >= 16 && V % 16 == 0 && V <= 65536);
    need_block(c, R_LOGITS, n_rows, V, 4);
    const float *x = c.host<float>(R_LOGITS);
    switch (c.kind) {
    case K_NUCLEUS: {
        REQUIRE(c, (p[2] | p[3] | p[4] | 1) == 1);
        need_block(c, R_SP, n_rows, 6, 4);
        need(c, R_OUT_TOK, n_rows, 4); need(c, R_OUT_TOK2, n_rows, 4);
        need(c, R_OUT_PROB, n_rows, 4, true); need(c, R_OUT_PROB2, n_rows, 4, true);
        REQUIRE(c, !c.find(R_OUT_PROB) == !c.find(R_OUT_PROB2));
        const SampleRow *sp = c.host<SampleRow>(R_SP);
        for (int64_t r = 0; r < n_rows; ++r) {
            const int kind = sp[r].kind & 3;
            REQUIRE(c, (sp[r].kind & ~(3 | SAMPLE_WIDE)) == 0 && kind != 3);
            REQUIRE(c, std::isfinite(sp[r].top_p) && std::isfinite(sp[r].tau) && std::isfinite(sp[r].temperature) && sp[r].temperature > 0.f);
            REQUIRE(c, sp[r].uniform >= 0.f && sp[r].uniform <= 1.f && sp[r].top_k >= 0 && sp[r].top_k <= V);
            int64_t finite = 0;
            for (int64_t i = 0; i < V; ++i) {
                const float v = x[r * V + i];
                if (v != v || v == INFINITY) refuse(c, "row " + std::to_string(r) + " holds NaN or +inf: outside the sampler's contract");
                finite += v != -INFINITY;
            }
            if (!finite) refuse(c, "row " + std::to_string(r) + " holds nothing but -inf: outside the sampler's contract");
        }
        break;
    }
    case K_SOFTMAX:
        need_block(c, R_OUT, n_rows, V, 4);
        break;
    case K_SCORE: {
        need(c, R_TARGETS, n_rows, 4); need(c, R_OUT, n_rows, 4);
        const uint32_t *t = c.host<uint32_t>(R_TARGETS);
        for (int64_t r = 0; r < n_rows; ++r) REQUIRE(c, t[r] < (uint32_t)V || t[r] == 0xFFFFFFFFu);   // a token of the row, or RWKV_SCORE_SKIP
        break;
    }
    case K_ARGMAX:
        need(c, R_OUT, n_rows, 4); need(c, R_SCRATCH_V, n_rows * 32, 4); need(c, R_SCRATCH_I, n_rows * 32, 4);
        break;
    case K_ADJUST: {
        const int64_t n = p[2];
        REQUIRE(c, n >= 1 && n <= 65536);
        need(c, R_ROWS, n, 4); need(c, R_TOKS, n, 4); need(c, R_VALS, n, 4);
        const int *rows = c.host<int>(R_ROWS);
        for (int64_t i = 0; i < n; ++i) REQUIRE(c, rows[i] >= 0 && rows[i] < n_rows);   // toks outside [0, V) are ignored by the kernel; rows are not
        break;
    }
    case K_MASK: {
        const int64_t n = p[2];
        REQUIRE(c, n >= 1 && n <= n_rows && V % 4 == 0);
        need(c, R_ROWS, n, 4); need(c, R_ALLOW, n * V, 1);
        const int *rows = c.host<int>(R_ROWS);
        std::vector<char> used(n_rows, 0);
        for (int64_t j = 0; j < n; ++j) { REQUIRE(c, rows[j] >= 0 && rows[j] < n_rows && !used[rows[j]]); used[rows[j]] = 1; }
        break;
    }
    default: refuse(c, "unknown kind");
    }
}

static void launch(const Case &c, hipStream_t s, int round) {
    const std::vector<int64_t> &p = c.p;
    const int n_rows = p[0], V = p[1];
    switch (c.kind) {
    case K_NUCLEUS:
        launch_nucleus(c.ptr<float>(R_LOGITS), n_rows, V, c.ptr<SampleRow>(R_SP), p[2] != 0, p[3] != 0, p[4] != 0,
                       c.ptr<int>(round ? R_OUT_TOK2 : R_OUT_TOK), c.ptr<float>(round ? R_OUT_PROB2 : R_OUT_PROB), s);
        break;
    case K_SOFTMAX: launch_softmax(c.ptr<float>(R_LOGITS), c.ptr<float>(R_OUT), n_rows, V, s); break;
    case K_SCORE: launch_score_rows(c.ptr<float>(R_LOGITS), c.ptr<unsigned>(R_TARGETS), c.ptr<float>(R_OUT), n_rows, V, s); break;
    case K_ARGMAX: launch_argmax(c.ptr<float>(R_LOGITS), n_rows, V, c.ptr<int>(R_OUT), c.ptr<float>(R_SCRATCH_V), c.ptr<int>(R_SCRATCH_I), s); break;
    case K_ADJUST: launch_logit_adjust(c.ptr<float>(R_LOGITS), V, c.ptr<int>(R_ROWS), c.ptr<int>(R_TOKS), c.ptr<float>(R_VALS), (int)p[2], s); break;
    default: launch_logit_mask(c.ptr<float>(R_LOGITS), V, c.ptr<int>(R_ROWS), c.ptr<unsigned char>(R_ALLOW), (int)p[2], s); break;
    }
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: sample_probe <cases.bin> <results.bin>\n"); return 2; }
    FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) { std::fprintf(stderr, "sample_probe: cannot read %s\n", argv[1]); return 2; }
    Reader rd{fi};
    if (rd.i32() != 0x42525053) { std::fprintf(stderr, "sample_probe: bad magic\n"); return 2; }
    const int ncases = rd.i32();
    if (ncases < 0 || ncases > 4096) { std::fprintf(stderr, "sample_probe: bad case count\n"); return 2; }
    std::vector<Case> cases(ncases);
    for (Case &c : cases) {
        const int nl = rd.i32();
        if (nl < 0 || nl > 256) { std::fprintf(stderr, "sample_probe: bad name length\n"); return 2; }
        c.name.resize(nl); rd.get(&c.name[0], nl);
        c.kind = rd.i32();
        const int np = rd.i32();
        if (c.kind < 0 || c.kind >= K_COUNT || np < 0 || np > 8) { std::fprintf(stderr, "sample_probe: bad case header\n"); return 2; }
        c.p.resize(np); rd.get(c.p.data(), (size_t)np * 8);
        const int nb = rd.i32();
        if (nb < 0 || nb > R_COUNT) { std::fprintf(stderr, "sample_probe: bad buffer count\n"); return 2; }
        c.b.resize(nb);
        for (Buf &x : c.b) {
            x.role = rd.i32(); x.esize = rd.i32(); x.flags = rd.i32(); x.nbytes = rd.i64(); x.off = rd.i64();
            if (x.nbytes <= 0 || x.nbytes >= (int64_t)1 << 31 || (x.esize != 1 && x.esize != 4) || x.nbytes % x.esize) { std::fprintf(stderr, "sample_probe: bad buffer header\n"); return 2; }
            x.host.resize(x.nbytes);
            if (x.flags & 2) {
                if (x.esize == 4) for (int64_t i = 0; i < x.nbytes / 4; ++i) ((uint32_t *)x.host.data())[i] = SENT32;
                else std::memset(x.host.data(), SENT8, x.nbytes);
            } else rd.get(x.host.data(), x.nbytes);
        }
    }
    std::fclose(fi);
    for (const Case &c : cases) validate(c);                           // all of them, before the GPU is touched

    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) { std::fprintf(stderr, "sample_probe: cannot write %s\n", argv[2]); return 2; }
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    for (Case &c : cases) {
        for (Buf &x : c.b) {
            HIP_OK(hipMalloc(&x.dev, x.nbytes));
            HIP_OK(hipMemcpy(x.dev, x.host.data(), x.nbytes, hipMemcpyHostToDevice));
        }
        for (int round = 0; round < (c.kind == K_NUCLEUS ? 2 : 1); ++round) {
            launch(c, s, round);
            HIP_OK(hipGetLastError());
            HIP_OK(hipStreamSynchronize(s));
        }
        for (Buf &x : c.b) {
            if (x.flags & 1) {
                HIP_OK(hipMemcpy(x.host.data(), x.dev, x.nbytes, hipMemcpyDeviceToHost));
                if (std::fwrite(x.host.data(), 1, x.nbytes, fo) != (size_t)x.nbytes) { std::fprintf(stderr, "sample_probe: short write\n"); return 2; }
            }
            HIP_OK(hipFree(x.dev));
            x.dev = nullptr;
            std::vector<uint8_t>().swap(x.host);
        }
        std::printf("{\"case\": \"%s\", \"launcher\": \"%s\"", c.name.c_str(), KIND_NAME[c.kind]);
        for (size_t i = 0; i < c.p.size() && PARAMS[c.kind][i]; ++i) std::printf(", \"%s\": %lld", PARAMS[c.kind][i], (long long)c.p[i]);
        std::printf("}\n");
        std::fflush(stdout);
    }
    HIP_OK(hipStreamDestroy(s));
    if (std::fclose(fo) != 0) { std::fprintf(stderr, "sample_probe: close failed\n"); return 2; }
    return 0;
}

// sample_probe.hip — stand-alone driver of the sampling and vocabulary-row kernels for tests/test_gpu_sample_exact.py (DESIGN.md "Sampling
// and vocabulary-row probe").  Not part of librwkv_hip.so: it links the kernel objects the build leaves in ai00_server_amd/csrc and calls
// only the public launchers launch_nucleus, launch_softmax, launch_score_rows, launch_argmax, launch_logit_adjust and launch_logit_mask,
// ONE launch per case — a sampler case is launched a second time into a second pair of output buffers (the two must agree in every bit).
//
//   sample_probe <cases.bin> <results.bin>     one JSON line per case on stdout: the launcher arguments that went in
//
// The case file, the result file, the patterns and the order of work per case are those of every role-buffer probe: DESIGN.md "Probe container"
// (tests/cpp/probe_case.h, probe_common.h).  Here: elements of 1 | 4 bytes, spare rows inside `nbytes`, `off` a multiple of 4 (of 16 for logits
// and allow), and the validation of every case BEFORE anything is launched: every index the kernels form from the case's fields lies inside
// the buffer allocated for it, every logits block has a spare row on both sides, and a sampler row holds at least one finite entry and neither
// +inf nor NaN (anything else is outside the engine's contract: refused with the case's name).
#include "../../ai00_server_amd/csrc/rwkv_kernels.h"
#include "probe_common.h"
#include <cmath>

using namespace rwkv;

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

// `n` elements of `esize` bytes are reachable from the pointer of `role` with a guard band behind them (the role must exist unless optional)
static void need_g(const Case &c, int role, int64_t n, int esize, bool optional = false) { need(c, role, n, esize, optional, GUARD); }
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
        need_g(c, R_OUT_TOK, n_rows, 4); need_g(c, R_OUT_TOK2, n_rows, 4);
        need_g(c, R_OUT_PROB, n_rows, 4, true); need_g(c, R_OUT_PROB2, n_rows, 4, true);
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
        need_g(c, R_TARGETS, n_rows, 4); need_g(c, R_OUT, n_rows, 4);
        const uint32_t *t = c.host<uint32_t>(R_TARGETS);
        for (int64_t r = 0; r < n_rows; ++r) REQUIRE(c, t[r] < (uint32_t)V || t[r] == 0xFFFFFFFFu);   // a token of the row, or RWKV_SCORE_SKIP
        break;
    }
    case K_ARGMAX:
        need_g(c, R_OUT, n_rows, 4); need_g(c, R_SCRATCH_V, n_rows * 32, 4); need_g(c, R_SCRATCH_I, n_rows * 32, 4);
        break;
    case K_ADJUST: {
        const int64_t n = p[2];
        REQUIRE(c, n >= 1 && n <= 65536);
        need_g(c, R_ROWS, n, 4); need_g(c, R_TOKS, n, 4); need_g(c, R_VALS, n, 4);
        const int *rows = c.host<int>(R_ROWS);
        for (int64_t i = 0; i < n; ++i) REQUIRE(c, rows[i] >= 0 && rows[i] < n_rows);   // toks outside [0, V) are ignored by the kernel; rows are not
        break;
    }
    case K_MASK: {
        const int64_t n = p[2];
        REQUIRE(c, n >= 1 && n <= n_rows && V % 4 == 0);
        need_g(c, R_ROWS, n, 4); need_g(c, R_ALLOW, n * V, 1);
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
    launched(s);
}
static void launch_rounds(const Case &c, hipStream_t s) {
    for (int round = 0; round < (c.kind == K_NUCLEUS ? 2 : 1); ++round) launch(c, s, round);
}

static void fields(const Case &c) {
    std::printf(", \"launcher\": \"%s\"", KIND_NAME[c.kind]);
    for (size_t i = 0; i < c.p.size() && PARAMS[c.kind][i]; ++i) std::printf(", \"%s\": %lld", PARAMS[c.kind][i], (long long)c.p[i]);
}

int main(int argc, char **argv) {
    return probe_main<Case>(argc, argv, ProbeSpec{"sample_probe", 0x42525053, K_COUNT, 8, R_COUNT, 1}, validate, launch_rounds, fields);
}


// topn_probe.hip — stand-alone driver of launch_topn_rows for tests/test_gpu_topn_exact.py (DESIGN.md 3.8 "Top-n lists").  Not part of
// librwkv_hip.so: it links the kernel objects the build leaves in ai00_server_amd/csrc and calls the public launcher, ONE launch per case.
//
//   topn_probe <cases.bin> <results.bin>     one JSON line per case on stdout: the launcher arguments that went in
//
// The case file, the result file, the patterns and the order of work per case are those of every role-buffer probe: DESIGN.md "Probe container"
// (tests/cpp/probe_case.h, probe_common.h).  Here: elements of 4 bytes, spare rows inside `nbytes`, `off` a multiple of 4 (of 16 for the logits
// and the side copy of the rows), and the validation of every case BEFORE anything is launched: every index the kernel forms from the case's
// fields lies inside the buffer allocated for it, and every block has a spare row on both sides.
#include "../../ai00_server_amd/csrc/rwkv_kernels.h"
#include "probe_common.h"

using namespace rwkv;

constexpr int64_t GUARD = 256;                                         // elements on both sides of every buffer

enum Kind { K_TOPN = 0, K_COUNT };
enum Role { R_LOGITS = 0, R_OUT_IDS, R_OUT_LOGP, R_SIDE_MS, R_SIDE_ROWS, R_COUNT };

// a block of `rows` rows of `w` elements with one spare row before and one behind, inside the guard bands
static void need_block(const Case &c, int role, int64_t rows, int64_t w) {
    const Buf *x = c.find(role);
    if (!x) refuse(c, "missing buffer, role " + std::to_string(role));
    if (x->esize != 4 || rows < 1 || w < 1 || x->off < (GUARD + w) * 4 || x->off + ((rows + 1) * w + GUARD) * 4 > x->nbytes)
        refuse(c, "block of role " + std::to_string(role) + " has no spare row on both sides of " + std::to_string(rows) + " rows");
}

static void validate(const Case &c) {
    const std::vector<int64_t> &p = c.p;
    for (const Buf &x : c.b) {
        REQUIRE(c, x.role >= 0 && x.role < R_COUNT && x.esize == 4 && x.off >= 0 && x.off % 4 == 0 && x.off <= x.nbytes);
        if (x.role == R_LOGITS || x.role == R_SIDE_ROWS) REQUIRE(c, x.off % 16 == 0);   // read and written 16 bytes at a time
        int same = 0;
        for (const Buf &y : c.b) same += y.role == x.role;
        REQUIRE(c, same == 1);
    }
    REQUIRE(c, (int)p.size() == 4);
    const int64_t n_rows = p[0], V = p[1], n = p[2], side = p[3];
    REQUIRE(c, n_rows >= 1 && n_rows <= 4096 && V >= 16 && V % 16 == 0 && V <= 65536 && n >= 1 && n <= TOPN_MAX && (side | 1) == 1);
    need_block(c, R_LOGITS, n_rows, V);
    need_block(c, R_OUT_IDS, n_rows, n);
    need_block(c, R_OUT_LOGP, n_rows, n);
    REQUIRE(c, !c.find(R_SIDE_MS) == !side && !c.find(R_SIDE_ROWS) == !side);
    if (side) {
        need_block(c, R_SIDE_MS, n_rows, 2);
        need_block(c, R_SIDE_ROWS, n_rows, V);
    }
}

static void launch(const Case &c, hipStream_t s) {
    const std::vector<int64_t> &p = c.p;
    launch_topn_rows(c.ptr<float>(R_LOGITS), (int)p[2], c.ptr<unsigned>(R_OUT_IDS), c.ptr<float>(R_OUT_LOGP), (int)p[0], (int)p[1], s,
                     c.ptr<float>(R_SIDE_MS), c.ptr<float>(R_SIDE_ROWS));
    launched(s);
}

static void fields(const Case &c) {
    std::printf(", \"launcher\": \"topn_rows\", \"n_rows\": %lld, \"V\": %lld, \"n\": %lld, \"side\": %lld", (long long)c.p[0], (long long)c.p[1],
                (long long)c.p[2], (long long)c.p[3]);
}

int main(int argc, char **argv) {
    return probe_main<Case>(argc, argv, ProbeSpec{"topn_probe", 0x4E504F54, K_COUNT, 4, R_COUNT, 1}, validate, launch, fields);
}

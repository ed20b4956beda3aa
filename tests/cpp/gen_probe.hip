// gen_probe.hip — stand-alone driver of the resident-generation kernels for tests/test_gpu_gen_exact.py (DESIGN.md "Resident-generation
// probe").  Not part of librwkv_hip.so: it links the kernel objects the build leaves in ai00_server_amd/csrc and calls only the public
// launchers launch_gen_pre, launch_gen_topn, launch_gen_mask, launch_gen_pda_mask, launch_gen_post, launch_gen_publish, launch_gen_freeze,
// launch_gen_capture, launch_gen_inject, launch_gen_tokens and launch_gen_handover — one kind per launcher, ONE launch per case.  Two kinds
// more: topn_pair makes launch_gen_topn and then launch_topn_rows on the same rows into second outputs and second side buffers; step makes
// one whole step in the engine's order (rwkv_engine.cpp gen_sample and the mixed step around it: [gen_tokens] [gen_inject] [gen_capture]
// [gen_topn] gen_pre [gen_mask] [gen_pda_mask] launch_nucleus gen_post [gen_publish] gen_freeze, a bracketed launch when its role is there)
// n_steps times, the logits block uploaded again from the case's per-step images in front of each step (the head GEMM is not part of it).
//
//   gen_probe <cases.bin> <results.bin>     one JSON line per case on stdout: the launcher, the instantiation it selected (mixed, stops),
//                                           the shape, and for kind step the launches made
//
// The case file, the result file, the patterns and the order of work per case are those of every role-buffer probe: DESIGN.md "Probe container"
// (tests/cpp/probe_case.h, probe_common.h).  Here: elements of 1 | 4 bytes; the 16-bit planes (tok_end, the automaton's table) travel as byte
// buffers whose `off` is a multiple of 16.  Every role is one member of GenArgs (a missing role is a null pointer), except the MEMORY roles
// that nested pointers point into (dfa_trans, dfa_flags, pda_next, pda_act, pda_flags, cap_mem, shadow_mem, ring).
//
// Nested pointers.  GenSlot, GenStop, GenDfa, GenPda, GenCap, GenWatchDev and the shadow table travel as byte images in 4-byte words.  A pointer member is one
// 64-bit word of the image and holds an OFFSET from the launcher's pointer of its memory role — in floats for cap_mem / shadow_mem, in bytes
// for dfa_trans / dfa_flags / pda_next / pda_act / pda_flags / ring — or -1 for null.  validate() checks every offset and the extent behind it, launch() puts the device
// address (or null) in its place on the device, and after the launch every such word is set to ZERO on the device again, so that the image
// is copied back like any other buffer and its non-pointer words can be compared.  The word positions (in 4-byte words of one entry):
//   GenDfa      [6 words]  trans 0-1 -> dfa_trans, flags 2-3 -> dfa_flags          (state 4, mode 5)
//   GenPda      [44 words] next 32-33 -> pda_next, act 34-35 -> pda_act, flags 36-37 -> pda_flags   (stack 0-31, state 38, depth 39, mode 40, max_depth 41)
//   GenCap      [8 words]  p_state 0-1, p_row 2-3, f_row 4-5, inj_row 6-7 -> cap_mem
//   GenWatchDev [8 words]  ring 0-1 -> ring (must be 0), cancel 2-3 -> ring (must be gen_watch_cancel_off)   (seq 4-5, ring_steps 6)
//   shadow      [2 words]  per slot -> shadow_mem
// The ring lives in a block of hipHostMalloc(hipHostMallocMapped | hipHostMallocCoherent) memory whose device alias hipHostGetDevicePointer
// gives, as in the engine; after the stream synchronise it is read with a plain host copy.
//
// Validation of every case BEFORE anything is launched: every index a kernel can form from the case's fields lies inside its buffer between
// the guard bands — row_slot and out_rows, slot x V rows, the ring cells of run_step (and run_step + 1 for gen_topn of a decode-only
// step), the token table's offsets, automaton states against the number of states, state strides that are multiples of 64 floats,
// V % 16 == 0 and 16 <= V <= 65536 — and the logits block has a spare row on both sides.  A refused case ends the process with status 4.
#include "../../ai00_server_amd/csrc/rwkv_kernels.h"
#include "probe_common.h"
#include <cmath>
#include <cstddef>

using namespace rwkv;

constexpr int64_t GUARD = 256;                                         // elements on both sides of every buffer

enum Kind {
    K_PRE = 0, K_TOPN, K_MASK, K_POST, K_PUBLISH, K_FREEZE, K_CAPTURE, K_INJECT, K_TOKENS, K_HANDOVER, K_TOPN_PAIR, K_PDA_MASK, K_STEP,
    K_COUNT
};
static const char *const KIND_NAME[K_COUNT] = {"gen_pre", "gen_topn", "gen_mask", "gen_post", "gen_publish", "gen_freeze", "gen_capture", "gen_inject",
                                               "gen_tokens", "gen_handover", "topn_pair", "gen_pda_mask", "step"};
enum Param {
    P_V = 0, P_B, P_NROWS, P_T, P_MIXED, P_NTOK, P_STEPS, P_NSX, P_NW, P_FIRST, P_TO_HELD, P_DFA_STATES, P_RING_STEPS, P_N, P_PDA_STATES,
    P_NSTEPS, P_ANY_MIRO,
    P_CANCEL_STEP, P_CANCEL_SLOT,                                      // kind step: the host sets this slot's cancel word in front of this step (-1: never)
    P_COUNT
};
enum Role {
    R_SLOTS = 0, R_DFA, R_TOK_END, R_TOK_OFF, R_TOK_BYTES, R_ROW_SLOT, R_OUT_ROWS, R_HELD, R_LOGITS, R_PENALTY, R_BIAS, R_ROWS, R_SAMP_TOK,
    R_SAMP_PROB, R_FEEDBACK, R_OUT_TOK, R_OUT_PROB, R_RUN_STEP, R_SXA, R_SXF, R_WKV, R_SHADOW, R_TOPN_N, R_TOP_IDS, R_TOP_LOGP, R_TOK_LOGP,
    R_SIDE_MS, R_SIDE_ROWS, R_WATCH, R_CAP, R_TOKEN, R_DFA_TRANS, R_DFA_FLAGS, R_CAP_MEM, R_SHADOW_MEM, R_RING, R_OUT_IDS2, R_OUT_LOGP2,
    R_SIDE_MS2, R_SIDE_ROWS2, R_STOPS, R_PDA, R_PDA_NEXT, R_PDA_ACT, R_PDA_FLAGS, R_LOGITS_STEPS,
    R_COUNT
};
constexpr int SLOT_WORDS = 30, DFA_WORDS = 6, CAP_WORDS = 8, WATCH_WORDS = 8, STOP_WORDS = 392, PDA_WORDS = 44;
static_assert(sizeof(GenSlot) == 4 * SLOT_WORDS && offsetof(GenSlot, seed) == 40 && offsetof(GenSlot, finish) == 64 && offsetof(GenSlot, stop) == 80 &&
                  offsetof(GenSlot, wide) == 112, "the case file carries GenSlot as thirty 4-byte words");
static_assert(sizeof(GenDfa) == 4 * DFA_WORDS && offsetof(GenDfa, flags) == 8 && offsetof(GenDfa, state) == 16, "GenDfa: six words, two pointers first");
static_assert(sizeof(GenStop) == 4 * STOP_WORDS && offsetof(GenStop, buf) == 1024 && offsetof(GenStop, len) == 1536 && offsetof(GenStop, n_str) == 1552,
              "GenStop: eight strings, the buffer, eight lengths, n_str, buf_len");
static_assert(sizeof(GenPda) == 4 * PDA_WORDS && offsetof(GenPda, next) == 128 && offsetof(GenPda, flags) == 144 && offsetof(GenPda, state) == 152 &&
                  offsetof(GenPda, max_depth) == 164, "GenPda: the stack, three pointers, state, depth, mode, max_depth");
static_assert(sizeof(GenCap) == 4 * CAP_WORDS && offsetof(GenCap, inj_row) == 24, "GenCap: four pointers");
static_assert(sizeof(GenWatchDev) == 4 * WATCH_WORDS && offsetof(GenWatchDev, cancel) == 8 && offsetof(GenWatchDev, seq) == 16 &&
                  offsetof(GenWatchDev, ring_steps) == 24, "GenWatchDev: two pointers, the sequence number, ring_steps");
static_assert(sizeof(SampleRow) == 24, "the case file carries SampleRow as six 4-byte words");
static_assert(sizeof(float *) == 8, "a pointer is one 64-bit word of an image");

// `n` elements of `esize` bytes are reachable from the pointer of `role` between guard bands
static void need_g(const Case &c, int role, int64_t n, int esize) { need(c, role, n, esize, false, GUARD); }
static int64_t extent(const Case &c, int role) {                       // elements behind the launcher's pointer, the guard band cut off
    const Buf *x = c.find(role);
    return x ? (x->nbytes - x->off) / x->esize - GUARD : -1;
}
// a block of `rows` rows of `w` elements with one spare row before and one behind, inside the guard bands
static void need_block(const Case &c, int role, int64_t rows, int64_t w, int esize) {
    const Buf *x = c.find(role);
    if (!x) refuse(c, "missing buffer, role " + std::to_string(role));
    if (x->esize != esize || rows < 1 || w < 1 || x->off < (GUARD + w) * esize || x->off + ((rows + 1) * w + GUARD) * esize > x->nbytes)
        refuse(c, "block of role " + std::to_string(role) + " has no spare row on both sides of " + std::to_string(rows) + " rows");
}

// ---- the nested pointers: (image role, byte position in the image's owned part, memory role, bytes per offset unit) ----
struct PtrWord { int role; int64_t at; int mem; int unit; };
static std::vector<PtrWord> ptr_words(const Case &c) {
    std::vector<PtrWord> v;
    const int64_t B = c.p[P_B];
    if (c.find(R_DFA))
        for (int64_t b = 0; b < B; ++b) { v.push_back({R_DFA, b * 24, R_DFA_TRANS, 1}); v.push_back({R_DFA, b * 24 + 8, R_DFA_FLAGS, 1}); }
    if (c.find(R_PDA))
        for (int64_t b = 0; b < B; ++b) for (int k = 0; k < 3; ++k) v.push_back({R_PDA, b * 176 + 128 + 8 * k, R_PDA_NEXT + k, 1});
    if (c.find(R_CAP))
        for (int64_t b = 0; b < B; ++b) for (int k = 0; k < 4; ++k) v.push_back({R_CAP, b * 32 + 8 * k, R_CAP_MEM, 4});
    if (c.find(R_SHADOW)) for (int64_t b = 0; b < B; ++b) v.push_back({R_SHADOW, b * 8, R_SHADOW_MEM, 4});
    if (c.find(R_WATCH)) { v.push_back({R_WATCH, 0, R_RING, 1}); v.push_back({R_WATCH, 8, R_RING, 1}); }
    return v;
}
static int64_t ptr_off(const Case &c, const PtrWord &w) {
    int64_t o;
    std::memcpy(&o, c.host<uint8_t>(w.role) + w.at, 8);
    return o;
}
// the offset behind pointer word `at` of `role` has `n` units of its memory role behind it (or is -1); `align` in units
static int64_t need_ptr(const Case &c, int role, int64_t at, int mem, int64_t n, int64_t align) {
    const PtrWord w{role, at, mem, 0};
    const int64_t o = ptr_off(c, w);
    if (o == -1) return o;
    if (o < 0 || o % align || !c.find(mem) || o + n > extent(c, mem))
        refuse(c, "pointer word at byte " + std::to_string(at) + " of role " + std::to_string(role) + ": offset " + std::to_string(o) + " with " +
                      std::to_string(n) + " units behind it is outside role " + std::to_string(mem));
    return o;
}

static int slot_of(const Case &c, int64_t row) {
    const int *rs = c.host<int>(R_ROW_SLOT);
    return c.p[P_MIXED] ? rs[c.host<int>(R_OUT_ROWS)[row]] : rs[row];
}
static const uint32_t *slot_words(const Case &c, int slot) { return c.host<uint32_t>(R_SLOTS) + (int64_t)slot * SLOT_WORDS; }

// one launcher's needs, with run_step == k when it is launched; in_step: a launch of kind `step`, whose tok_end is gen_mask's own
static void validate_as(const Case &c, int kind, int64_t k, bool in_step) {
    const std::vector<int64_t> &p = c.p;
    const int64_t V = p[P_V], B = p[P_B], n_rows = p[P_NROWS], T = p[P_T], mixed = p[P_MIXED], steps = p[P_STEPS], nsx = p[P_NSX], nw = p[P_NW];
    REQUIRE(c, V >= 16 && V % 16 == 0 && V <= 65536 && B >= 1 && B <= 4096 && (mixed | 1) == 1 && T >= 0 && T <= 4096 && steps >= 0 && steps <= 64);
    REQUIRE(c, nsx >= 0 && nsx % 64 == 0 && nw >= 0 && nw % 64 == 0 && nsx <= (1 << 20) && nw <= (1 << 20));
    if (kind == K_TOKENS || kind == K_HANDOVER) {
        REQUIRE(c, kind == K_TOKENS || T > 0);
        need_g(c, R_ROW_SLOT, T, 4); need_g(c, R_HELD, B, 4); need_g(c, kind == K_TOKENS ? R_TOKEN : R_FEEDBACK, T, 4);
        for (int64_t r = 0; r < T; ++r) REQUIRE(c, c.host<int>(R_ROW_SLOT)[r] >= 0 && c.host<int>(R_ROW_SLOT)[r] < B);
        return;
    }
    need_g(c, R_SLOTS, B * SLOT_WORDS, 4);
    if (kind == K_PUBLISH) {                                         // reads slots, the step's ring cells, run_step and the descriptor
        REQUIRE(c, k >= -1 && k < steps);
        need_g(c, R_OUT_TOK, steps * B, 4); need_g(c, R_OUT_PROB, steps * B, 4); need_g(c, R_WATCH, WATCH_WORDS, 4);
        const int64_t rs = p[P_RING_STEPS];
        REQUIRE(c, rs >= 1 && rs <= GEN_WATCH_MAX_STEPS && c.host<int>(R_WATCH)[6] == rs);
        const int64_t ring = need_ptr(c, R_WATCH, 0, R_RING, (int64_t)gen_watch_bytes((int)rs, (int)B), 16);
        if (ring == -1) return;
        REQUIRE(c, ring == 0 && c.find(R_RING)->esize == 1);
        REQUIRE(c, need_ptr(c, R_WATCH, 8, R_RING, 4 * B, 4) == (int64_t)gen_watch_cancel_off((int)rs, (int)B));
        return;
    }
    // ---- the kinds that walk the rows of the logits block ----
    REQUIRE(c, n_rows >= 1 && n_rows <= B);
    need_g(c, R_ROW_SLOT, mixed ? T : n_rows, 4);
    REQUIRE(c, !c.find(R_OUT_ROWS) == !mixed && (mixed || T == n_rows));
    if (mixed) need_g(c, R_OUT_ROWS, n_rows, 4);
    std::vector<char> seen(B, 0);
    for (int64_t r = 0; r < n_rows; ++r) {
        if (mixed) REQUIRE(c, c.host<int>(R_OUT_ROWS)[r] >= 0 && c.host<int>(R_OUT_ROWS)[r] < T);
        const int s = slot_of(c, r);
        REQUIRE(c, s >= 0 && s < B && !seen[s]);                       // a slot has at most one logits row in a step
        seen[s] = 1;
    }
    const bool rows_v = kind != K_FREEZE && kind != K_POST;        // those two never touch the logits block
    if (rows_v) need_block(c, R_LOGITS, n_rows, V, 4);
    auto live = [&](int64_t r) { return slot_words(c, slot_of(c, r))[16] == 0; };
    switch (kind) {
    case K_PRE: {
        need_g(c, R_ROWS, n_rows * 6, 4); need_g(c, R_PENALTY, B * V, 4);
        bool bias = false;
        for (int64_t r = 0; r < n_rows; ++r) bias |= live(r) && slot_words(c, slot_of(c, r))[18] != 0;
        if (bias || c.find(R_BIAS)) need_g(c, R_BIAS, B * V, 4);
        break;
    }
    case K_TOPN: case K_TOPN_PAIR: {
        const int64_t kk = k + (mixed ? 0 : 1);
        REQUIRE(c, kk >= 0 && kk < steps);
        need_g(c, R_TOPN_N, B, 4); need_g(c, R_TOP_IDS, steps * B * TOPN_MAX, 4); need_g(c, R_TOP_LOGP, steps * B * TOPN_MAX, 4);
        need_g(c, R_SIDE_MS, n_rows * 2, 4); need_g(c, R_SIDE_ROWS, n_rows * V, 4);
        if (kind == K_TOPN_PAIR) {
            const int64_t n = p[P_N];
            REQUIRE(c, n >= 1 && n <= TOPN_MAX);
            need_g(c, R_OUT_IDS2, n_rows * n, 4); need_g(c, R_OUT_LOGP2, n_rows * n, 4); need_g(c, R_SIDE_MS2, n_rows * 2, 4); need_g(c, R_SIDE_ROWS2, n_rows * V, 4);
        }
        break;
    }
    case K_MASK: case K_PDA_MASK: case K_POST: {
        const int64_t nq = p[P_DFA_STATES], npq = p[P_PDA_STATES], n_tok = p[P_NTOK];
        if (kind == K_MASK) REQUIRE(c, c.find(R_DFA) != nullptr);
        if (kind == K_PDA_MASK) REQUIRE(c, c.find(R_PDA) != nullptr);
        if (kind == K_POST) {
            REQUIRE(c, k >= 0 && k < steps);
            need_g(c, R_PENALTY, B * V, 4); need_g(c, R_SAMP_TOK, n_rows, 4); need_g(c, R_SAMP_PROB, n_rows, 4);
            need_g(c, R_OUT_TOK, steps * B, 4); need_g(c, R_OUT_PROB, steps * B, 4);
            need_g(c, mixed ? R_HELD : R_FEEDBACK, mixed ? B : n_rows, 4);
            for (int64_t b = 0; b < B; ++b) REQUIRE(c, (int)slot_words(c, b)[19] >= 0 && (int)slot_words(c, b)[19] <= GEN_MAX_STOP);
            if (c.find(R_TOPN_N)) {
                need_g(c, R_TOPN_N, B, 4); need_g(c, R_TOK_LOGP, steps * B, 4); need_g(c, R_SIDE_MS, n_rows * 2, 4); need_g(c, R_SIDE_ROWS, n_rows * V, 4);
            }
            if (c.find(R_STOPS)) need_g(c, R_STOPS, B * STOP_WORDS, 4);   // every field of a GenStop is clamped by the kernel before it indexes
        }
        REQUIRE(c, n_tok >= 0 && n_tok <= V);
        if (kind != K_POST || c.find(R_STOPS) || c.find(R_PDA)) {    // the token table: offsets ascending and inside the bytes
            need_g(c, R_TOK_OFF, n_tok + 1, 4); REQUIRE(c, c.find(R_TOK_BYTES) && c.find(R_TOK_BYTES)->esize == 1);
            const int64_t nbytes = extent(c, R_TOK_BYTES);
            const uint32_t *o = c.host<uint32_t>(R_TOK_OFF);
            for (int64_t v = 0; v <= n_tok; ++v) REQUIRE(c, (int64_t)(o[v] & ~GEN_TOK_UNKNOWN) <= nbytes && (!v || (o[v - 1] & ~GEN_TOK_UNKNOWN) <= (o[v] & ~GEN_TOK_UNKNOWN)));
        }
        if (c.find(R_DFA) && kind != K_PDA_MASK) {
            need_g(c, R_DFA, B * DFA_WORDS, 4); need_g(c, R_TOK_END, n_rows * V * 2, 1);
            REQUIRE(c, nq >= 2 && nq <= GEN_DFA_MAX_STATES);
            for (int64_t r = 0; r < n_rows; ++r) {
                const int s = slot_of(c, r);
                const int64_t tr = need_ptr(c, R_DFA, s * 24, R_DFA_TRANS, nq * 512, 2), fl = need_ptr(c, R_DFA, s * 24 + 8, R_DFA_FLAGS, nq, 1);
                if (tr == -1) continue;
                REQUIRE(c, fl != -1 && c.find(R_DFA_TRANS)->esize == 1 && c.find(R_DFA_FLAGS)->esize == 1);
                const int state = c.host<int>(R_DFA)[s * DFA_WORDS + 4];
                REQUIRE(c, state >= 0 && state < nq);
                const uint16_t *t = (const uint16_t *)(c.host<uint8_t>(R_DFA_TRANS) + tr);
                for (int64_t i = 0; i < nq * 256; ++i) REQUIRE(c, t[i] < nq);
                if (kind == K_POST && !in_step) {                    // the end states gen_mask left: flags[e] is read for the drawn token's
                    const uint16_t *e = (const uint16_t *)c.host<uint8_t>(R_TOK_END) + r * V;
                    for (int64_t v = 0; v < V; ++v) REQUIRE(c, e[v] < nq);
                }
            }
        }
        if (c.find(R_PDA) && kind != K_MASK) {
            need_g(c, R_PDA, B * PDA_WORDS, 4);
            REQUIRE(c, npq >= 2 && npq <= GEN_PDA_MAX_STATES);
            for (int64_t r = 0; r < n_rows; ++r) {
                const int s = slot_of(c, r);
                const int64_t nx = need_ptr(c, R_PDA, s * 176 + 128, R_PDA_NEXT, npq * 512, 2), ac = need_ptr(c, R_PDA, s * 176 + 136, R_PDA_ACT, npq * 512, 2),
                              fl = need_ptr(c, R_PDA, s * 176 + 144, R_PDA_FLAGS, npq, 1);
                if (nx == -1) continue;
                REQUIRE(c, ac != -1 && fl != -1 && c.find(R_PDA_NEXT)->esize == 1 && c.find(R_PDA_ACT)->esize == 1 && c.find(R_PDA_FLAGS)->esize == 1);
                const int *w = c.host<int>(R_PDA) + s * PDA_WORDS;
                const int state = w[38], depth = w[39], max_depth = w[41];
                REQUIRE(c, state >= 0 && state < npq && depth >= 0 && depth <= GEN_PDA_MAX_DEPTH && max_depth >= 1 && max_depth <= GEN_PDA_MAX_DEPTH);
                const uint16_t *stack = (const uint16_t *)w;
                for (int d = 0; d < depth; ++d) REQUIRE(c, stack[d] < npq);
                const uint16_t *tn = (const uint16_t *)(c.host<uint8_t>(R_PDA_NEXT) + nx), *ta = (const uint16_t *)(c.host<uint8_t>(R_PDA_ACT) + ac);
                for (int64_t i = 0; i < npq * 256; ++i) REQUIRE(c, tn[i] < npq && (ta[i] < npq || ta[i] == GEN_PDA_POP));
            }
        }
        break;
    }
    case K_FREEZE: {
        need_g(c, R_SXA, B * nsx, 4); need_g(c, R_SXF, B * nsx, 4); need_g(c, R_WKV, B * nw, 4); need_g(c, R_SHADOW, B * 2, 4);
        for (int64_t r = 0; r < n_rows; ++r) need_ptr(c, R_SHADOW, slot_of(c, r) * 8, R_SHADOW_MEM, 2 * nsx + nw, 4);
        break;
    }
    case K_CAPTURE: case K_INJECT: {
        need_g(c, R_CAP, B * CAP_WORDS, 4);
        if (kind == K_INJECT) REQUIRE(c, mixed && p[P_FIRST] >= 0 && p[P_FIRST] < n_rows);
        else { need_g(c, R_SXA, B * nsx, 4); need_g(c, R_SXF, B * nsx, 4); need_g(c, R_WKV, B * nw, 4); }
        for (int64_t r = 0; r < n_rows; ++r) {
            const int64_t at = slot_of(c, r) * 32;
            need_ptr(c, R_CAP, at, R_CAP_MEM, 2 * nsx + nw, 4); need_ptr(c, R_CAP, at + 8, R_CAP_MEM, V, 4);
            need_ptr(c, R_CAP, at + 16, R_CAP_MEM, V, 4); need_ptr(c, R_CAP, at + 24, R_CAP_MEM, V, 4);
            if (ptr_off(c, {R_CAP, at + 8, R_CAP_MEM, 4}) != -1) REQUIRE(c, ptr_off(c, {R_CAP, at, R_CAP_MEM, 4}) != -1);   // a prompt row comes with its state
        }
        break;
    }
    default: refuse(c, "unknown kind");
    }
}

static void validate(const Case &c) {
    const std::vector<int64_t> &p = c.p;
    for (const Buf &x : c.b) {
        REQUIRE(c, x.role >= 0 && x.role < R_COUNT && (x.esize == 1 || x.esize == 4) && x.off >= 0 && x.off % 16 == 0 && x.off <= x.nbytes);
        int same = 0;
        for (const Buf &y : c.b) same += y.role == x.role;
        REQUIRE(c, same == 1);
    }
    REQUIRE(c, (int)p.size() == P_COUNT);
    need_g(c, R_RUN_STEP, 1, 4);
    const int64_t k0 = *c.host<int>(R_RUN_STEP);
    if (c.kind != K_STEP) { validate_as(c, c.kind, k0, false); return; }
    // ---- kind step: every launch of every step, with the run_step it will see; then what launch_nucleus needs ----
    const int64_t N = p[P_NSTEPS], V = p[P_V], B = p[P_B], n_rows = p[P_NROWS], mixed = p[P_MIXED];
    REQUIRE(c, N >= 1 && N <= 8 && (p[P_ANY_MIRO] | 1) == 1);
    REQUIRE(c, p[P_CANCEL_STEP] >= -1 && p[P_CANCEL_STEP] < N);
    if (p[P_CANCEL_STEP] >= 0) {                                       // the word lies in the ring the descriptor points at (validated as gen_publish below)
        REQUIRE(c, p[P_CANCEL_SLOT] >= 0 && p[P_CANCEL_SLOT] < B && c.find(R_WATCH) && c.find(R_RING));
        REQUIRE(c, ptr_off(c, {R_WATCH, 0, R_RING, 1}) == 0);
    }
    for (int64_t i = 0; i < N; ++i) {
        const int64_t k = k0 + i + 1;                                  // what gen_post, gen_publish and gen_freeze of step i see
        if (mixed) validate_as(c, K_TOKENS, k - 1, true);
        if (c.find(R_CAP) && mixed && p[P_FIRST] < n_rows) validate_as(c, K_INJECT, k, true);
        if (c.find(R_CAP)) validate_as(c, K_CAPTURE, k, true);
        if (c.find(R_TOPN_N)) validate_as(c, K_TOPN, mixed ? k : k - 1, true);
        validate_as(c, K_PRE, k - 1, true);
        if (c.find(R_DFA)) validate_as(c, K_MASK, k, true);
        if (c.find(R_PDA)) validate_as(c, K_PDA_MASK, k, true);
        validate_as(c, K_POST, k, true);
        if (c.find(R_WATCH)) validate_as(c, K_PUBLISH, k, true);
        validate_as(c, K_FREEZE, k, true);
    }
    need_g(c, R_LOGITS_STEPS, N * n_rows * V, 4);
    const float *x = c.host<float>(R_LOGITS_STEPS);
    for (int64_t r = 0; r < N * n_rows; ++r) {                         // a sampler row: an entry above -inf, neither NaN nor +inf
        int64_t finite = 0;
        for (int64_t i = 0; i < V; ++i) { const float v = x[r * V + i]; REQUIRE(c, v == v && v != INFINITY); finite += v != -INFINITY; }
        REQUIRE(c, finite > 0);
    }
    auto sampler_ok = [&](float top_p, int top_k, float temperature, int kind, float tau) {
        return kind >= 0 && kind <= 2 && std::isfinite(top_p) && std::isfinite(tau) && std::isfinite(temperature) && temperature > 0.f && top_k >= 0 && top_k <= V;
    };
    for (int64_t b = 0; b < B; ++b) {                                  // what gen_pre hands to the sampler, and finite edits of the rows
        const GenSlot *g = (const GenSlot *)slot_words(c, (int)b);
        REQUIRE(c, sampler_ok(g->top_p, g->top_k, g->temperature, g->kind, g->tau) && g->wide == 0 && (p[P_ANY_MIRO] || g->kind != 2));
        REQUIRE(c, std::isfinite(g->presence) && std::isfinite(g->frequency) && std::isfinite(g->decay));
        REQUIRE(c, std::isfinite(g->miro_target) && std::isfinite(g->miro_rate));
        for (int64_t i = 0; i < V; ++i) {
            const uint32_t pb = c.host<uint32_t>(R_PENALTY)[b * V + i];
            REQUIRE(c, pb == GEN_ABSENT || std::isfinite(c.host<float>(R_PENALTY)[b * V + i]));
            if (c.find(R_BIAS)) REQUIRE(c, std::isfinite(c.host<float>(R_BIAS)[b * V + i]));
        }
    }
    const SampleRow *sp = c.host<SampleRow>(R_ROWS);                   // a rider of a decode-only step keeps the row it finds: valid from the start
    for (int64_t r = 0; r < n_rows; ++r) {
        REQUIRE(c, sampler_ok(sp[r].top_p, sp[r].top_k, sp[r].temperature, sp[r].kind, sp[r].tau));
        REQUIRE(c, sp[r].uniform >= 0.f && sp[r].uniform <= 1.f);
    }
}

static GenArgs args_of(const Case &c) {
    GenArgs a{};
    a.slots = c.ptr<GenSlot>(R_SLOTS); a.dfa = c.ptr<GenDfa>(R_DFA); a.tok_end = c.ptr<unsigned short>(R_TOK_END);
    a.tok_off = c.ptr<unsigned>(R_TOK_OFF); a.tok_bytes = c.ptr<unsigned char>(R_TOK_BYTES); a.n_tok = (int)c.p[P_NTOK];
    a.row_slot = c.ptr<int>(R_ROW_SLOT); a.out_rows = c.ptr<int>(R_OUT_ROWS); a.held = c.ptr<int>(R_HELD);
    a.logits = c.ptr<float>(R_LOGITS); a.penalty = c.ptr<float>(R_PENALTY); a.bias = c.ptr<float>(R_BIAS);
    a.rows = c.ptr<SampleRow>(R_ROWS); a.samp_tok = c.ptr<int>(R_SAMP_TOK); a.samp_prob = c.ptr<float>(R_SAMP_PROB);
    a.feedback = c.ptr<int>(R_FEEDBACK); a.out_tok = c.ptr<unsigned>(R_OUT_TOK); a.out_prob = c.ptr<float>(R_OUT_PROB);
    a.run_step = c.ptr<int>(R_RUN_STEP); a.max_batch = (int)c.p[P_B]; a.V = (int)c.p[P_V]; a.n_rows = (int)c.p[P_NROWS];
    a.sxa = c.ptr<float>(R_SXA); a.sxf = c.ptr<float>(R_SXF); a.wkv = c.ptr<float>(R_WKV);
    a.sx_slot_stride = (long)c.p[P_NSX]; a.wkv_slot_stride = (long)c.p[P_NW]; a.shadow = c.ptr<float *>(R_SHADOW);
    a.topn_n = c.ptr<int>(R_TOPN_N); a.top_ids = c.ptr<unsigned>(R_TOP_IDS); a.top_logp = c.ptr<float>(R_TOP_LOGP);
    a.tok_logp = c.ptr<float>(R_TOK_LOGP); a.side_ms = c.ptr<float>(R_SIDE_MS); a.side_rows = c.ptr<float>(R_SIDE_ROWS);
    a.watch = c.ptr<GenWatchDev>(R_WATCH); a.cap = c.ptr<GenCap>(R_CAP); a.stops = c.ptr<GenStop>(R_STOPS); a.pda = c.ptr<GenPda>(R_PDA);
    return a;
}

static void launch(const Case &c, hipStream_t s) {
    const std::vector<int64_t> &p = c.p;
    // the ring: a mapped, coherent host block that holds the role's whole image, guard bands included
    const Buf *ring = c.find(R_RING);
    void *ring_host = nullptr, *ring_dev = nullptr;
    if (ring && (c.kind == K_PUBLISH || c.kind == K_STEP)) {
        HIP_OK(hipHostMalloc(&ring_host, ring->nbytes, hipHostMallocMapped | hipHostMallocCoherent));
        std::memcpy(ring_host, ring->host.data(), ring->nbytes);
        HIP_OK(hipHostGetDevicePointer(&ring_dev, ring_host, 0));
    }
    // offsets -> device addresses, on the device's copy of the images
    const std::vector<PtrWord> words = ptr_words(c);
    for (const PtrWord &w : words) {
        const int64_t o = ptr_off(c, w);
        const Buf *m = c.find(w.mem);
        uint64_t addr = 0;
        if (o != -1 && m) addr = (uint64_t)((w.mem == R_RING && ring_dev ? (char *)ring_dev : (char *)m->dev) + m->off + o * w.unit);
        HIP_OK(hipMemcpy(c.ptr<char>(w.role) + w.at, &addr, 8, hipMemcpyHostToDevice));
    }
    const GenArgs a = args_of(c);
    switch (c.kind) {
    case K_PRE: launch_gen_pre(a, s); break;
    case K_TOPN: launch_gen_topn(a, s); break;
    case K_MASK: launch_gen_mask(a, s); break;
    case K_PDA_MASK: launch_gen_pda_mask(a, s); break;
    case K_POST: launch_gen_post(a, s); break;
    case K_PUBLISH: launch_gen_publish(a, s); break;
    case K_FREEZE: launch_gen_freeze(a, s); break;
    case K_CAPTURE: launch_gen_capture(a, s); break;
    case K_INJECT: launch_gen_inject(a, (int)p[P_FIRST], s); break;
    case K_TOKENS: launch_gen_tokens(c.ptr<int>(R_TOKEN), a.row_slot, a.held, a.run_step, (int)p[P_T], s); break;
    case K_HANDOVER: launch_gen_handover(a.feedback, a.held, a.row_slot, (int)p[P_T], p[P_TO_HELD] != 0, s); break;
    case K_STEP:                                                       // rwkv_engine.cpp gen_sample and the mixed step around it, N times
        for (int64_t i = 0; i < p[P_NSTEPS]; ++i) {
            if (ring_host && i == p[P_CANCEL_STEP]) {                  // the host side of the watch, between two steps (every launch before is synchronised)
                unsigned *cancel = (unsigned *)((char *)ring_host + ring->off + gen_watch_cancel_off((int)p[P_RING_STEPS], (int)p[P_B]));
                __atomic_store_n(cancel + p[P_CANCEL_SLOT], 1u, __ATOMIC_RELEASE);   // as rwkv_gen_watch_cancel stores it: a plain host store
            }
            const size_t block = (size_t)a.n_rows * a.V * 4;           // the head GEMM's part: this step's logits image
            HIP_OK(hipMemcpy(a.logits, c.ptr<char>(R_LOGITS_STEPS) + i * block, block, hipMemcpyDeviceToDevice));
            if (a.out_rows) {                                          // the plan's token array: prompt ids and -1, written anew for every step
                HIP_OK(hipMemcpy(c.ptr<int>(R_TOKEN), c.host<int>(R_TOKEN), (size_t)p[P_T] * 4, hipMemcpyHostToDevice));
                launch_gen_tokens(c.ptr<int>(R_TOKEN), a.row_slot, a.held, a.run_step, (int)p[P_T], s); launched(s);
            }
            if (a.cap && a.out_rows && p[P_FIRST] < a.n_rows) { launch_gen_inject(a, (int)p[P_FIRST], s); launched(s); }
            if (a.cap) { launch_gen_capture(a, s); launched(s); }
            if (a.topn_n) { launch_gen_topn(a, s); launched(s); }
            launch_gen_pre(a, s); launched(s);
            if (a.dfa) { launch_gen_mask(a, s); launched(s); }
            if (a.pda) { launch_gen_pda_mask(a, s); launched(s); }
            launch_nucleus(a.logits, a.n_rows, a.V, a.rows, true, p[P_ANY_MIRO] != 0, false, (int *)a.samp_tok, (float *)a.samp_prob, s);
            launched(s);
            launch_gen_post(a, s); launched(s);
            if (a.watch) { launch_gen_publish(a, s); launched(s); }
            launch_gen_freeze(a, s);
            if (i + 1 < p[P_NSTEPS]) launched(s);
        }
        break;
    default:
        launch_gen_topn(a, s);
        launched(s);
        launch_topn_rows(a.logits, (int)p[P_N], c.ptr<unsigned>(R_OUT_IDS2), c.ptr<float>(R_OUT_LOGP2), a.n_rows, a.V, s, c.ptr<float>(R_SIDE_MS2),
                         c.ptr<float>(R_SIDE_ROWS2));
        break;
    }
    launched(s);
    const uint64_t zero = 0;                                           // the pointer words are nulled again: the images come back comparable
    for (const PtrWord &w : words) HIP_OK(hipMemcpy(c.ptr<char>(w.role) + w.at, &zero, 8, hipMemcpyHostToDevice));
    if (ring_host) {                            // a plain host read of the block, handed to the copy-back through the role's device buffer
        std::vector<uint8_t> got((const uint8_t *)ring_host, (const uint8_t *)ring_host + ring->nbytes);
        HIP_OK(hipMemcpy(ring->dev, got.data(), ring->nbytes, hipMemcpyHostToDevice));
        HIP_OK(hipHostFree(ring_host));
    }
}

static void fields(const Case &c) {
    const std::vector<int64_t> &p = c.p;
    if (c.kind == K_STEP) {
        const bool inject = c.find(R_CAP) && p[P_MIXED] && p[P_FIRST] < p[P_NROWS];
        std::printf(", \"launches\": \"%s%s%s%spre,%s%snucleus,post,%sfreeze x %lld\"", p[P_MIXED] ? "tokens," : "", inject ? "inject," : "",
                    c.find(R_CAP) ? "capture," : "", c.find(R_TOPN_N) ? "topn," : "", c.find(R_DFA) ? "mask," : "", c.find(R_PDA) ? "pda_mask," : "",
                    c.find(R_WATCH) ? "publish," : "", (long long)p[P_NSTEPS]);
    }
    const bool stops = c.find(R_STOPS) && (c.kind == K_POST || c.kind == K_STEP);
    std::printf(", \"launcher\": \"%s\", \"mixed\": %d, \"stops\": %d, \"n_rows\": %lld, \"V\": %lld, \"max_batch\": %lld", KIND_NAME[c.kind],
                (int)(p[P_MIXED] != 0), (int)stops, (long long)p[P_NROWS], (long long)p[P_V], (long long)p[P_B]);
}

int main(int argc, char **argv) {
    return probe_main<Case>(argc, argv, ProbeSpec{"gen_probe", 0x4E454750, K_COUNT, P_COUNT, R_COUNT, 1}, validate, launch, fields);
}

// gen_stop.h — the stop-STRING matcher of the `process` loop (run.rs:855-869, 899-932, 990-1011) as host/device functions.
// Host-only header (no HIP include, like gemm_plan.h / graph_cache.h): gen_post_kernel<., true> (rwkv_kernels.hip) calls exactly these
// functions, one lane per stop string, and tests/cpp/gen_stop_test.cpp compiles the same text with g++ and drives it in the kernel's order.
//
// Per drawn token the reference appends the token's bytes to the request's buffer, walks the WHOLE buffer once per stop string
// (gen_stop_scan), picks one result with `min_by` (gen_stop_merge), splits the buffer there into head | tail, and — unless the request
// finishes — drops the head from the buffer only if it is valid UTF-8 (gen_utf8_valid); otherwise the buffer is kept whole and grows.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef RWKV_HD
#ifdef __HIP__
#define RWKV_HD __host__ __device__
#else
#define RWKV_HD
#endif
#endif

namespace rwkv {

constexpr int GEN_MAX_STOP_STR = 8;     // stop strings per slot (RWKV_GEN_MAX_STOP_STR)
constexpr int GEN_STOP_LEN = 128;       // bytes per stop string
constexpr int GEN_STOP_BUF = 512;       // bytes of buffer per slot; a token whose bytes do not fit hands the slot back (GEN_FIN_HANDBACK)
constexpr int GEN_TOKEN_LEN = 256;      // bytes per token of the token table
constexpr unsigned GEN_TOK_UNKNOWN = 0x80000000u;   // bit of a token-table offset: the id is not in the vocabulary (decode error, run.rs:858-862)
enum : int { GEN_FIN_RUNNING = 0, GEN_FIN_STOP = 1, GEN_FIN_LENGTH = 2, GEN_FIN_HANDBACK = 3 };   // RWKV_GEN_*

struct GenStopScan { int safe; int matched; };              // (index_safe, matched) of run.rs:913 / 924
// what a lane without a stop string contributes: loses against every real result, whichever side it stands on
constexpr GenStopScan GEN_STOP_NONE = {0x7fffffff, 0};

// run.rs:905-924, one stop string over the buffer.  On a mismatch index_safe moves BEHIND the mismatching byte, which is not retried as
// the start of a match: "ab" over "aab" does not match.  A match that ends exactly at the buffer's end counts; an empty string always matches.
RWKV_HD inline GenStopScan gen_stop_scan(const unsigned char *buffer, int n, const unsigned char *stop, int len) {
    int index_safe = 0, index_unsafe = 0;
    while (index_unsafe < n) {
        const int index_stop = index_unsafe - index_safe;
        if (index_stop >= len) return GenStopScan{index_safe, 1};
        const unsigned char out = buffer[index_unsafe], st = stop[index_stop];
        ++index_unsafe;
        if (out != st) index_safe = index_unsafe;
    }
    return GenStopScan{index_safe, index_unsafe - index_safe >= len ? 1 : 0};
}

// run.rs:926-930, `min_by` over two results of which `a` stands EARLIER in the request's list: a matched stop before an unmatched one,
// then the smaller index_safe, and of equals the first (Iterator::min_by).  Associative, so a lane reduction that keeps the order may use it.
RWKV_HD inline GenStopScan gen_stop_merge(GenStopScan a, GenStopScan b) {
    const bool b_less = (b.matched && !a.matched) || (b.matched == a.matched && b.safe < a.safe);
    return b_less ? b : a;
}

// String::from_utf8 (run.rs:1008): the well-formed byte sequences of the Unicode standard (table 3-7) — no overlong form, no surrogate,
// nothing above U+10FFFF, no truncated character at the end.
RWKV_HD inline bool gen_utf8_valid(const unsigned char *p, int n) {
    int i = 0;
    while (i < n) {
        const unsigned c = p[i];
        if (c < 0x80) { ++i; continue; }
        int more;
        unsigned lo = 0x80, hi = 0xBF;                       // range of the SECOND byte
        if (c >= 0xC2 && c <= 0xDF) more = 1;
        else if (c == 0xE0) { more = 2; lo = 0xA0; }
        else if (c >= 0xE1 && c <= 0xEF) { more = 2; if (c == 0xED) hi = 0x9F; }
        else if (c == 0xF0) { more = 3; lo = 0x90; }
        else if (c >= 0xF1 && c <= 0xF3) more = 3;
        else if (c == 0xF4) { more = 3; hi = 0x8F; }
        else return false;
        if (n - i <= more) return false;
        if (p[i + 1] < lo || p[i + 1] > hi) return false;
        for (int k = 2; k <= more; ++k) if ((p[i + k] & 0xC0) != 0x80) return false;
        i += more + 1;
    }
    return true;
}

// The finish decision for one drawn token, in this order (run.rs:990-1011 with the bounded buffer of the device put in):
//   stop_token   token 0, a listed stop token, or an id that is not in the vocabulary          -> STOP
//   !fits        the token's bytes do not fit the buffer: this token cannot be decided here    -> HANDBACK
//   matched                                                                                     -> STOP
//   at_max       the slot has emitted max_tokens                                                -> LENGTH
//   otherwise RUNNING: the caller trims the buffer under the UTF-8 rule
RWKV_HD inline int gen_stop_decide(bool stop_token, bool fits, bool matched, bool at_max) {
    if (stop_token) return GEN_FIN_STOP;
    if (!fits) return GEN_FIN_HANDBACK;
    if (matched) return GEN_FIN_STOP;
    return at_max ? GEN_FIN_LENGTH : GEN_FIN_RUNNING;
}

// The trim of a slot that goes on (run.rs:1008-1010): first byte of the buffer that is kept.
RWKV_HD inline int gen_stop_keep_from(const unsigned char *buffer, int index_safe) {
    return gen_utf8_valid(buffer, index_safe) ? index_safe : 0;
}

}  // namespace rwkv

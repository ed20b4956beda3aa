// gen_pda.h — the stack-automaton constraint of resident generation as host/device functions: a third implementation of the reference's
// `Formatter` trait (`transform` = mask, `update` = advance and maybe halt; sampler/bnf.rs:34-48, run.rs:676-680, 892-897, 990), beside kbnf
// on the host and the byte-level DFA of gen_dfa.h on the device, for what a RETURN-STATE STACK expresses: nested brackets, which is what
// "answer in JSON" needs.  It is not kbnf and no port of it: general context-free grammars stay on the host (rwkv_infer_sample with `allow`).
// Host-only header (no HIP include, like gen_dfa.h): gen_pda_mask_kernel and gen_post_kernel (rwkv_kernels.hip) call exactly these
// functions, so do rwkv_pda_walk / rwkv_pda_allow (rwkv_pda.cpp), and tests/cpp/gen_pda_test.cpp compiles the same text with g++ and drives
// it in the kernels' order.
//
// THE CONTRACT
//   Tables       States 0 .. n_states - 1, n_states <= GEN_PDA_MAX_STATES.  State 0 is DEAD: both of its rows are zero.  Two uint16 planes
//                [n_states][256], `next` and `act`, accepting[n_states], a start state, and max_depth in 1 .. GEN_PDA_MAX_DEPTH.
//   Transitions  For state q and byte b:
//                  act == 0            PLAIN: go to next; next == 0 is dead.
//                  act == GEN_PDA_POP  POP: the next state is the popped entry; an empty stack is dead; `next` is ignored.
//                  any other act       PUSH: act is a live state id and next != 0; push act as the return state and go to next; a stack
//                                      that already holds max_depth entries is dead.
//   Configuration (state, stack of uint16).  LIVE: state != 0.  ACCEPTS: accepting[state] and an empty stack.  END, a per-state flag
//                computed on the host: no plain or push entry with a live target (pops do not count: the stack is empty where it matters).
//   ALLOWED      Token v is allowed in a configuration iff v is in the token table, known, non-empty and not id 0 (gen_dfa.h says why), and
//                walking its bytes ends LIVE — with one addition, THE SPAN RULE: while a token is walked, `low` is the smallest depth
//                reached so far; a push that would make depth - low > GEN_PDA_TOKEN_SPAN makes the token not allowed.  Host and device
//                apply the same rule, so it is part of the language, not an implementation limit: the entries a token owns (those above
//                `low`) always fit a 128-bit shift register, and everything at or below `low` is the configuration's own stack, read only.
//   ADVANCE      A drawn token that is not allowed leaves the configuration where it was and does not halt.
//   HALT         GEN_PDA_HALT_FINAL: the new configuration ACCEPTS and its state is END.  GEN_PDA_HALT_ACCEPT: it ACCEPTS.
//   LIVENESS     (pda_never_stuck, rwkv_pda.h) is what guarantees that no masked row is all -inf, at any depth.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gen_stop.h"   // RWKV_HD, GEN_TOK_UNKNOWN, GEN_TOKEN_LEN

namespace rwkv {

constexpr int GEN_PDA_MAX_STATES = 4096;            // RWKV_PDA_MAX_STATES, DEAD included
constexpr int GEN_PDA_MAX_DEPTH = 64;               // RWKV_PDA_MAX_DEPTH
constexpr int GEN_PDA_TOKEN_SPAN = 8;               // RWKV_PDA_TOKEN_SPAN: entries one token may own; 8 x 16 bits = the shift register below
constexpr unsigned GEN_PDA_POP = 0xFFFFu;           // RWKV_PDA_POP
enum : int { GEN_PDA_HALT_FINAL = 0, GEN_PDA_HALT_ACCEPT = 1 };   // RWKV_PDA_HALT_*
constexpr unsigned char GEN_PDA_ACCEPT = 1, GEN_PDA_END = 2;

// One byte on a REAL stack (rwkv_pda_walk): the state behind byte b, 0 once dead; stack[0 .. *depth) is rewritten in place.
RWKV_HD inline unsigned gen_pda_step(const unsigned short *next, const unsigned short *act, int max_depth, unsigned q, unsigned short *stack,
                                     int *depth, unsigned char b) {
    if (!q) return 0;
    const unsigned a = act[q * 256u + b], n = next[q * 256u + b];
    if (a == 0) return n;
    if (a == GEN_PDA_POP) return *depth > 0 ? stack[--*depth] : 0u;
    if (n == 0 || *depth >= max_depth) return 0;
    stack[(*depth)++] = (unsigned short)a;
    return n;
}

// The flag byte of state q (computed once on the host, when a table is taken in).
RWKV_HD inline unsigned char gen_pda_flags(const unsigned short *next, const unsigned short *act, const unsigned char *accepting, unsigned q) {
    bool live_next = false;
    for (int c = 0; c < 256; ++c) live_next |= act[q * 256u + c] != GEN_PDA_POP && next[q * 256u + c] != 0;
    return (unsigned char)((q && accepting[q] ? GEN_PDA_ACCEPT : 0) | (live_next ? 0 : GEN_PDA_END));
}

// What a token walk leaves: the entries the token owns as a shift register (push = shift 16 bits in at the bottom, pop = shift them
// out: no dynamic indexing, so a kernel keeps it in registers), the lowest depth it reached and the depth it ends at.  depth - low entries
// are owned, the top of the stack in the low 16 bits of `lo`; the stack below `low` is the configuration's, untouched.
struct GenPdaWalk {
    unsigned long long lo, hi;
    int low, depth;
    unsigned state;                                 // 0: the token is not allowed
};

// `n` bytes from (q, base[0 .. depth)) by the transition rules and the span rule above; `base` is only read.
RWKV_HD inline GenPdaWalk gen_pda_token_walk(const unsigned short *next, const unsigned short *act, int max_depth, unsigned q,
                                             const unsigned short *base, int depth, const unsigned char *bytes, int n) {
    GenPdaWalk w{0ull, 0ull, depth, depth, q};
    for (int i = 0; i < n && w.state; ++i) {
        const unsigned at = w.state * 256u + bytes[i];
        const unsigned a = act[at], t = next[at];
        if (a == 0) {
            w.state = t;
        } else if (a == GEN_PDA_POP) {
            if (w.depth > w.low) {                  // an entry of the token's own
                w.state = (unsigned)(w.lo & 0xFFFFu);
                w.lo = (w.lo >> 16) | (w.hi << 48);
                w.hi >>= 16;
                w.depth -= 1;
            } else if (w.depth > 0) {               // below everything the token pushed: the configuration's stack
                w.state = base[w.depth - 1];
                w.depth -= 1;
                w.low = w.depth;
            } else {
                w.state = 0;
            }
        } else {
            if (t == 0 || w.depth >= max_depth || w.depth - w.low >= GEN_PDA_TOKEN_SPAN) {
                w.state = 0;
            } else {
                w.hi = (w.hi << 16) | (w.lo >> 48);
                w.lo = (w.lo << 16) | a;
                w.depth += 1;
                w.state = t;
            }
        }
    }
    return w;
}

// The ALLOWED predicate as the walk of token v from (q, base[0 .. depth)): .state == 0 when the token is not allowed (see gen_dfa_token_end
// for the table's form and for why token 0, empty and unknown tokens never are).
RWKV_HD inline GenPdaWalk gen_pda_token_end(const unsigned short *next, const unsigned short *act, int max_depth, unsigned q,
                                            const unsigned short *base, int depth, const unsigned *tok_off, const unsigned char *tok_bytes,
                                            int n_tok, int v) {
    const GenPdaWalk dead{0ull, 0ull, depth, depth, 0u};
    if (q == 0 || v <= 0 || v >= n_tok) return dead;
    const unsigned o0 = tok_off[v], o1 = tok_off[v + 1];
    if (o0 & GEN_TOK_UNKNOWN) return dead;
    const unsigned beg = o0, end = o1 & ~GEN_TOK_UNKNOWN;
    if (end <= beg) return dead;                                // the empty token
    int len = (int)(end - beg);
    if (len > GEN_TOKEN_LEN) len = GEN_TOKEN_LEN;               // the table never holds a longer one (rwkv_gen_set_token_bytes refuses it)
    return gen_pda_token_walk(next, act, max_depth, q, base, depth, tok_bytes + beg, len);
}

// The HALT predicate for a drawn token that ended in `end` at depth `depth` (end == 0: it was not allowed, which never halts);
// flags = flags[end].
RWKV_HD inline bool gen_pda_halt(unsigned end, int depth, unsigned char flags, int mode) {
    if (!end || depth != 0 || !(flags & GEN_PDA_ACCEPT)) return false;
    return mode == GEN_PDA_HALT_ACCEPT || (flags & GEN_PDA_END) != 0;
}

// `update` (bnf.rs:40-48) for a drawn token: the serial walk of its at most GEN_TOKEN_LEN bytes, then the slot's real configuration
// (*state, stack[0 .. *depth)) is rewritten behind it — the entries the token owns go on top of what it left of the stack — and the halt
// predicate is returned.  It is the mask's own walk, so a token the mask forbade is the token this leaves alone: the configuration stays
// where it was and nothing halts.
RWKV_HD inline bool gen_pda_commit(const unsigned short *next, const unsigned short *act, const unsigned char *flags, int max_depth, int mode,
                                   int *state, unsigned short *stack, int *depth, const unsigned *tok_off, const unsigned char *tok_bytes,
                                   int n_tok, int v) {
    GenPdaWalk w = gen_pda_token_end(next, act, max_depth, (unsigned)*state, stack, *depth, tok_off, tok_bytes, n_tok, v);
    if (!w.state) return false;
    for (int d = w.depth - 1; d >= w.low; --d) {                // at most GEN_PDA_TOKEN_SPAN entries, the top first
        stack[d] = (unsigned short)(w.lo & 0xFFFFu);
        w.lo = (w.lo >> 16) | (w.hi << 48);
        w.hi >>= 16;
    }
    *state = (int)w.state;
    *depth = w.depth;
    return gen_pda_halt(w.state, w.depth, flags[w.state], mode);
}

}  // namespace rwkv

// gen_dfa.h — the byte-automaton constraint of resident generation as host/device functions: a second implementation of the reference's
// `Formatter` trait (`transform` = mask, `update` = advance and maybe halt; sampler/bnf.rs:34-48, run.rs:676-680, 892-897, 990) for REGULAR
// constraints.  It is not kbnf and no port of it: context-free grammars stay on the host (rwkv_infer_sample with `allow`).
// Host-only header (no HIP include, like gen_stop.h): gen_mask_kernel and gen_post_kernel (rwkv_kernels.hip) call exactly these functions,
// so do rwkv_dfa_walk / rwkv_dfa_allow (rwkv_dfa.cpp), and tests/cpp/gen_dfa_test.cpp compiles the same text with g++ and drives it in the
// kernels' order.
//
// The automaton: trans[n_states][256] of uint16, state 0 is DEAD (its row is all zeros), a state is LIVE when it is not 0.  Per state one
// flag byte: GEN_DFA_ACCEPT, and GEN_DFA_END when no byte leads from it to a live state.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gen_stop.h"   // RWKV_HD, GEN_TOK_UNKNOWN, GEN_TOKEN_LEN

namespace rwkv {

constexpr int GEN_DFA_MAX_STATES = 4096;            // RWKV_DFA_MAX_STATES, DEAD included
enum : int { GEN_DFA_HALT_FINAL = 0, GEN_DFA_HALT_ACCEPT = 1 };   // RWKV_DFA_HALT_*
constexpr unsigned char GEN_DFA_ACCEPT = 1, GEN_DFA_END = 2;

// walk `n` bytes from state q; DEAD is absorbing
RWKV_HD inline unsigned gen_dfa_walk(const unsigned short *trans, unsigned q, const unsigned char *bytes, int n) {
    for (int i = 0; i < n && q; ++i) q = trans[q * 256u + bytes[i]];
    return q;
}

// The flag byte of state q (computed once on the host, when a table is taken in).
RWKV_HD inline unsigned char gen_dfa_flags(const unsigned short *trans, const unsigned char *accepting, unsigned q) {
    bool live_next = false;
    for (int c = 0; c < 256; ++c) live_next |= trans[q * 256u + c] != 0;
    return (unsigned char)((q && accepting[q] ? GEN_DFA_ACCEPT : 0) | (live_next ? 0 : GEN_DFA_END));
}

// The ALLOWED predicate, as the state the token ends in: token v is allowed in state q iff v < n_tok, its table entry is known and
// non-empty, and walking its bytes from q ends in a live state.  Returns that state, or 0 (DEAD) when the token is not allowed: empty
// tokens (kbnf's vocabulary holds none either, bnf.rs:18) and unknown ids never are, and neither is token 0 — the World vocabulary has
// no entry for it, and whatever a table says, it is the end-of-sequence id (run.rs:855): a constrained slot never samples its own end.
// Token table as in GenArgs: bytes of id i are tok_bytes[off(i) .. off(i + 1)), off = tok_off[] & ~GEN_TOK_UNKNOWN.
RWKV_HD inline unsigned gen_dfa_token_end(const unsigned short *trans, unsigned q, const unsigned *tok_off, const unsigned char *tok_bytes,
                                          int n_tok, int v) {
    if (q == 0 || v <= 0 || v >= n_tok) return 0;
    const unsigned o0 = tok_off[v], o1 = tok_off[v + 1];
    if (o0 & GEN_TOK_UNKNOWN) return 0;
    const unsigned beg = o0, end = o1 & ~GEN_TOK_UNKNOWN;
    if (end <= beg) return 0;                                   // the empty token
    int len = (int)(end - beg);
    if (len > GEN_TOKEN_LEN) len = GEN_TOKEN_LEN;               // the table never holds a longer one (rwkv_gen_set_token_bytes refuses it)
    return gen_dfa_walk(trans, q, tok_bytes + beg, len);
}

// `update` (bnf.rs:40-48): the state behind a drawn token whose end state is `end` (gen_dfa_token_end).  A token that is not allowed
// leaves the state where it was — kbnf rejects it and goes on (bnf.rs:44).
RWKV_HD inline unsigned gen_dfa_advance(unsigned q, unsigned end) { return end ? end : q; }

// The HALT predicate for a drawn token that ended in `end` (0: it was not allowed, which never halts); flags = flags[end].
//   GEN_DFA_HALT_FINAL   the new state accepts and no byte leads from it to a live state
//   GEN_DFA_HALT_ACCEPT  the new state accepts
RWKV_HD inline bool gen_dfa_halt(unsigned end, unsigned char flags, int mode) {
    if (!end || !(flags & GEN_DFA_ACCEPT)) return false;
    return mode == GEN_DFA_HALT_ACCEPT || (flags & GEN_DFA_END) != 0;
}

}  // namespace rwkv

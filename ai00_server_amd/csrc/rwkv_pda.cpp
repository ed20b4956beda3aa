// rwkv_pda.cpp — byte automata with a return-state stack for the constraint of resident generation (rwkv_pda_*, include/rwkv_abi.h): the
// table check, the JSON automaton of RFC 8259, the walk, the host-side mask and the liveness rule.  Plain C++ with no HIP in it.  This is
// NOT kbnf (sampler/bnf.rs) and no port of it: it covers what a return-state stack expresses, nested brackets above all.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rwkv_abi.h"
#include "rwkv_pda.h"

extern "C" void rwkv_set_last_error(const char *msg);

static_assert(RWKV_PDA_MAX_STATES == rwkv::GEN_PDA_MAX_STATES && RWKV_PDA_MAX_DEPTH == rwkv::GEN_PDA_MAX_DEPTH &&
              RWKV_PDA_TOKEN_SPAN == rwkv::GEN_PDA_TOKEN_SPAN && RWKV_PDA_POP == rwkv::GEN_PDA_POP &&
              (int)RWKV_PDA_HALT_FINAL == (int)rwkv::GEN_PDA_HALT_FINAL && (int)RWKV_PDA_HALT_ACCEPT == (int)rwkv::GEN_PDA_HALT_ACCEPT,
              "include/rwkv_abi.h and csrc/gen_pda.h spell the same limits");

namespace {

struct PdaError {
    rwkv_status code;
    std::string msg;
};
[[noreturn]] void fail(rwkv_status code, const std::string &msg) { throw PdaError{code, msg}; }

std::unique_ptr<rwkv_pda> finish_table(std::vector<uint16_t> next, std::vector<uint16_t> act, std::vector<uint8_t> accepting, int n_states,
                                       int start, int max_depth) {
    auto p = std::make_unique<rwkv_pda>();
    p->n_states = n_states;
    p->start = start;
    p->max_depth = max_depth;
    p->next = std::move(next);
    p->act = std::move(act);
    p->accepting = std::move(accepting);
    p->flags.resize((size_t)n_states);
    for (int q = 0; q < n_states; ++q) p->flags[(size_t)q] = rwkv::gen_pda_flags(p->next.data(), p->act.data(), p->accepting.data(), (unsigned)q);
    return p;
}

// ---- the JSON automaton (RFC 8259 over bytes) ---------------------------------------------------------------------------------------
// A value in one of three contexts — top level, array element, object member — ends in the context's AFTER state; `[` and `{` push that
// AFTER state as the return state, `]` and `}` pop it.  A number has no terminator: the states in which one may end carry a copy of
// their context's AFTER row beside their own digits.
struct Builder {
    std::vector<std::vector<uint16_t>> next, act;
    std::vector<uint8_t> acc;
    Builder() { add(); }                                             // DEAD
    int add() {
        next.emplace_back(256, (uint16_t)0);
        act.emplace_back(256, (uint16_t)0);
        acc.push_back(0);
        return (int)next.size() - 1;
    }
    void plain(int q, int lo, int hi, int t) { for (int c = lo; c <= hi; ++c) { next[(size_t)q][(size_t)c] = (uint16_t)t; act[(size_t)q][(size_t)c] = 0; } }
    void plain(int q, const char *set, int t) { for (; *set; ++set) plain(q, (unsigned char)*set, (unsigned char)*set, t); }
    void push(int q, int c, int t, int ret) { next[(size_t)q][(size_t)c] = (uint16_t)t; act[(size_t)q][(size_t)c] = (uint16_t)ret; }
    void pop(int q, int c) { next[(size_t)q][(size_t)c] = 0; act[(size_t)q][(size_t)c] = (uint16_t)RWKV_PDA_POP; }

    // behind the opening quote; the closing quote leads to `done`.  Well-formed UTF-8 only (Unicode table 3-7), nothing below 0x20.
    int string(int done) {
        const int S = add(), E = add();
        int U[4];
        for (int &u : U) u = add();
        for (int c = 0x20; c < 0x80; ++c) if (c != '"' && c != '\\') plain(S, c, c, S);
        plain(S, "\"", done);
        plain(S, "\\", E);
        plain(E, "\"\\/bfnrt", S);
        plain(E, "u", U[0]);
        for (int i = 0; i < 4; ++i) plain(U[i], "0123456789abcdefABCDEF", i < 3 ? U[i + 1] : S);
        const int c1 = add(), c2 = add(), c3 = add(), e0 = add(), ed = add(), f0 = add(), f4 = add();
        plain(S, 0xC2, 0xDF, c1); plain(c1, 0x80, 0xBF, S);
        plain(S, 0xE0, 0xE0, e0); plain(e0, 0xA0, 0xBF, c1);
        plain(S, 0xE1, 0xEC, c2); plain(S, 0xEE, 0xEF, c2); plain(c2, 0x80, 0xBF, c1);
        plain(S, 0xED, 0xED, ed); plain(ed, 0x80, 0x9F, c1);
        plain(S, 0xF0, 0xF0, f0); plain(f0, 0x90, 0xBF, c2);
        plain(S, 0xF1, 0xF3, c3); plain(c3, 0x80, 0xBF, c2);
        plain(S, 0xF4, 0xF4, f4); plain(f4, 0x80, 0x8F, c2);
        return S;
    }
};

std::unique_ptr<rwkv_pda> json(uint32_t flags, int max_depth) {
    const bool object_only = (flags & RWKV_PDA_JSON_OBJECT) != 0;
    const char *ws = (flags & RWKV_PDA_JSON_COMPACT) ? "" : " \t\n\r";
    Builder m;
    const int AT = m.add(), AA = m.add(), AO = m.add();              // AFTER a value: top level, in an array, in an object
    m.acc[(size_t)AT] = 1;
    const int ARR_OPEN = m.add(), ARR_NEXT = m.add(), OBJ_OPEN = m.add(), OBJ_NEXT = m.add(), K_AFTER = m.add(), OBJ_VAL = m.add(), START = m.add();
    const int KEY = m.string(K_AFTER);
    m.plain(AT, ws, AT);
    m.plain(AA, ws, AA); m.plain(AA, ",", ARR_NEXT); m.pop(AA, ']');
    m.plain(AO, ws, AO); m.plain(AO, ",", OBJ_NEXT); m.pop(AO, '}');
    auto value_start = [&](int q, int after, bool containers_only) {
        m.plain(q, ws, q);
        m.push(q, '[', ARR_OPEN, after);
        m.push(q, '{', OBJ_OPEN, after);
        if (containers_only) return;
        m.plain(q, "\"", m.string(after));
        for (const char *lit : {"true", "false", "null"}) {
            int cur = q;
            for (size_t i = 0; lit[i]; ++i) {
                const unsigned char ch = (unsigned char)lit[i];
                if (!lit[i + 1]) { m.plain(cur, ch, ch, after); break; }
                if (!m.next[(size_t)cur][ch]) m.plain(cur, ch, ch, m.add());
                cur = m.next[(size_t)cur][ch];
            }
        }
        // -?(0|[1-9]\d*)(\.\d+)?([eE][+-]?\d+)?
        const int neg = m.add(), zero = m.add(), intd = m.add(), dot = m.add(), frac = m.add(), e = m.add(), es = m.add(), ed = m.add();
        m.plain(q, "-", neg); m.plain(q, "0", zero); m.plain(q, "123456789", intd);
        m.plain(neg, "0", zero); m.plain(neg, "123456789", intd);
        for (int f : {zero, intd, frac, ed}) {                       // the number may end here: the state takes over the AFTER row
            m.next[(size_t)f] = m.next[(size_t)after];
            m.act[(size_t)f] = m.act[(size_t)after];
            m.acc[(size_t)f] = m.acc[(size_t)after];
        }
        m.plain(intd, "0123456789", intd);
        for (int f : {zero, intd}) { m.plain(f, ".", dot); m.plain(f, "eE", e); }
        m.plain(dot, "0123456789", frac); m.plain(frac, "0123456789", frac); m.plain(frac, "eE", e);
        m.plain(e, "+-", es); m.plain(e, "0123456789", ed); m.plain(es, "0123456789", ed); m.plain(ed, "0123456789", ed);
    };
    value_start(START, AT, object_only);
    value_start(ARR_NEXT, AA, false);
    value_start(OBJ_VAL, AO, false);
    value_start(ARR_OPEN, AA, false);
    m.pop(ARR_OPEN, ']');
    m.plain(OBJ_OPEN, ws, OBJ_OPEN); m.plain(OBJ_OPEN, "\"", KEY); m.pop(OBJ_OPEN, '}');
    m.plain(OBJ_NEXT, ws, OBJ_NEXT); m.plain(OBJ_NEXT, "\"", KEY);
    m.plain(K_AFTER, ws, K_AFTER); m.plain(K_AFTER, ":", OBJ_VAL);

    // canonical numbering: breadth-first from the start state, bytes ascending, a push's target before its return state; DEAD = 0, start = 1
    const size_t N = m.next.size();
    std::vector<int> number(N, -1), order{0, START};
    number[0] = 0;
    number[(size_t)START] = 1;
    auto visit = [&](int t) { if (number[(size_t)t] < 0) { number[(size_t)t] = (int)order.size(); order.push_back(t); } };
    for (size_t at = 1; at < order.size(); ++at) {
        const int q = order[at];
        for (int c = 0; c < 256; ++c) {
            const unsigned a = m.act[(size_t)q][(size_t)c];
            if (a == RWKV_PDA_POP) continue;
            visit(m.next[(size_t)q][(size_t)c]);
            if (a) visit((int)a);
        }
    }
    const int n_states = (int)order.size();
    std::vector<uint16_t> next((size_t)n_states * 256, 0), act((size_t)n_states * 256, 0);
    std::vector<uint8_t> accepting((size_t)n_states, 0);
    for (int s = 1; s < n_states; ++s) {
        const int q = order[(size_t)s];
        accepting[(size_t)s] = m.acc[(size_t)q];
        for (int c = 0; c < 256; ++c) {
            const unsigned a = m.act[(size_t)q][(size_t)c];
            const size_t cell = (size_t)s * 256 + (size_t)c;
            if (a == RWKV_PDA_POP) { act[cell] = (uint16_t)RWKV_PDA_POP; continue; }
            next[cell] = (uint16_t)number[m.next[(size_t)q][(size_t)c]];
            act[cell] = a ? (uint16_t)number[a] : (uint16_t)0;
        }
    }
    return finish_table(std::move(next), std::move(act), std::move(accepting), n_states, 1, max_depth);
}

template <typename F>
rwkv_status pda_guard(F &&f) {
    try {
        f();
        return RWKV_OK;
    } catch (const PdaError &e) {
        rwkv_set_last_error(e.msg.c_str());
        return e.code;
    } catch (const std::bad_alloc &) {
        rwkv_set_last_error("host out of memory");
        return RWKV_ERR_OOM;
    } catch (const std::exception &e) {
        rwkv_set_last_error(e.what());
        return RWKV_ERR_INVALID;
    }
}

void check_depth(int32_t max_depth) {
    if (max_depth < 1 || max_depth > RWKV_PDA_MAX_DEPTH) fail(RWKV_ERR_INVALID, "pda: max_depth outside 1 .. RWKV_PDA_MAX_DEPTH");
}

// a configuration of `p`: any state of the table (0 = dead is one), a stack of live states no deeper than max_depth
void check_config(const rwkv_pda *p, int32_t state, const uint16_t *stack, int32_t depth) {
    if (!p) fail(RWKV_ERR_INVALID, "pda: null handle");
    if (state < 0 || state >= p->n_states) fail(RWKV_ERR_INVALID, "pda: state out of range");
    if (depth < 0 || depth > p->max_depth) fail(RWKV_ERR_INVALID, "pda: depth outside 0 .. max_depth");
    if (depth && !stack) fail(RWKV_ERR_INVALID, "pda: null stack");
    for (int32_t i = 0; i < depth; ++i) if (stack[i] < 1 || stack[i] >= p->n_states) fail(RWKV_ERR_INVALID, "pda: a stack entry is no live state of the table");
}

}  // namespace

namespace rwkv {
bool pda_never_stuck(const rwkv_pda &p, int state, const uint16_t *stack, int depth, const uint8_t single[256]) {
    enum : uint8_t { UNSEEN = 0, EMPTY_ONLY = 1, ANY_DEPTH = 2 };
    std::vector<uint8_t> mark((size_t)p.n_states, UNSEEN);
    std::vector<int> work;
    auto raise = [&](int q, uint8_t m) {
        if (q > 0 && mark[(size_t)q] < m) { mark[(size_t)q] = m; work.push_back(q); }
    };
    raise(state, depth == 0 ? EMPTY_ONLY : ANY_DEPTH);
    for (int i = 0; i < depth; ++i) raise(stack[i], i == 0 ? EMPTY_ONLY : ANY_DEPTH);   // each is entered by the pop that uncovers it
    while (!work.empty()) {
        const int q = work.back();
        work.pop_back();
        const uint8_t m = mark[(size_t)q];
        for (int c = 0; c < 256; ++c) {
            const unsigned a = p.act[(size_t)q * 256 + (size_t)c], t = p.next[(size_t)q * 256 + (size_t)c];
            if (a == GEN_PDA_POP) continue;                            // what a pop enters was raised where it was pushed
            if (a == 0) { raise((int)t, m); continue; }
            if (!t) continue;
            raise((int)t, ANY_DEPTH);
            raise((int)a, m);                                          // the return state is entered at the depth of the push
        }
    }
    for (int q = 1; q < p.n_states; ++q) {
        const uint8_t m = mark[(size_t)q];
        if (m == UNSEEN) continue;
        if (q != state && m == EMPTY_ONLY && p.flags[(size_t)q] == (GEN_PDA_ACCEPT | GEN_PDA_END)) continue;
        bool way_on = false;
        for (int c = 0; c < 256 && !way_on; ++c) {
            const unsigned a = p.act[(size_t)q * 256 + (size_t)c], t = p.next[(size_t)q * 256 + (size_t)c];
            if (!single[c] || a == GEN_PDA_POP || !t) continue;
            way_on = a == 0 || m == EMPTY_ONLY;
        }
        if (!way_on) return false;
    }
    return true;
}
}  // namespace rwkv

namespace {
// the token table of rwkv_gen_set_token_bytes in the engine's form, so that gen_pda_token_end reads here what the kernel reads
std::vector<unsigned> token_offsets(const uint8_t *bytes, const int32_t *lens, size_t n_tokens) {
    if (!lens && n_tokens) fail(RWKV_ERR_INVALID, "pda: null lens");
    if (n_tokens >= 0x7fffffffu) fail(RWKV_ERR_INVALID, "pda: too many tokens");
    std::vector<unsigned> off(n_tokens + 1);
    size_t pos = 0;
    for (size_t i = 0; i < n_tokens; ++i) {
        if (lens[i] < -1) fail(RWKV_ERR_INVALID, "token table: negative length");
        if (lens[i] > RWKV_GEN_TOKEN_LEN) fail(RWKV_ERR_UNSUPPORTED, "token table: a token is longer than RWKV_GEN_TOKEN_LEN");
        off[i] = (unsigned)pos | (lens[i] < 0 ? rwkv::GEN_TOK_UNKNOWN : 0u);
        if (lens[i] > 0) pos += (size_t)lens[i];
        if (pos >= rwkv::GEN_TOK_UNKNOWN) fail(RWKV_ERR_UNSUPPORTED, "token table: more than 2 GiB of bytes");
    }
    off[n_tokens] = (unsigned)pos;
    if (pos && !bytes) fail(RWKV_ERR_INVALID, "token table: null bytes");
    return off;
}
}  // namespace

extern "C" {

rwkv_status rwkv_pda_from_table(const uint16_t *next, const uint16_t *act, const uint8_t *accepting, int32_t n_states, int32_t start,
                                int32_t max_depth, rwkv_pda **out) {
    return pda_guard([&] {
        if (!out) fail(RWKV_ERR_INVALID, "pda: null out");
        *out = nullptr;
        if (!next || !act || !accepting) fail(RWKV_ERR_INVALID, "pda: null table");
        if (n_states < 2) fail(RWKV_ERR_INVALID, "pda: a table needs DEAD and a start state");
        if (n_states > RWKV_PDA_MAX_STATES) fail(RWKV_ERR_UNSUPPORTED, "pda: more than RWKV_PDA_MAX_STATES states");
        if (start < 1 || start >= n_states) fail(RWKV_ERR_INVALID, "pda: start state out of range");
        check_depth(max_depth);
        if (accepting[0]) fail(RWKV_ERR_INVALID, "pda: state 0 is DEAD and accepts nothing");
        for (int c = 0; c < 256; ++c) if (next[c] || act[c]) fail(RWKV_ERR_INVALID, "pda: state 0 is DEAD, both of its rows are all zeros");
        const size_t cells = (size_t)n_states * 256;
        for (size_t k = 256; k < cells; ++k) {
            if (act[k] == RWKV_PDA_POP) continue;                      // `next` is ignored
            if (next[k] >= n_states) fail(RWKV_ERR_INVALID, "pda: a transition leaves the table");
            if (act[k] == 0) continue;
            if (act[k] >= n_states) fail(RWKV_ERR_INVALID, "pda: a push names a return state outside the table");
            if (next[k] == 0) fail(RWKV_ERR_INVALID, "pda: a push needs a live target");
        }
        std::vector<uint8_t> acc(accepting, accepting + n_states);
        for (auto &a : acc) a = a ? 1 : 0;
        *out = finish_table(std::vector<uint16_t>(next, next + cells), std::vector<uint16_t>(act, act + cells), std::move(acc), n_states, start, max_depth).release();
    });
}

rwkv_status rwkv_pda_json(uint32_t flags, int32_t max_depth, rwkv_pda **out) {
    return pda_guard([&] {
        if (!out) fail(RWKV_ERR_INVALID, "pda: null out");
        *out = nullptr;
        if (flags & ~(uint32_t)(RWKV_PDA_JSON_OBJECT | RWKV_PDA_JSON_COMPACT)) fail(RWKV_ERR_INVALID, "pda: unknown JSON flag");
        check_depth(max_depth);
        *out = json(flags, max_depth).release();
    });
}

void rwkv_pda_free(rwkv_pda *p) { delete p; }
int32_t rwkv_pda_num_states(const rwkv_pda *p) { return p ? p->n_states : 0; }
int32_t rwkv_pda_start(const rwkv_pda *p) { return p ? p->start : 0; }
int32_t rwkv_pda_max_depth(const rwkv_pda *p) { return p ? p->max_depth : 0; }

rwkv_status rwkv_pda_table(const rwkv_pda *p, uint16_t *next, uint16_t *act, uint8_t *accepting) {
    return pda_guard([&] {
        if (!p) fail(RWKV_ERR_INVALID, "pda: null handle");
        if (next) std::memcpy(next, p->next.data(), p->next.size() * sizeof(uint16_t));
        if (act) std::memcpy(act, p->act.data(), p->act.size() * sizeof(uint16_t));
        if (accepting) std::memcpy(accepting, p->accepting.data(), p->accepting.size());
    });
}

rwkv_status rwkv_pda_walk(const rwkv_pda *p, int32_t state, const uint16_t *stack, int32_t depth, const uint8_t *bytes, size_t n,
                          int32_t *state_out, uint16_t *stack_out, int32_t *depth_out) {
    return pda_guard([&] {
        check_config(p, state, stack, depth);
        if (!state_out || !stack_out || !depth_out || (n && !bytes)) fail(RWKV_ERR_INVALID, "pda: null bytes / output");
        uint16_t st[RWKV_PDA_MAX_DEPTH] = {};
        for (int32_t i = 0; i < depth; ++i) st[i] = stack[i];
        unsigned q = (unsigned)state;
        int d = depth;
        for (size_t i = 0; i < n && q; ++i) q = rwkv::gen_pda_step(p->next.data(), p->act.data(), p->max_depth, q, st, &d, bytes[i]);
        *state_out = (int32_t)q;
        *depth_out = d;
        for (int i = 0; i < d; ++i) stack_out[i] = st[i];
    });
}

rwkv_status rwkv_pda_allow(const rwkv_pda *p, int32_t state, const uint16_t *stack, int32_t depth, const uint8_t *bytes, const int32_t *lens,
                           size_t n_tokens, uint8_t *allow, size_t num_vocab) {
    return pda_guard([&] {
        check_config(p, state, stack, depth);
        if (!allow && num_vocab) fail(RWKV_ERR_INVALID, "pda: null allow");
        const std::vector<unsigned> off = token_offsets(bytes, lens, n_tokens);
        for (size_t v = 0; v < num_vocab; ++v)
            allow[v] = v < n_tokens && rwkv::gen_pda_token_end(p->next.data(), p->act.data(), p->max_depth, (unsigned)state, stack, depth, off.data(), bytes,
                                                               (int)n_tokens, (int)v).state ? 1 : 0;
    });
}

rwkv_status rwkv_pda_check_live(const rwkv_pda *p, int32_t state, const uint16_t *stack, int32_t depth, const int32_t *lens, const uint8_t *bytes,
                                size_t n_tokens) {
    return pda_guard([&] {
        check_config(p, state, stack, depth);
        if (state == 0) fail(RWKV_ERR_INVALID, "pda: state 0 is dead");
        const std::vector<unsigned> off = token_offsets(bytes, lens, n_tokens);
        uint8_t single[256] = {};
        for (size_t i = 1; i < n_tokens; ++i)                          // token 0 is never allowed
            if (lens[i] == 1) single[bytes[off[i]]] = 1;
        if (!rwkv::pda_never_stuck(*p, state, stack, depth, single))
            fail(RWKV_ERR_UNSUPPORTED, "constraint: a reachable state has no single-byte token with a plain transition that leads on (a row could be masked whole)");
    });
}

}  // extern "C"

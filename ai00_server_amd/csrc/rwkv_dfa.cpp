// rwkv_dfa.cpp — byte-level DFAs for the constraint of resident generation (rwkv_dfa_*, include/rwkv_abi.h): the table check, a compiler
// for a small anchored regex dialect (Thompson NFA -> subset construction -> trim -> minimise -> canonical numbering), the walk and the
// host-side mask.  Plain C++ with no HIP in it.  This is NOT kbnf (sampler/bnf.rs) and no port of it: it covers regular constraints only.
#include <algorithm>
#include <array>
#include <bitset>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rwkv_abi.h"
#include "rwkv_dfa.h"

extern "C" void rwkv_set_last_error(const char *msg);

static_assert(RWKV_DFA_MAX_STATES == rwkv::GEN_DFA_MAX_STATES && (int)RWKV_DFA_HALT_FINAL == (int)rwkv::GEN_DFA_HALT_FINAL &&
              (int)RWKV_DFA_HALT_ACCEPT == (int)rwkv::GEN_DFA_HALT_ACCEPT, "include/rwkv_abi.h and csrc/gen_dfa.h spell the same limits");

namespace {

struct DfaError {
    rwkv_status code;
    std::string msg;
};
[[noreturn]] void fail(rwkv_status code, const std::string &msg) { throw DfaError{code, msg}; }
[[noreturn]] void bad_pattern(const std::string &msg, size_t off) { fail(RWKV_ERR_INVALID, "pattern: " + msg + " at offset " + std::to_string(off)); }

using ByteSet = std::bitset<256>;

// ---- the pattern's syntax tree ------------------------------------------------------------------------------------------------------
constexpr int MAX_DEPTH = 128;            // nesting of groups (the recursive passes below go this deep)
constexpr size_t MAX_NFA = 60000;         // Thompson states (bounded repeats are unrolled)
constexpr size_t MAX_SUBSETS = 16384;     // DFA states before minimisation

struct Node {
    enum Kind { EMPTY, SET, CAT, ALT, REPEAT } kind = EMPTY;
    ByteSet set;                          // SET
    std::vector<std::unique_ptr<Node>> kids;   // CAT / ALT: any number; REPEAT: one
    int lo = 0, hi = 0;                   // REPEAT: hi < 0 = unbounded
};
using NodeP = std::unique_ptr<Node>;

NodeP mk_set(const ByteSet &s) { auto n = std::make_unique<Node>(); n->kind = Node::SET; n->set = s; return n; }
NodeP mk_range(int lo, int hi) { ByteSet s; for (int c = lo; c <= hi; ++c) s.set((size_t)c); return mk_set(s); }
NodeP mk_cat(std::vector<NodeP> kids) {
    if (kids.size() == 1) return std::move(kids[0]);
    auto n = std::make_unique<Node>();
    n->kind = kids.empty() ? Node::EMPTY : Node::CAT;
    n->kids = std::move(kids);
    return n;
}
NodeP mk_alt(std::vector<NodeP> kids) {
    if (kids.size() == 1) return std::move(kids[0]);
    auto n = std::make_unique<Node>();
    n->kind = Node::ALT;
    n->kids = std::move(kids);
    return n;
}
NodeP mk_seq(std::initializer_list<std::pair<int, int>> ranges) {
    std::vector<NodeP> k;
    for (auto r : ranges) k.push_back(mk_range(r.first, r.second));
    return mk_cat(std::move(k));
}
// any well-formed UTF-8 character (Unicode table 3-7, the rule of gen_utf8_valid) whose ASCII form is not in `ascii`
NodeP mk_negated(const ByteSet &ascii) {
    ByteSet one;
    for (int c = 0; c < 0x80; ++c) if (!ascii.test((size_t)c)) one.set((size_t)c);
    std::vector<NodeP> alt;
    alt.push_back(mk_set(one));
    alt.push_back(mk_seq({{0xC2, 0xDF}, {0x80, 0xBF}}));
    alt.push_back(mk_seq({{0xE0, 0xE0}, {0xA0, 0xBF}, {0x80, 0xBF}}));
    alt.push_back(mk_seq({{0xE1, 0xEC}, {0x80, 0xBF}, {0x80, 0xBF}}));
    alt.push_back(mk_seq({{0xED, 0xED}, {0x80, 0x9F}, {0x80, 0xBF}}));
    alt.push_back(mk_seq({{0xEE, 0xEF}, {0x80, 0xBF}, {0x80, 0xBF}}));
    alt.push_back(mk_seq({{0xF0, 0xF0}, {0x90, 0xBF}, {0x80, 0xBF}, {0x80, 0xBF}}));
    alt.push_back(mk_seq({{0xF1, 0xF3}, {0x80, 0xBF}, {0x80, 0xBF}, {0x80, 0xBF}}));
    alt.push_back(mk_seq({{0xF4, 0xF4}, {0x80, 0x8F}, {0x80, 0xBF}, {0x80, 0xBF}}));
    return mk_alt(std::move(alt));
}

struct Parser {
    const uint8_t *p;
    size_t n, i = 0;
    int depth = 0;

    bool more() const { return i < n; }
    static int hex(uint8_t c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
    static bool meta(uint8_t c) { return std::strchr(".[](){}|*+?^$-", c) != nullptr && c != 0; }

    // an escape behind the backslash at p[i - 1]: a single byte (returned, >= 0) or a class (-1, added to `cls`)
    int escape(ByteSet &cls) {
        if (!more()) bad_pattern("dangling backslash", i - 1);
        const uint8_t c = p[i++];
        switch (c) {
        case 'n': return '\n';
        case 'r': return '\r';
        case 't': return '\t';
        case '\\': case '"': case '/': return c;
        case 'd': for (int k = '0'; k <= '9'; ++k) cls.set((size_t)k); return -1;
        case 'w':
            for (int k = '0'; k <= '9'; ++k) cls.set((size_t)k);
            for (int k = 'a'; k <= 'z'; ++k) { cls.set((size_t)k); cls.set((size_t)(k - 32)); }
            cls.set('_');
            return -1;
        case 's': cls.set(' '); cls.set('\t'); cls.set('\r'); cls.set('\n'); return -1;
        case 'x': {
            if (i + 2 > n || hex(p[i]) < 0 || hex(p[i + 1]) < 0) bad_pattern("\\x needs two hex digits", i - 2);
            const int v = hex(p[i]) * 16 + hex(p[i + 1]);
            i += 2;
            return v;
        }
        default:
            if (meta(c)) return c;
            bad_pattern("unknown escape", i - 2);
        }
    }

    NodeP klass() {                        // behind '['
        const size_t open = i - 1;
        bool neg = false;
        if (more() && p[i] == '^') { neg = true; ++i; }
        ByteSet s;
        for (;;) {
            if (!more()) bad_pattern("unterminated class", open);
            uint8_t c = p[i++];
            if (c == ']') break;
            int lo;
            if (c == '\\') {
                lo = escape(s);
                if (lo < 0) continue;        // \d \w \s: no range from a class
            } else lo = c;
            if (lo >= 0x80) bad_pattern("a class holds ASCII members only", i - 1);
            int hi = lo;
            if (i + 1 < n && p[i] == '-' && p[i + 1] != ']') {
                const size_t at = i;
                ++i;
                c = p[i++];
                if (c == '\\') {
                    ByteSet none;
                    hi = escape(none);
                    if (hi < 0) bad_pattern("a class escape cannot end a range", at);
                } else hi = c;
                if (hi >= 0x80) bad_pattern("a class holds ASCII members only", i - 1);
                if (hi < lo) bad_pattern("range out of order", at);
            }
            for (int k = lo; k <= hi; ++k) s.set((size_t)k);
        }
        return neg ? mk_negated(s) : mk_set(s);
    }

    // {m} {m,} {m,n} behind '{'
    void bounds(int &lo, int &hi) {
        const size_t open = i - 1;
        auto number = [&](int &v) {
            if (!more() || p[i] < '0' || p[i] > '9') return false;
            v = 0;
            while (more() && p[i] >= '0' && p[i] <= '9') {
                v = v * 10 + (p[i++] - '0');
                if (v > 255) bad_pattern("repeat count above 255", open);
            }
            return true;
        };
        if (!number(lo)) bad_pattern("a repeat needs a count", open);
        hi = lo;
        if (more() && p[i] == ',') {
            ++i;
            if (!number(hi)) hi = -1;
        }
        if (!more() || p[i] != '}') bad_pattern("unterminated repeat", open);
        ++i;
        if (hi >= 0 && hi < lo) bad_pattern("repeat bounds out of order", open);
    }

    NodeP atom() {
        const uint8_t c = p[i++];
        if (c == '(') {
            if (++depth > MAX_DEPTH) fail(RWKV_ERR_UNSUPPORTED, "pattern: groups nested deeper than " + std::to_string(MAX_DEPTH));
            const size_t open = i - 1;
            NodeP inner = alt();
            if (!more() || p[i] != ')') bad_pattern("unterminated group", open);
            ++i;
            --depth;
            return inner;
        }
        if (c == '[') return klass();
        if (c == '.') { ByteSet nl; nl.set('\n'); return mk_negated(nl); }
        if (c == '\\') {
            ByteSet cls;
            const int b = escape(cls);
            return b < 0 ? mk_set(cls) : mk_range(b, b);
        }
        if (c && std::strchr("[](){}|*+?^$", c)) bad_pattern(std::string("unescaped '") + (char)c + "'", i - 1);
        if (c < 0x80) return mk_range(c, c);
        // a literal multi-byte character is ONE atom (a repeat behind it repeats the character, not its last byte)
        const size_t at = i - 1;
        const int more_bytes = c >= 0xC2 && c <= 0xDF ? 1 : c >= 0xE0 && c <= 0xEF ? 2 : c >= 0xF0 && c <= 0xF4 ? 3 : -1;
        if (more_bytes < 0 || at + (size_t)more_bytes >= n || !rwkv::gen_utf8_valid(p + at, more_bytes + 1)) bad_pattern("malformed UTF-8", at);
        std::vector<NodeP> k;
        for (int j = 0; j <= more_bytes; ++j) k.push_back(mk_range(p[at + (size_t)j], p[at + (size_t)j]));
        i = at + (size_t)more_bytes + 1;
        return mk_cat(std::move(k));
    }

    NodeP repeat() {
        NodeP a = atom();
        if (more() && (p[i] == '*' || p[i] == '+' || p[i] == '?' || p[i] == '{')) {
            const uint8_t c = p[i++];
            auto r = std::make_unique<Node>();
            r->kind = Node::REPEAT;
            if (c == '*') { r->lo = 0; r->hi = -1; }
            else if (c == '+') { r->lo = 1; r->hi = -1; }
            else if (c == '?') { r->lo = 0; r->hi = 1; }
            else bounds(r->lo, r->hi);
            r->kids.push_back(std::move(a));
            a = std::move(r);
            if (more() && (p[i] == '*' || p[i] == '+' || p[i] == '?' || p[i] == '{')) bad_pattern("a repeat of a repeat needs a group", i);
        }
        return a;
    }

    NodeP alt() {
        std::vector<NodeP> alts;
        for (;;) {
            std::vector<NodeP> cat;
            while (more() && p[i] != '|' && p[i] != ')') cat.push_back(repeat());
            alts.push_back(mk_cat(std::move(cat)));
            if (more() && p[i] == '|') { ++i; continue; }
            break;
        }
        return mk_alt(std::move(alts));
    }

    NodeP parse() {
        NodeP r = alt();
        if (more()) bad_pattern("unmatched ')'", i);
        return r;
    }
};

// ---- Thompson NFA -------------------------------------------------------------------------------------------------------------------
struct Nfa {
    struct State { std::vector<int> eps; int set = -1, to = -1; };   // at most one byte edge: over sets[set] to `to`
    std::vector<State> st;
    std::vector<ByteSet> sets;            // distinct byte sets
    int add() {
        if (st.size() >= MAX_NFA) fail(RWKV_ERR_UNSUPPORTED, "pattern: too many states (the bounded repeats unroll past the limit)");
        st.emplace_back();
        return (int)st.size() - 1;
    }
    int set_id(const ByteSet &s) {
        for (size_t k = 0; k < sets.size(); ++k) if (sets[k] == s) return (int)k;
        sets.push_back(s);
        return (int)sets.size() - 1;
    }
    // builds `n` between a fresh start and a fresh end
    std::pair<int, int> build(const Node &n) {
        const int s = add(), e = add();
        switch (n.kind) {
        case Node::EMPTY: st[(size_t)s].eps.push_back(e); break;
        case Node::SET: st[(size_t)s].set = set_id(n.set); st[(size_t)s].to = e; break;
        case Node::CAT: {
            int cur = s;
            for (auto &k : n.kids) { auto f = build(*k); st[(size_t)cur].eps.push_back(f.first); cur = f.second; }
            st[(size_t)cur].eps.push_back(e);
            break;
        }
        case Node::ALT:
            for (auto &k : n.kids) { auto f = build(*k); st[(size_t)s].eps.push_back(f.first); st[(size_t)f.second].eps.push_back(e); }
            break;
        case Node::REPEAT: {
            int cur = s;
            for (int k = 0; k < n.lo; ++k) { auto f = build(*n.kids[0]); st[(size_t)cur].eps.push_back(f.first); cur = f.second; }
            if (n.hi < 0) {                                          // x*: a loop through one more copy
                auto f = build(*n.kids[0]);
                const int hub = add();
                st[(size_t)cur].eps.push_back(hub);
                st[(size_t)hub].eps.push_back(f.first);
                st[(size_t)f.second].eps.push_back(hub);
                cur = hub;
            } else {
                for (int k = n.lo; k < n.hi; ++k) {                  // x?: each optional copy may leave for the end
                    auto f = build(*n.kids[0]);
                    st[(size_t)cur].eps.push_back(e);
                    st[(size_t)cur].eps.push_back(f.first);
                    cur = f.second;
                }
            }
            st[(size_t)cur].eps.push_back(e);
            break;
        }
        }
        return {s, e};
    }
};

// ---- NFA -> the canonical minimal DFA ------------------------------------------------------------------------------------------------
std::unique_ptr<rwkv_dfa> finish_table(std::vector<uint16_t> trans, std::vector<uint8_t> accepting, int n_states, int start) {
    auto d = std::make_unique<rwkv_dfa>();
    d->n_states = n_states;
    d->start = start;
    d->trans = std::move(trans);
    d->accepting = std::move(accepting);
    d->flags.resize((size_t)n_states);
    for (int q = 0; q < n_states; ++q) d->flags[(size_t)q] = rwkv::gen_dfa_flags(d->trans.data(), d->accepting.data(), (unsigned)q);
    return d;
}

std::unique_ptr<rwkv_dfa> compile(const uint8_t *pattern, size_t len) {
    Parser ps{pattern, len};
    const NodeP tree = ps.parse();
    Nfa nfa;
    const auto frag = nfa.build(*tree);
    const size_t N = nfa.st.size();

    // byte classes: bytes no set of the NFA tells apart move together
    std::array<int, 256> cls{};
    std::vector<int> rep;
    {
        std::map<std::vector<bool>, int> seen;
        for (int c = 0; c < 256; ++c) {
            std::vector<bool> sig(nfa.sets.size());
            for (size_t k = 0; k < nfa.sets.size(); ++k) sig[k] = nfa.sets[k].test((size_t)c);
            auto it = seen.find(sig);
            if (it == seen.end()) { it = seen.emplace(std::move(sig), (int)rep.size()).first; rep.push_back(c); }
            cls[(size_t)c] = it->second;
        }
    }
    const size_t K = rep.size();

    // subset construction over the classes; subset 0 is the empty set = DEAD
    std::vector<int> stamp(N, -1), stack;
    int round = 0;
    auto closure = [&](std::vector<int> &set) {                        // epsilon closure, sorted
        ++round;
        stack.clear();
        for (int q : set) if (stamp[(size_t)q] != round) { stamp[(size_t)q] = round; stack.push_back(q); }
        set.clear();
        while (!stack.empty()) {
            const int q = stack.back();
            stack.pop_back();
            set.push_back(q);
            for (int t : nfa.st[(size_t)q].eps) if (stamp[(size_t)t] != round) { stamp[(size_t)t] = round; stack.push_back(t); }
        }
        std::sort(set.begin(), set.end());
    };
    std::map<std::vector<int>, int> ids;
    std::vector<std::vector<int>> subsets;
    std::vector<std::vector<int>> dt;                                  // [subset][class] -> subset
    std::vector<uint8_t> acc;
    auto intern = [&](std::vector<int> set) {
        auto it = ids.find(set);
        if (it != ids.end()) return it->second;
        if (subsets.size() >= MAX_SUBSETS) fail(RWKV_ERR_UNSUPPORTED, "pattern: too many states");
        const int id = (int)subsets.size();
        acc.push_back(std::binary_search(set.begin(), set.end(), frag.second) ? 1 : 0);
        ids.emplace(set, id);
        subsets.push_back(std::move(set));
        dt.emplace_back(K, 0);
        return id;
    };
    intern({});
    {
        std::vector<int> s0{frag.first};
        closure(s0);
        intern(std::move(s0));
    }
    for (size_t cur = 1; cur < subsets.size(); ++cur) {
        for (size_t k = 0; k < K; ++k) {
            std::vector<int> next;
            for (int q : subsets[cur]) {
                const Nfa::State &s = nfa.st[(size_t)q];
                if (s.set >= 0 && nfa.sets[(size_t)s.set].test((size_t)rep[k])) next.push_back(s.to);
            }
            if (next.empty()) continue;
            closure(next);
            const int id = intern(std::move(next));
            dt[cur][k] = id;
        }
    }
    const size_t S = subsets.size();

    // trim: a state that cannot reach an accepting state becomes DEAD
    std::vector<uint8_t> useful(S, 0);
    {
        std::vector<std::vector<int>> back(S);
        for (size_t q = 1; q < S; ++q) for (size_t k = 0; k < K; ++k) if (dt[q][k]) back[(size_t)dt[q][k]].push_back((int)q);
        std::vector<int> work;
        for (size_t q = 1; q < S; ++q) if (acc[q]) { useful[q] = 1; work.push_back((int)q); }
        while (!work.empty()) {
            const int q = work.back();
            work.pop_back();
            for (int f : back[(size_t)q]) if (!useful[(size_t)f]) { useful[(size_t)f] = 1; work.push_back(f); }
        }
    }
    if (!useful[1]) fail(RWKV_ERR_UNSUPPORTED, "pattern: it matches nothing (empty language)");
    for (size_t q = 1; q < S; ++q) for (size_t k = 0; k < K; ++k) if (!useful[(size_t)dt[q][k]]) dt[q][k] = 0;

    // minimise (Moore): refine {DEAD} | {accepting} | {the rest} by the blocks of the successors until nothing splits
    std::vector<int> block(S, 0);
    for (size_t q = 1; q < S; ++q) block[q] = !useful[q] ? 0 : acc[q] ? 1 : 2;
    for (size_t n_blocks = 0;;) {
        std::map<std::vector<int>, int> sig_id;
        std::vector<int> nb(S, 0);
        for (size_t q = 0; q < S; ++q) {
            if (q && !useful[q]) { nb[q] = -1; continue; }
            std::vector<int> sig(K + 1);
            sig[0] = block[q];
            for (size_t k = 0; k < K; ++k) sig[k + 1] = block[(size_t)dt[q][k]];
            nb[q] = sig_id.emplace(std::move(sig), (int)sig_id.size()).first->second;
        }
        for (size_t q = 0; q < S; ++q) block[q] = nb[q] < 0 ? nb[0] : nb[q];      // a useless state is DEAD's block
        if (sig_id.size() == n_blocks) break;
        n_blocks = sig_id.size();
    }

    // canonical numbering: breadth-first from the start state, bytes ascending; DEAD = 0, start = 1
    const int dead_block = block[0];
    std::map<int, int> number;
    std::vector<int> order;                                            // block representative (a subset id) per new state
    number[dead_block] = 0;
    order.push_back(0);
    number[block[1]] = 1;
    order.push_back(1);
    for (size_t at = 1; at < order.size(); ++at) {
        const int q = order[at];
        for (int c = 0; c < 256; ++c) {
            const int t = dt[(size_t)q][(size_t)cls[(size_t)c]];
            if (number.emplace(block[(size_t)t], (int)order.size()).second) order.push_back(t);
        }
    }
    const int n_states = (int)order.size();
    if (n_states > RWKV_DFA_MAX_STATES) fail(RWKV_ERR_UNSUPPORTED, "pattern: more than RWKV_DFA_MAX_STATES states");
    std::vector<uint16_t> trans((size_t)n_states * 256, 0);
    std::vector<uint8_t> accepting((size_t)n_states, 0);
    for (int s = 1; s < n_states; ++s) {
        const int q = order[(size_t)s];
        accepting[(size_t)s] = acc[(size_t)q];
        for (int c = 0; c < 256; ++c) trans[(size_t)s * 256 + (size_t)c] = (uint16_t)number[block[(size_t)dt[(size_t)q][(size_t)cls[(size_t)c]]]];
    }
    return finish_table(std::move(trans), std::move(accepting), n_states, 1);
}

template <typename F>
rwkv_status dfa_guard(F &&f) {
    try {
        f();
        return RWKV_OK;
    } catch (const DfaError &e) {
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

void check_state(const rwkv_dfa *d, int32_t state) {
    if (!d) fail(RWKV_ERR_INVALID, "dfa: null handle");
    if (state < 0 || state >= d->n_states) fail(RWKV_ERR_INVALID, "dfa: state out of range");
}

}  // namespace

namespace rwkv {
bool dfa_never_stuck(const rwkv_dfa &d, int state, int mode, const uint8_t single[256]) {
    std::vector<uint8_t> seen((size_t)d.n_states, 0);
    std::vector<int> work{state};
    seen[(size_t)state] = 1;
    while (!work.empty()) {
        const int q = work.back();
        work.pop_back();
        bool way_on = false;
        for (int c = 0; c < 256; ++c) {
            const int t = d.trans[(size_t)q * 256 + (size_t)c];
            if (!t) continue;
            way_on |= single[c] != 0;
            if (!seen[(size_t)t]) { seen[(size_t)t] = 1; work.push_back(t); }
        }
        const bool rests = q == state || !gen_dfa_halt((unsigned)q, d.flags[(size_t)q], mode);
        if (rests && !way_on) return false;
    }
    return true;
}
}  // namespace rwkv

extern "C" {

rwkv_status rwkv_dfa_from_table(const uint16_t *trans, const uint8_t *accepting, int32_t n_states, int32_t start, rwkv_dfa **out) {
    return dfa_guard([&] {
        if (!out) fail(RWKV_ERR_INVALID, "dfa: null out");
        *out = nullptr;
        if (!trans || !accepting) fail(RWKV_ERR_INVALID, "dfa: null table");
        if (n_states < 2) fail(RWKV_ERR_INVALID, "dfa: a table needs DEAD and a start state");
        if (n_states > RWKV_DFA_MAX_STATES) fail(RWKV_ERR_UNSUPPORTED, "dfa: more than RWKV_DFA_MAX_STATES states");
        if (start < 1 || start >= n_states) fail(RWKV_ERR_INVALID, "dfa: start state out of range");
        if (accepting[0]) fail(RWKV_ERR_INVALID, "dfa: state 0 is DEAD and accepts nothing");
        for (int c = 0; c < 256; ++c) if (trans[c]) fail(RWKV_ERR_INVALID, "dfa: state 0 is DEAD, its row is all zeros");
        const size_t cells = (size_t)n_states * 256;
        for (size_t k = 256; k < cells; ++k) if (trans[k] >= n_states) fail(RWKV_ERR_INVALID, "dfa: a transition leaves the table");
        std::vector<uint8_t> acc(accepting, accepting + n_states);
        for (auto &a : acc) a = a ? 1 : 0;
        *out = finish_table(std::vector<uint16_t>(trans, trans + cells), std::move(acc), n_states, start).release();
    });
}

rwkv_status rwkv_dfa_compile(const uint8_t *pattern, size_t len, rwkv_dfa **out) {
    return dfa_guard([&] {
        if (!out) fail(RWKV_ERR_INVALID, "dfa: null out");
        *out = nullptr;
        if (!pattern && len) fail(RWKV_ERR_INVALID, "dfa: null pattern");
        *out = compile(pattern, len).release();
    });
}

void rwkv_dfa_free(rwkv_dfa *d) { delete d; }
int32_t rwkv_dfa_num_states(const rwkv_dfa *d) { return d ? d->n_states : 0; }
int32_t rwkv_dfa_start(const rwkv_dfa *d) { return d ? d->start : 0; }

rwkv_status rwkv_dfa_table(const rwkv_dfa *d, uint16_t *trans, uint8_t *accepting) {
    return dfa_guard([&] {
        if (!d) fail(RWKV_ERR_INVALID, "dfa: null handle");
        if (trans) std::memcpy(trans, d->trans.data(), d->trans.size() * sizeof(uint16_t));
        if (accepting) std::memcpy(accepting, d->accepting.data(), d->accepting.size());
    });
}

rwkv_status rwkv_dfa_walk(const rwkv_dfa *d, int32_t state, const uint8_t *bytes, size_t n, int32_t *next) {
    return dfa_guard([&] {
        check_state(d, state);
        if (!next || (n && !bytes)) fail(RWKV_ERR_INVALID, "dfa: null bytes / next");
        unsigned q = (unsigned)state;
        for (size_t at = 0; at < n && q; at += 1u << 30) q = rwkv::gen_dfa_walk(d->trans.data(), q, bytes + at, (int)std::min<size_t>(n - at, 1u << 30));
        *next = (int32_t)q;
    });
}

rwkv_status rwkv_dfa_allow(const rwkv_dfa *d, int32_t state, const uint8_t *bytes, const int32_t *lens, size_t n_tokens, uint8_t *allow,
                           size_t num_vocab) {
    return dfa_guard([&] {
        check_state(d, state);
        if (!allow && num_vocab) fail(RWKV_ERR_INVALID, "dfa: null allow");
        if (!lens && n_tokens) fail(RWKV_ERR_INVALID, "dfa: null lens");
        if (n_tokens >= 0x7fffffffu) fail(RWKV_ERR_INVALID, "dfa: too many tokens");
        // the table in the engine's form (rwkv_gen_set_token_bytes), so that gen_dfa_token_end reads here what the kernel reads
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
        for (size_t v = 0; v < num_vocab; ++v)
            allow[v] = v < n_tokens && rwkv::gen_dfa_token_end(d->trans.data(), (unsigned)state, off.data(), bytes, (int)n_tokens, (int)v) ? 1 : 0;
    });
}

rwkv_status rwkv_dfa_check_live(const rwkv_dfa *d, int32_t state, int32_t halt_mode, const int32_t *lens, const uint8_t *bytes, size_t n_tokens) {
    return dfa_guard([&] {
        check_state(d, state);
        if (state == 0) fail(RWKV_ERR_INVALID, "dfa: state 0 is dead");
        if (halt_mode != RWKV_DFA_HALT_FINAL && halt_mode != RWKV_DFA_HALT_ACCEPT) fail(RWKV_ERR_INVALID, "dfa: unknown halt mode");
        if (!lens && n_tokens) fail(RWKV_ERR_INVALID, "dfa: null lens");
        uint8_t single[256] = {};
        size_t at = 0;
        for (size_t i = 0; i < n_tokens; ++i) {
            if (lens[i] < -1) fail(RWKV_ERR_INVALID, "token table: negative length");
            if (lens[i] > 0 && !bytes) fail(RWKV_ERR_INVALID, "token table: null bytes");
            if (lens[i] == 1 && i > 0) single[bytes[at]] = 1;          // token 0 is never allowed
            if (lens[i] > 0) at += (size_t)lens[i];
        }
        if (!rwkv::dfa_never_stuck(*d, state, halt_mode, single))
            fail(RWKV_ERR_UNSUPPORTED, "constraint: a reachable state has no single-byte token that leads on (a row could be masked whole)");
    });
}

}  // extern "C"

// gen_pda_test.cpp — ai00_server_amd/csrc/gen_pda.h compiled with g++ and driven in the kernels' order: gen_pda_mask (the slot's stack is
// staged once, every token id walks its bytes from the configuration with its own entries in the shift register, a token that is not allowed
// is masked), then gen_post's thread 0 for the drawn token (gen_pda_commit on the real stack, halt predicate, finish decision through
// gen_stop_decide with halt in the first argument).
// Stand-alone: no library, no device.  Prints "gen_pda_test: ok" and exits 0, or says what differed and exits 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ai00_server_amd/csrc/gen_pda.h"

using namespace rwkv;

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// Letters and balanced brackets, by hand: 0 DEAD; 1 TOP (accepts; `a` stays, `[` pushes 1 and goes to 2, `.` ends in 3); 2 IN (`a` and `,`
// stay, `[` pushes 2 and stays, `]` pops); 3 DONE (accepts, nothing leads on).
struct Table {
    std::vector<unsigned short> next, act;
    std::vector<unsigned char> accepting, flags;
    Table() : next(4 * 256, 0), act(4 * 256, 0), accepting(4, 0), flags(4, 0) {
        n(1, 'a') = 1; n(1, '[') = 2; a(1, '[') = 1; n(1, '.') = 3;
        n(2, 'a') = 2; n(2, ',') = 2; n(2, '[') = 2; a(2, '[') = 2; a(2, ']') = (unsigned short)GEN_PDA_POP;
        accepting[1] = accepting[3] = 1;
        for (unsigned q = 0; q < 4; ++q) flags[q] = gen_pda_flags(next.data(), act.data(), accepting.data(), q);
    }
    unsigned short &n(int q, int c) { return next[(size_t)q * 256 + (size_t)c]; }
    unsigned short &a(int q, int c) { return act[(size_t)q * 256 + (size_t)c]; }
};

// the token table in the engine's form (rwkv_gen_set_token_bytes): nullptr = unknown id
struct Tokens {
    std::vector<unsigned> off;
    std::vector<unsigned char> bytes;
    explicit Tokens(const std::vector<const char *> &words) {
        for (const char *w : words) {
            off.push_back((unsigned)bytes.size() | (w ? 0u : GEN_TOK_UNKNOWN));
            if (w) bytes.insert(bytes.end(), w, w + std::strlen(w));
        }
        off.push_back((unsigned)bytes.size());
    }
    int n() const { return (int)off.size() - 1; }
};

struct Slot {
    int state, depth, mode, max_depth;
    unsigned short stack[GEN_PDA_MAX_DEPTH];
    int emitted, max_tokens, finish;
    Slot(int q, std::vector<int> st, int mode_, int max_depth_, int max_tokens_ = 100)
        : state(q), depth((int)st.size()), mode(mode_), max_depth(max_depth_), stack{}, emitted(0), max_tokens(max_tokens_), finish(0) {
        for (size_t i = 0; i < st.size(); ++i) stack[i] = (unsigned short)st[i];
    }
    std::vector<int> config() const { std::vector<int> c{state}; for (int i = 0; i < depth; ++i) c.push_back(stack[i]); return c; }
};

// the same bytes one at a time on a real stack: what every allowed token must agree with
static std::vector<int> bytewise(const Table &t, const Slot &s, const std::string &bytes) {
    unsigned short st[GEN_PDA_MAX_DEPTH];
    std::memcpy(st, s.stack, sizeof(st));
    int d = s.depth;
    unsigned q = (unsigned)s.state;
    for (unsigned char b : bytes) q = gen_pda_step(t.next.data(), t.act.data(), s.max_depth, q, st, &d, b);
    std::vector<int> c{(int)q};
    for (int i = 0; i < d; ++i) c.push_back(st[i]);
    return c;
}

// one step of a slot: gen_pda_mask over V ids against a staged copy of the stack, then gen_post's thread 0 for the token `tok`
static std::vector<char> step(const Table &t, const Tokens &k, int V, Slot &s, int tok) {
    unsigned short staged[GEN_PDA_MAX_DEPTH];
    std::memcpy(staged, s.stack, sizeof(staged));
    std::vector<char> allowed((size_t)V);
    for (int v = 0; v < V; ++v)
        allowed[(size_t)v] = gen_pda_token_end(t.next.data(), t.act.data(), s.max_depth, (unsigned)s.state, staged, s.depth, k.off.data(), k.bytes.data(), k.n(), v).state != 0;
    CHECK(std::memcmp(staged, s.stack, sizeof(staged)) == 0);                       // the mask reads the stack, it never writes it
    const bool halt = gen_pda_commit(t.next.data(), t.act.data(), t.flags.data(), s.max_depth, s.mode, &s.state, s.stack, &s.depth, k.off.data(),
                                     k.bytes.data(), k.n(), tok >= 0 && tok < V ? tok : -1);
    s.emitted += 1;
    s.finish = gen_stop_decide(halt || tok == 0, true, false, s.emitted >= s.max_tokens);
    return allowed;
}

int main() {
    const Table t;
    const std::string longw = "[" + std::string(GEN_TOKEN_LEN - 2, 'a') + "]";
    //                0    1    2    3     4      5           6            7        8   9     10    11             12            13   14
    const Tokens k({"a", "a", "[", "]", "],[", "[[[[[[[[", "[[[[[[[[[", nullptr, "", "]]", "[]", longw.c_str(), "][[[[[[[[", ".", "]]]["});
    const int V = 20;                                            // ids 15 .. 19 are past the table: never allowed
    const std::vector<std::string> words = {"a", "a", "[", "]", "],[", "[[[[[[[[", "[[[[[[[[[", "", "", "]]", "[]", longw, "][[[[[[[[", ".", "]]]["};
    CHECK((int)longw.size() == GEN_TOKEN_LEN);

    // the flag bytes: END counts plain and push entries, not pops
    CHECK(t.flags[0] == GEN_PDA_END && t.flags[1] == GEN_PDA_ACCEPT && t.flags[2] == 0 && t.flags[3] == (GEN_PDA_ACCEPT | GEN_PDA_END));

    // depth 0, the start: `a`, `[`, eight `[` in one token, `[]`, the 256-byte token and `.`; never id 0 (the same bytes as id 1), the
    // unknown id, the empty token, ids past the table.  NINE `[` own nine entries: the span rule, though max_depth = 64 has room
    {
        Slot s(1, {}, GEN_PDA_HALT_FINAL, 64);
        const auto al = step(t, k, V, s, 5);
        const char want[20] = {0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0};
        for (int v = 0; v < V; ++v) CHECK(al[(size_t)v] == want[v]);
        CHECK((s.config() == std::vector<int>{2, 1, 2, 2, 2, 2, 2, 2, 2}) && s.finish == GEN_FIN_RUNNING);   // exactly 8 own entries, committed
        CHECK(gen_pda_token_end(t.next.data(), t.act.data(), 64, 1, s.stack, 0, k.off.data(), k.bytes.data(), k.n(), -1).state == 0);
        CHECK(gen_pda_token_end(t.next.data(), t.act.data(), 64, 0, s.stack, 0, k.off.data(), k.bytes.data(), k.n(), 1).state == 0);   // nothing in DEAD
    }
    // every allowed token ends where the byte-wise walk on a real stack ends; a token that is not allowed leaves the configuration alone
    for (const std::vector<int> &st : {std::vector<int>{}, std::vector<int>{1}, std::vector<int>{1, 2}, std::vector<int>{1, 2, 2}}) {
        for (int q : {1, 2}) {
            if ((q == 1) != st.empty()) continue;
            for (int tok = -1; tok < V + 2; ++tok) {
                Slot s(q, st, GEN_PDA_HALT_ACCEPT, 12);
                const Slot before = s;
                const auto al = step(t, k, V, s, tok);
                const bool ok = tok >= 0 && tok < V && al[(size_t)tok];
                if (!ok) { CHECK(s.config() == before.config() && s.finish == (tok == 0 ? GEN_FIN_STOP : GEN_FIN_RUNNING)); continue; }
                CHECK(s.config() == bytewise(t, before, words[(size_t)tok]));
                CHECK((s.finish == GEN_FIN_STOP) == (s.depth == 0 && t.accepting[(size_t)s.state]));
            }
        }
    }
    // pop on an empty stack: state 2 with nothing under it
    {
        Slot s(2, {}, GEN_PDA_HALT_FINAL, 64);
        const auto al = step(t, k, V, s, 3);
        CHECK(!al[3] && !al[9] && !al[4] && al[1] && al[2] && (s.config() == std::vector<int>{2}));
    }
    // push at max_depth = 3: `[` is dead, `a` and `]` are not, and `],[` pops first and so has room again
    {
        Slot s(2, {1, 2, 2}, GEN_PDA_HALT_FINAL, 3);
        const auto al = step(t, k, V, s, 4);
        CHECK(!al[2] && !al[5] && !al[10] && al[1] && al[3] && al[4] && al[9] && !al[11]);
        CHECK((s.config() == std::vector<int>{2, 1, 2, 2}));
    }
    // a token that pops below its start depth and then pushes: `],[` from depth 2 ends at depth 2 over a NEW entry; from depth 1 the pop
    // uncovers TOP, where `,` is dead; `]]][` from depth 3 pops three and pushes on the empty stack
    {
        Slot s(2, {1, 2}, GEN_PDA_HALT_FINAL, 64);
        step(t, k, V, s, 4);
        CHECK((s.config() == std::vector<int>{2, 1, 2}));
        Slot u(2, {1}, GEN_PDA_HALT_FINAL, 64);
        const auto al = step(t, k, V, u, 4);
        CHECK(!al[4] && !al[9] && al[3] && (u.config() == std::vector<int>{2, 1}));
        Slot w(2, {1, 2, 2}, GEN_PDA_HALT_FINAL, 64);
        step(t, k, V, w, 14);
        CHECK((w.config() == std::vector<int>{2, 1}));
    }
    // the span counts from the LOWEST depth the token reached: `]` and eight `[` is allowed, and at max_depth = 9 from depth 2 it just fits
    {
        Slot s(2, {1, 2}, GEN_PDA_HALT_FINAL, 9);
        const auto al = step(t, k, V, s, 12);
        CHECK(al[12] && !al[6] && !al[5] && (s.config() == std::vector<int>{2, 1, 2, 2, 2, 2, 2, 2, 2, 2}));
    }
    // both halt modes: `[]` returns to TOP with an empty stack — ACCEPT halts, FINAL does not (`a` leads on); `.` is FINAL; inside a bracket
    // nothing halts; max_tokens gives LENGTH; token 0 still stops
    {
        Slot f(1, {}, GEN_PDA_HALT_FINAL, 64, 3), a(1, {}, GEN_PDA_HALT_ACCEPT, 64, 3);
        step(t, k, V, f, 10);
        step(t, k, V, a, 10);
        CHECK(f.finish == GEN_FIN_RUNNING && a.finish == GEN_FIN_STOP && (f.config() == std::vector<int>{1}));
        step(t, k, V, f, 2);
        CHECK(f.finish == GEN_FIN_RUNNING && (f.config() == std::vector<int>{2, 1}));
        step(t, k, V, f, 1);
        CHECK(f.finish == GEN_FIN_LENGTH);
        Slot g(1, {}, GEN_PDA_HALT_FINAL, 64);
        step(t, k, V, g, 13);
        CHECK(g.finish == GEN_FIN_STOP && (g.config() == std::vector<int>{3}));
        Slot z(2, {1}, GEN_PDA_HALT_ACCEPT, 64);
        step(t, k, V, z, 0);
        CHECK(z.finish == GEN_FIN_STOP && (z.config() == std::vector<int>{2, 1}));
    }
    // a token of exactly GEN_TOKEN_LEN bytes is walked whole
    {
        Slot s(1, {}, GEN_PDA_HALT_ACCEPT, 64);
        step(t, k, V, s, 11);
        CHECK((s.config() == std::vector<int>{1}) && s.finish == GEN_FIN_STOP);
    }
    if (failures) { std::printf("gen_pda_test: %d checks failed\n", failures); return 1; }
    std::printf("gen_pda_test: ok\n");
    return 0;
}

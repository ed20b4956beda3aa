// gen_dfa_test.cpp — ai00_server_amd/csrc/gen_dfa.h compiled with g++ and driven in the kernels' order: gen_mask (every token id walks its
// bytes from the slot's state, the end state is kept, a token that is not allowed is masked), then gen_post's thread 0 for the drawn token
// (advance by one load, halt predicate, finish decision through gen_stop_decide with halt in the first argument).
// Stand-alone: no library, no device.  Prints "gen_dfa_test: ok" and exits 0, or says what differed and exits 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ai00_server_amd/csrc/gen_dfa.h"

using namespace rwkv;

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// the automaton of  ab*c | d  by hand: 0 DEAD, 1 start, 2 after a (b loops), 3 after c (accepts, no way on), 4 after d (accepts, e loops)
struct Table {
    std::vector<unsigned short> trans;
    std::vector<unsigned char> accepting, flags;
    Table() : trans(5 * 256, 0), accepting(5, 0), flags(5, 0) {
        at(1, 'a') = 2; at(2, 'b') = 2; at(2, 'c') = 3; at(1, 'd') = 4; at(4, 'e') = 4;
        accepting[3] = accepting[4] = 1;
        for (unsigned q = 0; q < 5; ++q) flags[q] = gen_dfa_flags(trans.data(), accepting.data(), q);
    }
    unsigned short &at(int q, int c) { return trans[(size_t)q * 256 + (size_t)c]; }
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

struct Slot { unsigned state; int mode; int emitted, max_tokens, finish; };

// one step of a slot: gen_mask over V ids, then gen_post's thread 0 for the token `tok` the sampler drew
static std::vector<unsigned short> step(const Table &t, const Tokens &k, int V, Slot &s, int tok, std::vector<float> *logits = nullptr) {
    std::vector<unsigned short> end((size_t)V);
    for (int v = 0; v < V; ++v) {
        end[(size_t)v] = (unsigned short)gen_dfa_token_end(t.trans.data(), s.state, k.off.data(), k.bytes.data(), k.n(), v);
        if (logits && !end[(size_t)v]) (*logits)[(size_t)v] = -1.0f / 0.0f;
    }
    const unsigned e = tok >= 0 && tok < V ? end[(size_t)tok] : 0u;
    s.state = gen_dfa_advance(s.state, e);
    const bool halt = gen_dfa_halt(e, e ? t.flags[e] : (unsigned char)0, s.mode);
    s.emitted += 1;
    const bool stop_token = tok == 0;
    s.finish = gen_stop_decide(halt || stop_token, true, false, s.emitted >= s.max_tokens);
    return end;
}

int main() {
    const Table t;
    //                0     1    2    3    4     5      6    7        8    9
    const Tokens k({"a", "a", "b", "c", "bc", "abbc", "d", nullptr, "", "e"});
    const int V = 16;                                            // ids 10 .. 15 are past the table: never allowed

    // the flag bytes
    CHECK(t.flags[0] == GEN_DFA_END && t.flags[1] == 0 && t.flags[2] == 0);
    CHECK(t.flags[3] == (GEN_DFA_ACCEPT | GEN_DFA_END) && t.flags[4] == GEN_DFA_ACCEPT);

    // the walk: DEAD absorbs, an empty walk stays
    const unsigned char abbc[] = {'a', 'b', 'b', 'c'}, abx[] = {'a', 'b', 'x', 'c'};
    CHECK(gen_dfa_walk(t.trans.data(), 1, abbc, 4) == 3 && gen_dfa_walk(t.trans.data(), 1, abbc, 3) == 2 && gen_dfa_walk(t.trans.data(), 1, abbc, 0) == 1);
    CHECK(gen_dfa_walk(t.trans.data(), 1, abx, 4) == 0 && gen_dfa_walk(t.trans.data(), 0, abbc, 4) == 0 && gen_dfa_walk(t.trans.data(), 3, abbc, 1) == 0);

    // the allowed predicate in the start state: "a" (ids 0 and 1 hold the same bytes, but token 0 is the end-of-sequence id and never
    // allowed), "abbc", "d"; never the unknown id, the empty token, ids past the table
    {
        Slot s{1, GEN_DFA_HALT_FINAL, 0, 100, 0};
        std::vector<float> x((size_t)V, 0.5f);
        const auto end = step(t, k, V, s, 5, &x);
        const unsigned short want[16] = {0, 2, 0, 0, 0, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int v = 0; v < V; ++v) {
            CHECK(end[(size_t)v] == want[v]);
            CHECK((x[(size_t)v] == 0.5f) == (want[v] != 0));
            CHECK(want[v] != 0 || x[(size_t)v] < -1e38f);
        }
        CHECK(gen_dfa_token_end(t.trans.data(), 1, k.off.data(), k.bytes.data(), k.n(), -1) == 0);
        CHECK(gen_dfa_token_end(t.trans.data(), 0, k.off.data(), k.bytes.data(), k.n(), 1) == 0);       // nothing is allowed in DEAD
        // "abbc" was drawn: state 3 accepts and has no way on: HALT_FINAL halts, the token is the slot's last
        CHECK(s.state == 3 && s.finish == GEN_FIN_STOP && s.emitted == 1);
    }
    // both halt modes over  d e e : ACCEPT halts at once, FINAL never (e always leads on) and runs into max_tokens
    {
        Slot f{1, GEN_DFA_HALT_FINAL, 0, 3, 0}, a{1, GEN_DFA_HALT_ACCEPT, 0, 3, 0};
        step(t, k, V, f, 6);
        step(t, k, V, a, 6);
        CHECK(f.state == 4 && f.finish == GEN_FIN_RUNNING && a.state == 4 && a.finish == GEN_FIN_STOP);
        step(t, k, V, f, 9);
        CHECK(f.state == 4 && f.finish == GEN_FIN_RUNNING);
        step(t, k, V, f, 9);
        CHECK(f.state == 4 && f.finish == GEN_FIN_LENGTH);
    }
    // a rejected token keeps the state and does not halt, in either mode — even when the state it was drawn in accepts
    for (int mode : {GEN_DFA_HALT_FINAL, GEN_DFA_HALT_ACCEPT}) {
        Slot s{2, mode, 0, 100, 0};
        for (int tok : {1, 6, 7, 8, 12, 99}) {                    // "a" and "d" die from state 2; unknown, empty, past the table, past V
            step(t, k, V, s, tok);
            CHECK(s.state == 2 && s.finish == GEN_FIN_RUNNING);
        }
        Slot acc{4, mode, 0, 100, 0};
        step(t, k, V, acc, 1);
        CHECK(acc.state == 4 && acc.finish == GEN_FIN_RUNNING);
        step(t, k, V, s, 4);                                        // "bc" from state 2: accepted, final
        CHECK(s.state == 3 && s.finish == GEN_FIN_STOP);
    }
    // token 0 still stops (run.rs:855) whatever the automaton says, and halt beats a full stop buffer (first argument of gen_stop_decide)
    {
        Slot s{2, GEN_DFA_HALT_FINAL, 0, 100, 0};
        step(t, k, V, s, 0);
        CHECK(s.state == 2 && s.finish == GEN_FIN_STOP);
        CHECK(gen_stop_decide(true, false, false, false) == GEN_FIN_STOP && gen_stop_decide(false, false, false, false) == GEN_FIN_HANDBACK);
    }
    // a token of exactly GEN_TOKEN_LEN bytes is walked whole
    {
        std::string longw = "a" + std::string(GEN_TOKEN_LEN - 2, 'b') + "c";
        const Tokens big({"x", longw.c_str()});
        CHECK((int)longw.size() == GEN_TOKEN_LEN);
        CHECK(gen_dfa_token_end(t.trans.data(), 1, big.off.data(), big.bytes.data(), big.n(), 1) == 3);
    }
    if (failures) { std::printf("gen_dfa_test: %d checks failed\n", failures); return 1; }
    std::printf("gen_dfa_test: ok\n");
    return 0;
}

// fuzz_dfa.cpp — a stand-alone program (its own main) over the host functions of ai00_server_amd/csrc/rwkv_dfa.cpp: mutated patterns
// through rwkv_dfa_compile, mutated tables through rwkv_dfa_from_table, and walks / masks over whatever handle comes back.  Every call must
// answer with a status; nothing may abort.  Compiled TOGETHER with rwkv_dfa.cpp (no library) so that -fsanitize=address,undefined sees the
// compiler's own code: tests/test_dfa_cpu.py builds and runs it that way.
//     fuzz_dfa <iterations> [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rwkv_abi.h"

// the error slot of the library, which this program stands in for
static std::string g_err;
extern "C" void rwkv_set_last_error(const char *msg) { g_err = msg ? msg : ""; }
extern "C" const char *rwkv_last_error(void) { return g_err.c_str(); }

static uint64_t rng_state = 1;
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static size_t below(size_t n) { return n ? (size_t)(rnd() % n) : 0; }

static const char *SEEDS[] = {
    "abc", "a{2,5}b*", "(ab|cd)+e?", "[a-z0-9_]+@[a-z]+\\.(com|org)", "\\d{4}-\\d{2}-\\d{2}", "\"([^\"\\\\]|\\\\[\"\\\\/bfnrt])*\"",
    "\\{\"name\":\"[^\"]*\",\"age\":\\d{1,3}\\}", "(true|false|null)", "-?(0|[1-9]\\d*)(\\.\\d+)?([eE][+-]?\\d+)?", ".*", "[^a-c]{0,3}\xe4\xb8\xad+",
    "(a|b|)*c{255}", "((((a))))", "\\x41\\x7f[\\x00-\\x1f]", "\\w+\\s\\w+", "(a{10}){10}", "[]", "a|", "()",
};
static const char ALPHABET[] = "ab(|)*+?{},0129[]^-\\.dwsx\"/ \n\xe4\xb8\xad\xff\xc2\x80";

static std::string mutate(std::string s) {
    const size_t rounds = 1 + below(4);
    for (size_t r = 0; r < rounds; ++r) {
        switch (below(6)) {
        case 0: if (!s.empty()) s.erase(below(s.size()), 1 + below(3)); break;
        case 1: s.insert(below(s.size() + 1), 1, ALPHABET[below(sizeof(ALPHABET) - 1)]); break;
        case 2: if (!s.empty()) s[below(s.size())] = (char)rnd(); break;
        case 3: if (!s.empty()) { const size_t a = below(s.size()); s.insert(below(s.size() + 1), s.substr(a, 1 + below(8))); } break;
        case 4: s = "(" + s + ")" + "*+?"[below(3)]; break;
        default: s += SEEDS[below(sizeof(SEEDS) / sizeof(SEEDS[0]))]; break;
        }
        if (s.size() > 400) s.resize(400);
    }
    return s;
}

static unsigned long long n_ok = 0, n_invalid = 0, n_unsupported = 0;

static void count(rwkv_status st, rwkv_dfa *d) {
    if (st == RWKV_OK) ++n_ok; else if (st == RWKV_ERR_INVALID) ++n_invalid; else if (st == RWKV_ERR_UNSUPPORTED) ++n_unsupported;
    else if (st != RWKV_ERR_OOM) { std::printf("unexpected status %d: %s\n", (int)st, rwkv_last_error()); std::exit(1); }
    if ((st == RWKV_OK) != (d != nullptr)) { std::printf("status %d with handle %p\n", (int)st, (void *)d); std::exit(1); }
    if (st != RWKV_OK && !*rwkv_last_error()) { std::printf("status %d without a message\n", (int)st); std::exit(1); }
}

// a handle that came back must be a table rwkv_dfa_from_table accepts, and walks / masks over it (bad states included) answer with statuses
static void exercise(rwkv_dfa *d) {
    const int32_t n = rwkv_dfa_num_states(d), start = rwkv_dfa_start(d);
    std::vector<uint16_t> trans((size_t)n * 256);
    std::vector<uint8_t> acc((size_t)n);
    if (rwkv_dfa_table(d, trans.data(), acc.data()) != RWKV_OK) { std::printf("rwkv_dfa_table failed\n"); std::exit(1); }
    rwkv_dfa *again = nullptr;
    if (rwkv_dfa_from_table(trans.data(), acc.data(), n, start, &again) != RWKV_OK) { std::printf("a returned table is refused: %s\n", rwkv_last_error()); std::exit(1); }
    rwkv_dfa_free(again);
    uint8_t bytes[64];
    for (auto &b : bytes) b = (uint8_t)rnd();
    int32_t next = -1;
    for (int32_t state : {start, (int32_t)below((size_t)n), (int32_t)0, (int32_t)-1, n, (int32_t)0x7fffffff}) {
        const rwkv_status st = rwkv_dfa_walk(d, state, bytes, below(sizeof(bytes)), &next);
        if (st == RWKV_OK && (next < 0 || next >= n)) { std::printf("walk left the table\n"); std::exit(1); }
        // a small token table: unknown ids, empty tokens, fewer tokens than the vocabulary
        int32_t lens[8];
        size_t total = 0;
        for (auto &l : lens) { l = (int32_t)below(9) - 1; if (below(40) == 0) l = 300; if (below(40) == 0) l = -5; if (l > 0 && l <= 256) total += (size_t)l; }
        std::vector<uint8_t> tb(total + 1);
        for (auto &b : tb) b = (uint8_t)rnd();
        uint8_t allow[12];
        (void)rwkv_dfa_allow(d, state, tb.data(), lens, 8, allow, sizeof(allow));
    }
}

int main(int argc, char **argv) {
    const long iters = argc > 1 ? std::atol(argv[1]) : 2000;
    rng_state = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    for (long it = 0; it < iters; ++it) {
        rwkv_dfa *d = nullptr;
        if (it % 4 != 3) {
            const std::string pat = it < (long)(sizeof(SEEDS) / sizeof(SEEDS[0])) ? SEEDS[it] : mutate(SEEDS[below(sizeof(SEEDS) / sizeof(SEEDS[0]))]);
            const rwkv_status st = rwkv_dfa_compile((const uint8_t *)pat.data(), pat.size(), &d);
            count(st, d);
        } else {
            // a random table: mostly valid targets, sometimes one past the end, a live state 0, a bad start, a bad size
            const int32_t n = (int32_t)(2 + below(40));
            std::vector<uint16_t> trans((size_t)n * 256, 0);
            std::vector<uint8_t> acc((size_t)n, 0);
            for (size_t k = 256; k < trans.size(); ++k) if (below(8) == 0) trans[k] = (uint16_t)below((size_t)n);
            for (auto &a : acc) a = (uint8_t)(below(3) == 0);
            acc[0] = 0;
            int32_t start = (int32_t)(1 + below((size_t)n - 1)), size = n;
            switch (below(8)) {
            case 0: trans[256 + below(trans.size() - 256)] = (uint16_t)(n + below(3)); break;
            case 1: trans[below(256)] = 1; break;
            case 2: acc[0] = 1; break;
            case 3: start = (int32_t)below(3) == 0 ? 0 : below(2) ? n : -1; break;
            case 4: size = (int32_t)below(2); break;
            default: break;
            }
            const rwkv_status st = rwkv_dfa_from_table(trans.data(), acc.data(), size, start, &d);
            count(st, d);
        }
        if (d) exercise(d);
        rwkv_dfa_free(d);
    }
    {   // the limit itself: 4096 states load, 4097 are refused as unsupported; null arguments are statuses
        std::vector<uint16_t> trans((size_t)4097 * 256, 0);
        std::vector<uint8_t> acc(4097, 0);
        rwkv_dfa *d = nullptr;
        if (rwkv_dfa_from_table(trans.data(), acc.data(), 4096, 4095, &d) != RWKV_OK || !d) { std::printf("4096 states refused\n"); return 1; }
        rwkv_dfa_free(d);
        if (rwkv_dfa_from_table(trans.data(), acc.data(), 4097, 1, &d) != RWKV_ERR_UNSUPPORTED || d) { std::printf("4097 states not refused\n"); return 1; }
        if (rwkv_dfa_from_table(nullptr, acc.data(), 2, 1, &d) != RWKV_ERR_INVALID || rwkv_dfa_compile(nullptr, 3, &d) != RWKV_ERR_INVALID ||
            rwkv_dfa_compile((const uint8_t *)"a", 1, nullptr) != RWKV_ERR_INVALID || rwkv_dfa_walk(nullptr, 1, nullptr, 0, nullptr) != RWKV_ERR_INVALID) {
            std::printf("a null argument was not refused\n");
            return 1;
        }
        rwkv_dfa_free(nullptr);
    }
    std::printf("fuzz_dfa: %ld iterations, %llu ok, %llu invalid, %llu unsupported: no crash\n", iters, n_ok, n_invalid, n_unsupported);
    return n_ok && n_invalid && n_unsupported ? 0 : 1;
}

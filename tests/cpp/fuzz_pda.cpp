// fuzz_pda.cpp — a stand-alone program (its own main) over the host functions of ai00_server_amd/csrc/rwkv_pda.cpp: random tables through
// rwkv_pda_from_table (mostly valid, sometimes broken in one of the ways the header lists), rwkv_pda_json with good and bad arguments, and
// walks / masks / liveness checks over whatever handle comes back, from good and bad configurations.  Every call must answer with a status;
// nothing may abort.  Compiled TOGETHER with rwkv_pda.cpp (no library) so that -fsanitize=address,undefined sees the code under test:
// tests/test_pda_cpu.py builds and runs it that way.
//     fuzz_pda <iterations> [seed]
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

static unsigned long long n_ok = 0, n_invalid = 0, n_unsupported = 0;

static void count(rwkv_status st, rwkv_pda *p) {
    if (st == RWKV_OK) ++n_ok; else if (st == RWKV_ERR_INVALID) ++n_invalid; else if (st == RWKV_ERR_UNSUPPORTED) ++n_unsupported;
    else if (st != RWKV_ERR_OOM) { std::printf("unexpected status %d: %s\n", (int)st, rwkv_last_error()); std::exit(1); }
    if ((st == RWKV_OK) != (p != nullptr)) { std::printf("status %d with handle %p\n", (int)st, (void *)p); std::exit(1); }
    if (st != RWKV_OK && !*rwkv_last_error()) { std::printf("status %d without a message\n", (int)st); std::exit(1); }
}

// a handle that came back must be a table rwkv_pda_from_table accepts, and walks / masks / liveness checks over it answer with statuses
static void exercise(rwkv_pda *p) {
    const int32_t n = rwkv_pda_num_states(p), start = rwkv_pda_start(p), max_depth = rwkv_pda_max_depth(p);
    std::vector<uint16_t> next((size_t)n * 256), act((size_t)n * 256);
    std::vector<uint8_t> acc((size_t)n);
    if (rwkv_pda_table(p, next.data(), act.data(), acc.data()) != RWKV_OK) { std::printf("rwkv_pda_table failed\n"); std::exit(1); }
    rwkv_pda *again = nullptr;
    if (rwkv_pda_from_table(next.data(), act.data(), acc.data(), n, start, max_depth, &again) != RWKV_OK) { std::printf("a returned table is refused: %s\n", rwkv_last_error()); std::exit(1); }
    rwkv_pda_free(again);
    static const char ALPHABET[] = "[]{}\",:ab01-.e \n\\u\xc3\xa9\xff";
    for (int round = 0; round < 6; ++round) {
        // a configuration: mostly valid, sometimes a bad state, a bad depth or a bad stack entry
        uint16_t stack[RWKV_PDA_MAX_DEPTH + 4];
        int32_t depth = (int32_t)below((size_t)max_depth + 1), state = round == 0 ? start : (int32_t)below((size_t)n);
        for (auto &e : stack) e = (uint16_t)(1 + below((size_t)n - 1));
        switch (below(10)) {
        case 0: state = below(2) ? n : -1; break;
        case 1: depth = below(2) ? max_depth + 1 : -1; break;
        case 2: if (depth) stack[below((size_t)depth)] = (uint16_t)(below(2) ? 0 : n + below(3)); break;
        default: break;
        }
        uint8_t bytes[96];
        for (auto &b : bytes) b = below(4) ? (uint8_t)ALPHABET[below(sizeof(ALPHABET) - 1)] : (uint8_t)rnd();
        int32_t q = -1, d = -1;
        uint16_t out[RWKV_PDA_MAX_DEPTH];
        const rwkv_status st = rwkv_pda_walk(p, state, stack, depth, bytes, below(sizeof(bytes)), &q, out, &d);
        if (st == RWKV_OK) {
            if (q < 0 || q >= n || d < 0 || d > max_depth) { std::printf("walk left the table or the stack\n"); std::exit(1); }
            for (int32_t i = 0; i < d; ++i) if (out[i] < 1 || out[i] >= n) { std::printf("walk pushed a state outside the table\n"); std::exit(1); }
        }
        // a small token table: unknown ids, empty tokens, single bytes, fewer tokens than the vocabulary
        int32_t lens[10];
        size_t total = 0;
        for (auto &l : lens) { l = (int32_t)below(12) - 1; if (below(40) == 0) l = 300; if (below(40) == 0) l = -5; if (l > 0 && l <= 256) total += (size_t)l; }
        std::vector<uint8_t> tb(total + 1);
        for (auto &b : tb) b = below(3) ? (uint8_t)ALPHABET[below(sizeof(ALPHABET) - 1)] : (uint8_t)rnd();
        uint8_t allow[14];
        (void)rwkv_pda_allow(p, state, stack, depth, tb.data(), lens, 10, allow, sizeof(allow));
        const rwkv_status live = rwkv_pda_check_live(p, state, stack, depth, lens, tb.data(), 10);
        if (live != RWKV_OK && live != RWKV_ERR_INVALID && live != RWKV_ERR_UNSUPPORTED) { std::printf("check_live: status %d\n", (int)live); std::exit(1); }
    }
}

int main(int argc, char **argv) {
    const long iters = argc > 1 ? std::atol(argv[1]) : 2000;
    rng_state = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    for (long it = 0; it < iters; ++it) {
        rwkv_pda *p = nullptr;
        if (it % 8 == 7) {
            const uint32_t flags = below(6) ? (uint32_t)below(4) : (uint32_t)rnd();
            const int32_t max_depth = below(6) ? (int32_t)(1 + below(RWKV_PDA_MAX_DEPTH)) : (int32_t)below(200) - 60;
            const rwkv_status st = rwkv_pda_json(flags, max_depth, &p);
            count(st, p);
        } else {
            // a random table over a small alphabet: plain, push and pop entries; sometimes broken in one way
            const int32_t n = (int32_t)(2 + below(30));
            std::vector<uint16_t> next((size_t)n * 256, 0), act((size_t)n * 256, 0);
            std::vector<uint8_t> acc((size_t)n, 0);
            for (size_t k = 256; k < next.size(); ++k) {
                const size_t kind = below(24);
                if (kind == 0) next[k] = (uint16_t)below((size_t)n);
                else if (kind == 1) { next[k] = (uint16_t)(1 + below((size_t)n - 1)); act[k] = (uint16_t)(1 + below((size_t)n - 1)); }
                else if (kind == 2) { act[k] = (uint16_t)RWKV_PDA_POP; next[k] = (uint16_t)rnd(); }      // `next` of a pop is ignored
            }
            for (auto &a : acc) a = (uint8_t)(below(3) == 0);
            acc[0] = 0;
            int32_t start = (int32_t)(1 + below((size_t)n - 1)), size = n, max_depth = (int32_t)(1 + below(RWKV_PDA_MAX_DEPTH));
            const size_t cell = 256 + below(next.size() - 256);
            switch (below(12)) {
            case 0: next[cell] = (uint16_t)(n + below(3)); act[cell] = 0; break;
            case 1: (below(2) ? next : act)[below(256)] = 1; break;
            case 2: acc[0] = 1; break;
            case 3: start = (int32_t)below(3) == 0 ? 0 : below(2) ? n : -1; break;
            case 4: size = (int32_t)below(2); break;
            case 5: act[cell] = (uint16_t)(n + below(100)); next[cell] = 1; break;                      // a return state outside the table
            case 6: act[cell] = 1; next[cell] = 0; break;                                               // a push without a target
            case 7: max_depth = below(2) ? 0 : RWKV_PDA_MAX_DEPTH + 1 + (int32_t)below(5); break;
            default: break;
            }
            const rwkv_status st = rwkv_pda_from_table(next.data(), act.data(), acc.data(), size, start, max_depth, &p);
            count(st, p);
        }
        if (p) exercise(p);
        rwkv_pda_free(p);
    }
    {   // the limit itself: 4096 states load, 4097 are refused as unsupported; null arguments are statuses
        std::vector<uint16_t> next((size_t)4097 * 256, 0), act((size_t)4097 * 256, 0);
        std::vector<uint8_t> acc(4097, 0);
        rwkv_pda *p = nullptr;
        if (rwkv_pda_from_table(next.data(), act.data(), acc.data(), 4096, 4095, 64, &p) != RWKV_OK || !p) { std::printf("4096 states refused\n"); return 1; }
        rwkv_pda_free(p);
        if (rwkv_pda_from_table(next.data(), act.data(), acc.data(), 4097, 1, 64, &p) != RWKV_ERR_UNSUPPORTED || p) { std::printf("4097 states not refused\n"); return 1; }
        ++n_unsupported;
        int32_t q = 0, d = 0;
        uint16_t out[RWKV_PDA_MAX_DEPTH];
        if (rwkv_pda_from_table(nullptr, act.data(), acc.data(), 2, 1, 1, &p) != RWKV_ERR_INVALID || rwkv_pda_from_table(next.data(), nullptr, acc.data(), 2, 1, 1, &p) != RWKV_ERR_INVALID ||
            rwkv_pda_json(0, 8, nullptr) != RWKV_ERR_INVALID || rwkv_pda_walk(nullptr, 1, nullptr, 0, nullptr, 0, &q, out, &d) != RWKV_ERR_INVALID ||
            rwkv_pda_allow(nullptr, 1, nullptr, 0, nullptr, nullptr, 0, nullptr, 0) != RWKV_ERR_INVALID ||
            rwkv_pda_check_live(nullptr, 1, nullptr, 0, nullptr, nullptr, 0) != RWKV_ERR_INVALID || rwkv_pda_table(nullptr, nullptr, nullptr, nullptr) != RWKV_ERR_INVALID) {
            std::printf("a null argument was not refused\n");
            return 1;
        }
        rwkv_pda_free(nullptr);
    }
    std::printf("fuzz_pda: %ld iterations, %llu ok, %llu invalid, %llu unsupported: no crash\n", iters, n_ok, n_invalid, n_unsupported);
    return n_ok && n_invalid && n_unsupported ? 0 : 1;
}

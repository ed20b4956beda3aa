// CPU driver of ai00_server_amd/csrc/graph_cache.h for tests/test_graph_cache_cpp.py: integer handles, a deleter that records what it is given.
// usage: graph_cache_test <case>; prints "<case>: ok" and exits 0, or prints what failed and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ai00_server_amd/csrc/graph_cache.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); ++g_fail; } } while (0)

struct Recorder {
    std::vector<int> *log;
    void operator()(int h) const { log->push_back(h); }
};
template <class Key>
using Cache = rwkv::GraphCache<Key, int, Recorder>;

// what the engine does with a key: replay, run directly, or capture (handle = 1000 + key); returns 'r', 'd' or 'c'
static char visit(Cache<uint64_t> &c, uint64_t key) {
    if (c.find(key)) return 'r';
    if (!c.should_capture(key)) return 'd';
    c.insert(key, 1000 + (int)key);
    return 'c';
}

static void second_sight() {
    std::vector<int> log;
    Cache<uint64_t> c(64, Recorder{&log});
    CHECK(visit(c, 7) == 'd');                                   // first sight: run directly, nothing kept
    CHECK(c.find(7) == nullptr);
    CHECK(visit(c, 7) == 'c');                                   // second sight: captured
    CHECK(visit(c, 7) == 'r' && *c.find(7) == 1007);
    CHECK(visit(c, 8) == 'd' && visit(c, 7) == 'r' && visit(c, 8) == 'c');   // another key in between changes nothing
    CHECK(log.empty());
    // a vector key (the generation row sets) behaves the same
    std::vector<int> vlog;
    Cache<std::vector<uint64_t>> v(64, Recorder{&vlog});
    const std::vector<uint64_t> a{5, 1}, b{5, 2};
    CHECK(!v.should_capture(a) && !v.should_capture(b) && v.should_capture(a) && v.should_capture(b));
    v.insert(a, 1);
    CHECK(v.find(a) && *v.find(a) == 1 && !v.find(b));
}

static void evicts_oldest_find() {
    std::vector<int> log;
    Cache<uint64_t> c(64, Recorder{&log});
    for (uint64_t k = 0; k < 64; ++k) c.insert(k, 1000 + (int)k);            // insertion order 0..63
    for (uint64_t k = 0; k < 64; ++k) if (k != 17) CHECK(c.find(k) != nullptr);   // every entry but 17 replayed since: 17 has the oldest use,
    CHECK(log.empty());                                                      // 0 the oldest insert
    c.insert(64, 1064);                                                      // the 65th
    CHECK(log == std::vector<int>{1017});
    CHECK(c.find(17) == nullptr && c.find(0) != nullptr && c.find(64) != nullptr);
    for (uint64_t k = 0; k < 64; ++k) if (k != 17) CHECK(c.find(k) && *c.find(k) == 1000 + (int)k);   // the rest stay, handles intact
}

static void find_refreshes() {
    std::vector<int> log;
    Cache<uint64_t> c(3, Recorder{&log});
    c.insert(1, 11); c.insert(2, 12); c.insert(3, 13);
    CHECK(c.find(1) != nullptr);                                 // 1 is now the most recently used, 2 the least
    c.insert(4, 14);
    CHECK(log == std::vector<int>{12});
    c.insert(5, 15);                                             // then 3 (never found), not 1
    CHECK((log == std::vector<int>{12, 13}));
    CHECK(c.find(1) && c.find(4) && c.find(5) && !c.find(2) && !c.find(3));
    c.insert(6, 16);                                             // uses now: 1, 4, 5 in that order
    CHECK((log == std::vector<int>{12, 13, 11}));
    CHECK(c.should_capture(2) == false);                         // eviction is not "seen": only should_capture records a sight
}

static void seen_set_clears() {
    std::vector<int> log;
    Cache<uint64_t> c(64, Recorder{&log});
    const uint64_t N = Cache<uint64_t>::SEEN_MAX;
    CHECK(N == 4096);
    for (uint64_t k = 0; k < N; ++k) CHECK(!c.should_capture(k));            // 4096 keys seen once: the set is full, not past its bound
    CHECK(c.should_capture(0) && c.should_capture(N - 1));                   // ... and still knows them all
    CHECK(!c.should_capture(N));                                             // the insertion that passes 4096 clears the set
    CHECK(!c.should_capture(0) && !c.should_capture(N - 1));                 // forgotten: first sight again (and recorded again)
    CHECK(c.should_capture(N));                                              // the key that caused the clear is captured on its next visit
    CHECK(c.should_capture(0) && c.should_capture(N - 1));
    CHECK(log.empty());                                                      // the seen-set never touches handles
    c.insert(3, 1003);
    for (uint64_t k = N + 1; k <= 2 * N + 8; ++k) (void)c.should_capture(k); // another clear leaves cached entries alone
    CHECK(c.find(3) && *c.find(3) == 1003 && log.empty());
}

static void deleter_once() {
    std::vector<int> log;
    {
        Cache<uint64_t> c(8, Recorder{&log});
        for (uint64_t k = 0; k < 20; ++k) { c.insert(k, 1000 + (int)k); if (k % 3 == 0) (void)c.find(k / 2); }
        CHECK(log.size() == 12);                                 // 20 inserts into 8 places
        c.clear();
        CHECK(log.size() == 20);
        CHECK(c.find(19) == nullptr);
        c.insert(100, 1100);                                     // usable after clear()
    }                                                            // the destructor releases what is left
    CHECK(log.size() == 21);
    std::vector<int> sorted = log;
    std::sort(sorted.begin(), sorted.end());
    CHECK(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end());     // no handle twice
    for (int k = 0; k < 20; ++k) CHECK(std::binary_search(sorted.begin(), sorted.end(), 1000 + k));
    CHECK(std::binary_search(sorted.begin(), sorted.end(), 1100));
}

static void never_evicts_within_capacity() {
    std::vector<int> log;
    {
        Cache<int> c(4, Recorder{&log});                         // the greedy cache: keyed by slot count, room for every count, captured on first sight
        for (int round = 0; round < 50; ++round)
            for (int n = 1; n <= 4; ++n) {
                if (!c.find(n)) c.insert(n, 10 * n);
                CHECK(*c.find(n) == 10 * n);
            }
        CHECK(log.empty());
    }
    std::sort(log.begin(), log.end());
    CHECK((log == std::vector<int>{10, 20, 30, 40}));            // teardown: each once
}

int main(int argc, char **argv) {
    const std::string want = argc > 1 ? argv[1] : "";
    struct { const char *name; void (*fn)(); } cases[] = {
        {"second_sight", second_sight}, {"evicts_oldest_find", evicts_oldest_find}, {"find_refreshes", find_refreshes},
        {"seen_set_clears", seen_set_clears}, {"deleter_once", deleter_once}, {"never_evicts_within_capacity", never_evicts_within_capacity},
    };
    for (auto &c : cases)
        if (want == c.name) {
            c.fn();
            if (!g_fail) std::printf("%s: ok\n", c.name);
            return g_fail ? 1 : 0;
        }
    std::printf("unknown case '%s'\n", want.c_str());
    return 2;
}

// The record ring of a watch (ai00_server_amd/csrc/gen_watch.h) on the host: the same writer and reader functions gen_publish_kernel and
// rwkv_gen_watch_read use, driven by one thread and by two.  Stand-alone (its own main, no library): built plain, with -fsanitize=thread
// and with -fsanitize=address,undefined by tests/test_gen_watch_cpu.py.
//
//   gen_watch_test single      the single-thread cases: empty ring, in-order reads, ring_steps = 1, a reader exactly ring_steps behind,
//                              one ring_steps + 3 behind, max_steps smaller than what is there; cursor and head after each
//   gen_watch_test nolap [N]   writer and reader threads, ring_steps = N: nothing can be overwritten, so lost == 0 and all N come back
//   gen_watch_test lap [N]     the same with ring_steps = 8 and an unpaced writer: every record returned is whole, the sequence numbers
//                              strictly increase, returned + lost == N
// Every payload word is a fixed function of (sequence, slot, field); word (slot 0, field 0) is the sequence number itself, which is how the
// reader of `lap` knows which records it got.  Prints one line per case and exits non-zero at the first violation.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../ai00_server_amd/csrc/gen_watch.h"

using namespace rwkv;
typedef unsigned long long u64;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static unsigned word(u64 seq, int slot, int field) {
    if (slot == 0 && field == 0) return (unsigned)seq;
    u64 z = seq * 0x9E3779B97F4A7C15ull + (u64)(slot * 3 + field + 1) * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 29;
    return (unsigned)(z * 0x94D049BB133111EBull >> 16);
}

struct Ring {
    int steps, B;
    unsigned char *mem;
    Ring(int steps_, int B_) : steps(steps_), B(B_) {
        const size_t bytes = (gen_watch_bytes(steps, B) + 15) & ~(size_t)15;
        mem = (unsigned char *)std::aligned_alloc(16, bytes);
        REQUIRE(mem);
        std::memset(mem, 0, bytes);
    }
    ~Ring() { std::free(mem); }
    void publish(u64 seq) {                                         // what gen_publish_kernel does, on one thread
        unsigned char *rec = gen_watch_rec(mem, steps, B, seq);
        gen_watch_open_rec(rec);
        for (int b = 0; b < B; ++b) gen_watch_put(rec, B, b, word(seq, b, 0), word(seq, b, 1), (int)word(seq, b, 2));
        gen_watch_commit(rec, gen_watch_head_ptr(mem, steps, B), seq);
    }
    u64 head() const { return gen_watch_head(mem, steps, B); }
};

struct Rows {
    std::vector<unsigned> tok, prob;
    std::vector<int> fin;
    Rows(int max_steps, int B) : tok((size_t)max_steps * B + 1), prob((size_t)max_steps * B + 1), fin((size_t)max_steps * B + 1) {}
};
// row r of a read is record `seq`, word for word
static void require_row(const Rows &rows, int r, int B, u64 seq) {
    for (int b = 0; b < B; ++b) {
        REQUIRE(rows.tok[(size_t)r * B + b] == word(seq, b, 0));
        REQUIRE(rows.prob[(size_t)r * B + b] == word(seq, b, 1));
        REQUIRE(rows.fin[(size_t)r * B + b] == (int)word(seq, b, 2));
    }
}

static void single() {
    const int B = 3;
    {   // empty ring
        Ring r(4, B); Rows rows(8, B);
        u64 cur = 0, lost = 77;
        REQUIRE(gen_watch_read(r.mem, r.steps, B, &cur, 8, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 0);
        REQUIRE(cur == 0 && lost == 0 && r.head() == 0);
    }
    {   // in-order reads, one record at a time and then a batch; probs / finish may be null
        Ring r(4, B); Rows rows(8, B);
        u64 cur = 0, lost = 0;
        for (u64 s = 0; s < 10; ++s) {
            r.publish(s);
            REQUIRE(r.head() == s + 1);
            REQUIRE(gen_watch_read(r.mem, r.steps, B, &cur, 8, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 1);
            REQUIRE(cur == s + 1 && lost == 0);
            require_row(rows, 0, B, s);
            REQUIRE(gen_watch_read(r.mem, r.steps, B, &cur, 8, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 0);
            REQUIRE(cur == s + 1 && lost == 0);
        }
        r.publish(10); r.publish(11); r.publish(12);
        REQUIRE(gen_watch_read(r.mem, r.steps, B, &cur, 8, rows.tok.data(), nullptr, nullptr, &lost) == 3);
        REQUIRE(cur == 13 && lost == 0 && r.head() == 13);
        for (int i = 0; i < 3; ++i) REQUIRE(rows.tok[(size_t)i * B] == (unsigned)(10 + i) && rows.tok[(size_t)i * B + 2] == word(10 + (u64)i, 2, 0));
    }
    {   // ring_steps = 1: only the youngest record is ever there
        Ring r(1, B); Rows rows(4, B);
        u64 cur = 0, lost = 0;
        r.publish(0);
        REQUIRE(gen_watch_read(r.mem, 1, B, &cur, 4, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 1);
        REQUIRE(cur == 1 && lost == 0);
        require_row(rows, 0, B, 0);
        r.publish(1); r.publish(2); r.publish(3);
        REQUIRE(gen_watch_read(r.mem, 1, B, &cur, 4, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 1);
        REQUIRE(cur == 4 && lost == 2 && r.head() == 4);
        require_row(rows, 0, B, 3);
    }
    {   // a reader exactly ring_steps behind loses nothing
        Ring r(5, B); Rows rows(8, B);
        u64 cur = 0, lost = 0;
        for (u64 s = 0; s < 2; ++s) r.publish(s);
        REQUIRE(gen_watch_read(r.mem, 5, B, &cur, 8, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 2 && cur == 2);
        for (u64 s = 2; s < 7; ++s) r.publish(s);                   // head 7, cursor 2: ring_steps behind
        REQUIRE(gen_watch_read(r.mem, 5, B, &cur, 8, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 5);
        REQUIRE(cur == 7 && lost == 0 && r.head() == 7);
        for (int i = 0; i < 5; ++i) require_row(rows, i, B, 2 + (u64)i);
    }
    {   // ring_steps + 3 behind: lost = 3, and the oldest record still there is intact
        Ring r(5, B); Rows rows(8, B);
        u64 cur = 0, lost = 0;
        for (u64 s = 0; s < 8; ++s) r.publish(s);
        REQUIRE(gen_watch_read(r.mem, 5, B, &cur, 8, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 5);
        REQUIRE(cur == 8 && lost == 3 && r.head() == 8);
        for (int i = 0; i < 5; ++i) require_row(rows, i, B, 3 + (u64)i);
    }
    {   // max_steps smaller than what is available: the rest stays for the next call; the row behind the last one is not written
        Ring r(8, B); Rows rows(2, B);
        u64 cur = 0, lost = 0;
        for (u64 s = 0; s < 5; ++s) r.publish(s);
        rows.tok.back() = rows.prob.back() = 0xABCDEF01u; rows.fin.back() = -5;
        REQUIRE(gen_watch_read(r.mem, 8, B, &cur, 2, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 2 && cur == 2 && lost == 0);
        require_row(rows, 0, B, 0); require_row(rows, 1, B, 1);
        REQUIRE(rows.tok.back() == 0xABCDEF01u && rows.prob.back() == 0xABCDEF01u && rows.fin.back() == -5);
        REQUIRE(gen_watch_read(r.mem, 8, B, &cur, 2, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 2 && cur == 4 && lost == 0);
        require_row(rows, 0, B, 2); require_row(rows, 1, B, 3);
        REQUIRE(gen_watch_read(r.mem, 8, B, &cur, 0, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 0 && cur == 4);
        REQUIRE(gen_watch_read(r.mem, 8, B, &cur, 2, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost) == 1 && cur == 5 && lost == 0);
        require_row(rows, 0, B, 4);
        REQUIRE(r.head() == 5);
    }
    {   // the layout the ABI documents
        REQUIRE(gen_watch_rec_bytes(3) == 48 && gen_watch_rec_bytes(32) == 400 && gen_watch_rec_bytes(2) == 32);
        REQUIRE(gen_watch_bytes(4, 3) == 4 * 48 + 16 + 12);
    }
    std::printf("single ok\n");
}

// writer and reader threads over a ring of `steps`; returns through the counters.  The reader stops once the writer is done and the cursor
// has reached the head, or at the deadline.
static void two_threads(const char *name, int steps, u64 N) {
    const int B = 3, MAX = 37;
    Ring r(steps, B);
    std::atomic<bool> writer_done{false};
    u64 returned = 0, lost_total = 0, cur = 0, last_seq = 0;
    bool have_last = false, timed_out = false;
    std::thread writer([&] {
        for (u64 s = 0; s < N; ++s) r.publish(s);
        writer_done.store(true, std::memory_order_release);
    });
    std::thread reader([&] {
        Rows rows(MAX, B);
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(120);
        for (;;) {
            const bool done = writer_done.load(std::memory_order_acquire);   // looked at BEFORE the read
            u64 lost = 0;
            const int n = gen_watch_read(r.mem, steps, B, &cur, MAX, rows.tok.data(), rows.prob.data(), rows.fin.data(), &lost);
            lost_total += lost;
            for (int i = 0; i < n; ++i) {
                const u64 seq = rows.tok[(size_t)i * B];              // word (slot 0, field 0) is the sequence number
                REQUIRE(seq < N);
                REQUIRE(!have_last || seq > last_seq);                // strictly increasing
                require_row(rows, i, B, seq);                         // whole: every word is this record's
                last_seq = seq; have_last = true;
            }
            returned += (u64)n;
            if (done && n == 0 && cur >= N) break;
            if (std::chrono::steady_clock::now() > deadline) { timed_out = true; break; }
        }
    });
    writer.join();
    reader.join();
    REQUIRE(!timed_out);
    REQUIRE(cur == N && r.head() == N);
    REQUIRE(returned + lost_total == N);
    if ((u64)steps >= N) {                                          // no lap possible: everything arrives, in order
        REQUIRE(lost_total == 0 && returned == N && last_seq == N - 1);
    }
    std::printf("%s ok: ring_steps %d, records %llu, returned %llu, lost %llu\n", name, steps, N, returned, lost_total);
}

int main(int argc, char **argv) {
    const char *what = argc > 1 ? argv[1] : "all";
    const u64 N = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 100000ull;
    const bool all = !std::strcmp(what, "all");
    bool ran = false;
    if (all || !std::strcmp(what, "single")) { single(); ran = true; }
    if (all || !std::strcmp(what, "nolap")) { two_threads("nolap", (int)N, N); ran = true; }
    if (all || !std::strcmp(what, "lap")) { two_threads("lap", 8, N); ran = true; }
    if (!ran) { std::fprintf(stderr, "usage: gen_watch_test [single | nolap [N] | lap [N] | all]\n"); return 2; }
    return 0;
}

// gen_watch.h — the record ring of a WATCH (rwkv_gen_watch_*): what lets another thread see a running rwkv_gen_run and reach into it.
// The reference sends every token as it is drawn (run.rs:1009, `sender.send(Token::Content(word))`) and ends a request whose client is
// gone (run.rs:934-935, `context.sender.is_disconnected()`); in resident mode the host is not between the steps, so the step itself
// publishes one record into mapped, coherent host memory and reads one cancel word per slot from it.
// Host-only header (no HIP include, like gen_stop.h / gen_dfa.h / gen_pda.h): gen_publish_kernel (rwkv_kernels.hip) writes records with
// exactly these functions, rwkv_gen_watch_read (rwkv_engine.cpp) reads them with gen_watch_read, and tests/cpp/gen_watch_test.cpp compiles
// the same text with g++ and runs writer and reader on two threads under ThreadSanitizer.
//
// Memory, one pinned allocation:   ring_steps RECORDS | u64 head (padded to 16 bytes) | u32 cancel[B]
// A record, padded to 16 bytes:    u64 stamp | u32 tok[B] | f32 prob[B] (as bits) | i32 finish[B]
// Record s (the sequence number, from 0) lives in cell s % ring_steps; `head` is the number of records published.
//
// A sequence lock per record.  The WRITER of record s:  stamp <- 0; fence; payload; fence; stamp <- s + 1 (release); head <- s + 1
// (release).  The READER of s < head:  acquire-load the stamp, which must be s + 1; copy the payload; fence; reload the stamp, which must
// be unchanged — otherwise the writer has lapped the reader and the record is LOST, never returned torn.  Nobody waits for anybody.
// On the device the fences and atomics are system scope; on the host they are the __atomic builtins and every payload word is a relaxed
// 32-bit atomic, so the protocol is race-free in the C++ sense and ThreadSanitizer can hold it to that.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef RWKV_HD
#ifdef __HIP__
#define RWKV_HD __host__ __device__
#else
#define RWKV_HD
#endif
#endif

namespace rwkv {

constexpr int GEN_WATCH_MAX_STEPS = 65536;       // RWKV_GEN_WATCH_MAX_STEPS
constexpr int GEN_FIN_CANCELLED = 4;             // RWKV_GEN_CANCELLED, behind GEN_FIN_HANDBACK (gen_stop.h)
constexpr unsigned GEN_WATCH_NO_TOKEN = 0xFFFFFFFFu;   // a slot that emitted nothing in the step: the padding of rwkv_gen_run's outputs

RWKV_HD inline size_t gen_watch_rec_bytes(int B) { return ((size_t)8 + (size_t)12 * (size_t)B + 15) & ~(size_t)15; }
RWKV_HD inline size_t gen_watch_head_off(int ring_steps, int B) { return (size_t)ring_steps * gen_watch_rec_bytes(B); }
RWKV_HD inline size_t gen_watch_cancel_off(int ring_steps, int B) { return gen_watch_head_off(ring_steps, B) + 16; }
RWKV_HD inline size_t gen_watch_bytes(int ring_steps, int B) { return gen_watch_cancel_off(ring_steps, B) + (size_t)4 * (size_t)B; }

// ---- the memory operations of the protocol: system scope on the device, the __atomic builtins on the host ----
RWKV_HD inline void gen_watch_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
    __threadfence_system();
#else
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
#endif
}
RWKV_HD inline void gen_watch_store64(unsigned long long *p, unsigned long long v, bool release) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (release) __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
    if (release) __atomic_store_n(p, v, __ATOMIC_RELEASE);
    else __atomic_store_n(p, v, __ATOMIC_RELAXED);
#endif
}
RWKV_HD inline unsigned long long gen_watch_load64(const unsigned long long *p, bool acquire) {
#if defined(__HIP_DEVICE_COMPILE__)
    return acquire ? __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
    return acquire ? __atomic_load_n(p, __ATOMIC_ACQUIRE) : __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}
RWKV_HD inline void gen_watch_store32(unsigned *p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
    __atomic_store_n(p, v, __ATOMIC_RELAXED);
#endif
}
RWKV_HD inline unsigned gen_watch_load32(const unsigned *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

// ---- addresses ----
RWKV_HD inline unsigned char *gen_watch_rec(unsigned char *ring, int ring_steps, int B, unsigned long long seq) {
    return ring + (size_t)(seq % (unsigned long long)ring_steps) * gen_watch_rec_bytes(B);
}
RWKV_HD inline unsigned long long *gen_watch_head_ptr(unsigned char *ring, int ring_steps, int B) {
    return (unsigned long long *)(ring + gen_watch_head_off(ring_steps, B));
}
RWKV_HD inline unsigned *gen_watch_cancel_ptr(unsigned char *ring, int ring_steps, int B) {
    return (unsigned *)(ring + gen_watch_cancel_off(ring_steps, B));
}

// ---- the writer, in three parts so that the lanes of one block can share the payload (gen_publish_kernel: thread 0 opens, a barrier,
// thread b puts slot b and fences, a barrier, thread 0 commits); a single thread calls them back to back ----
RWKV_HD inline void gen_watch_open_rec(unsigned char *rec) {
    gen_watch_store64((unsigned long long *)rec, 0ull, false);
    gen_watch_fence();
}
RWKV_HD inline void gen_watch_put(unsigned char *rec, int B, int b, unsigned tok, unsigned prob_bits, int finish) {
    unsigned *w = (unsigned *)(rec + 8);
    gen_watch_store32(w + b, tok);
    gen_watch_store32(w + B + b, prob_bits);
    gen_watch_store32(w + 2 * B + b, (unsigned)finish);
}
RWKV_HD inline void gen_watch_commit(unsigned char *rec, unsigned long long *head, unsigned long long seq) {
    gen_watch_fence();
    gen_watch_store64((unsigned long long *)rec, seq + 1, true);
    gen_watch_store64(head, seq + 1, true);
}

RWKV_HD inline unsigned long long gen_watch_head(const unsigned char *ring, int ring_steps, int B) {
    return gen_watch_load64((const unsigned long long *)(ring + gen_watch_head_off(ring_steps, B)), true);
}

// ---- the reader: record `seq` into tokens / probs / finish ([B] each; probs and finish may be null).  False: the record is lost (it is
// being, or has been, overwritten); whatever was copied is garbage and the caller must not hand it on ----
RWKV_HD inline bool gen_watch_read_one(const unsigned char *ring, int ring_steps, int B, unsigned long long seq, unsigned *tokens, unsigned *probs,
                                       int *finish) {
    const unsigned char *rec = ring + (size_t)(seq % (unsigned long long)ring_steps) * gen_watch_rec_bytes(B);
    const unsigned long long *stamp = (const unsigned long long *)rec;
    if (gen_watch_load64(stamp, true) != seq + 1) return false;
    const unsigned *w = (const unsigned *)(rec + 8);
    for (int b = 0; b < B; ++b) tokens[b] = gen_watch_load32(w + b);
    if (probs) for (int b = 0; b < B; ++b) probs[b] = gen_watch_load32(w + B + b);
    if (finish) for (int b = 0; b < B; ++b) finish[b] = (int)gen_watch_load32(w + 2 * B + b);
    gen_watch_fence();
    return gen_watch_load64(stamp, false) == seq + 1;
}

// rwkv_gen_watch_read: the records *cursor .. into rows of B words each, at most max_steps of them; *cursor moves behind the last record
// looked at, *lost counts the records skipped (overwritten before they could be copied).  A reader more than ring_steps behind jumps to
// the oldest record the ring can still hold.  Returns the number of rows written.  Never waits: what is not published yet is not there.
RWKV_HD inline int gen_watch_read(const unsigned char *ring, int ring_steps, int B, unsigned long long *cursor, int max_steps, unsigned *tokens,
                                  unsigned *probs, int *finish, unsigned long long *lost) {
    unsigned long long c = *cursor, skipped = 0;
    unsigned long long head = gen_watch_head(ring, ring_steps, B);
    int n = 0;
    while (n < max_steps && c < head) {
        if (head - c > (unsigned long long)ring_steps) {           // lapped: cell c % ring_steps holds a younger record by now
            skipped += head - (unsigned long long)ring_steps - c;
            c = head - (unsigned long long)ring_steps;
        }
        const size_t at = (size_t)n * (size_t)B;
        if (gen_watch_read_one(ring, ring_steps, B, c, tokens + at, probs ? probs + at : nullptr, finish ? finish + at : nullptr)) ++n;
        else {                                                     // the writer went past while we looked: see how far it is now
            ++skipped;
            head = gen_watch_head(ring, ring_steps, B);
        }
        ++c;
    }
    *cursor = c;
    *lost = skipped;
    return n;
}

}  // namespace rwkv

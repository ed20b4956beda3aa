// gen_host.h — what a resident-generation step is made of, as the host names it: the sampler kernels its rows need, the optional kernels
// that join it, and the key under which its captured graph is kept.  Host-only (no HIP include; tests/test_gen_key_cpu.py compiles it with g++).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace rwkv {

// which sampler kernels a set of rows needs, as bits (the low bits of a generation graph's flag word)
enum : unsigned { NEEDS_NT = 1, NEEDS_MIRO = 2, NEEDS_WIDE = 4 };   // nucleus / typical, mirostat, rows of sample_wide_kernel (any kind)
// the features of a step: each one adds a launch to it, or selects a kernel variant (the high bits of the flag word)
enum : uint64_t {
    FEAT_STOPS = 1ull << 32,        // a slot of the row set has stop strings: gen_post_kernel<., true>
    FEAT_DFA = 1ull << 33,          // ... a byte automaton: gen_mask_kernel joins the step
    FEAT_TOPN = 1ull << 34,         // ... lists: gen_topn_kernel joins the step
    FEAT_PDA = 1ull << 35,          // ... a stack automaton: gen_pda_mask_kernel joins the step
    FEAT_WATCH = 1ull << 36,        // a watch is open: gen_publish joins the step
    FEAT_CAPTURE = 1ull << 37,      // a slot keeps its rows for an item: gen_capture_kernel joins the step
};
// the key of a decode-only step: the slot mask in (max_batch + 63) / 64 words, then the flag word
inline std::vector<uint64_t> gen_step_key(int max_batch, const std::vector<int> &slots, unsigned needs, uint64_t feats) {
    std::vector<uint64_t> key((size_t)(max_batch + 63) / 64 + 1, 0);
    for (int b : slots) key[(size_t)b / 64] |= 1ull << (b % 64);
    key.back() = needs | feats;
    return key;
}

}  // namespace rwkv

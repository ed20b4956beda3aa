// rwkv_dfa.h — the `rwkv_dfa` handle of include/rwkv_abi.h as the engine sees it.  Host only; rwkv_dfa.cpp defines the ABI functions
// (plain C++, no HIP: tests/cpp/fuzz_dfa.cpp compiles it with g++ and sanitizers).
#pragma once
#include <cstdint>
#include <vector>

#include "gen_dfa.h"

struct rwkv_dfa {                        // immutable once built
    int n_states = 0, start = 0;
    std::vector<uint16_t> trans;         // [n_states][256]
    std::vector<uint8_t> accepting;      // [n_states] as handed in (0 / 1)
    std::vector<uint8_t> flags;          // [n_states] GEN_DFA_ACCEPT | GEN_DFA_END (gen_dfa_flags)
};

namespace rwkv {
// The liveness rule of rwkv_gen_set_constraint: every live state reachable from `state` over bytes in which a slot can come to rest (the
// state itself, and every state that does not halt under `mode`) has a single-byte token (single[c] != 0) that leads to a live state.
// This is what guarantees that a masked row is never all -inf.  O(states x 256).
bool dfa_never_stuck(const rwkv_dfa &d, int state, int mode, const uint8_t single[256]);
}  // namespace rwkv

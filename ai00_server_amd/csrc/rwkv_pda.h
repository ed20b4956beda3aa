// rwkv_pda.h — the `rwkv_pda` handle of include/rwkv_abi.h as the engine sees it.  Host only; rwkv_pda.cpp defines the ABI functions
// (plain C++, no HIP: tests/cpp/fuzz_pda.cpp compiles it with g++ and sanitizers).
#pragma once
#include <cstdint>
#include <vector>

#include "gen_pda.h"

struct rwkv_pda {                        // immutable once built
    int n_states = 0, start = 0, max_depth = 0;
    std::vector<uint16_t> next, act;     // [n_states][256] each
    std::vector<uint8_t> accepting;      // [n_states] as handed in (0 / 1)
    std::vector<uint8_t> flags;          // [n_states] GEN_PDA_ACCEPT | GEN_PDA_END (gen_pda_flags)
};

namespace rwkv {
// The LIVENESS rule of rwkv_gen_set_pda, conservative and static, O(states x 256).  From the configuration (state, stack[0 .. depth)) every
// state that any sequence of transitions could enter is collected — a plain or push target, and every return state a collected state pushes —
// together with one bit: whether it can only ever be entered WITH AN EMPTY STACK (a plain target of such a state, or the return state such a
// state pushed).  Every collected state must then have a single-byte token (single[c] != 0) with a PLAIN live transition: a plain
// transition works at every depth, max_depth included, where every push is dead, and with an empty stack, where every pop is.  A state
// that is only ever entered with an empty stack may use a PUSH instead (max_depth >= 1: it cannot fail there).  The only exempt state is one
// that is ACCEPT and END and only ever entered with an empty stack — entering it halts in both modes — and never the configuration's own state,
// whose row is masked before anything halts.
bool pda_never_stuck(const rwkv_pda &p, int state, const uint16_t *stack, int depth, const uint8_t single[256]);
}  // namespace rwkv

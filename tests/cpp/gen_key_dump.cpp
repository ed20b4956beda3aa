// CPU driver of ai00_server_amd/csrc/gen_host.h for tests/test_gen_key_cpu.py: the key gen_decode_steps keeps a captured step under.
// Reads lines of "<max_batch> <needs> <features> <slot> ..." from stdin and prints one line per key: its 64-bit words in hex, separated by
// blanks.  max_batch and the slots (ascending) are decimal; needs and features are a hex number, or the header's own names joined by `+`
// (nt, miro, wide; stops, dfa, topn, pda, watch, capture), so that a caller can ask for a bit without knowing where it lies.
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../ai00_server_amd/csrc/gen_host.h"

static const std::map<std::string, uint64_t> kNames = {
    {"nt", rwkv::NEEDS_NT}, {"miro", rwkv::NEEDS_MIRO}, {"wide", rwkv::NEEDS_WIDE},
    {"stops", rwkv::FEAT_STOPS}, {"dfa", rwkv::FEAT_DFA}, {"topn", rwkv::FEAT_TOPN}, {"pda", rwkv::FEAT_PDA}, {"watch", rwkv::FEAT_WATCH}, {"capture", rwkv::FEAT_CAPTURE},
};

static uint64_t word(const std::string &s) {
    if (s[0] >= '0' && s[0] <= '9') return std::stoull(s, nullptr, 16);
    uint64_t w = 0;
    std::istringstream names(s);
    for (std::string name; std::getline(names, name, '+');) w |= kNames.at(name);
    return w;
}

int main() {
    std::string line;
    for (int n = 0; std::getline(std::cin, line); ++n) {
        std::istringstream ws(line);
        int max_batch = 0;
        std::string needs, feats;
        if (!(ws >> max_batch >> needs >> feats) || max_batch < 1) { std::fprintf(stderr, "line %d: want <max_batch> <needs> <features> <slot> ...\n", n); return 2; }
        std::vector<int> slots;
        for (int b; ws >> b;) {
            if (b < 0 || b >= max_batch) { std::fprintf(stderr, "line %d: slot %d outside 0 .. %d\n", n, b, max_batch - 1); return 2; }
            slots.push_back(b);
        }
        std::vector<uint64_t> key;
        try { key = rwkv::gen_step_key(max_batch, slots, (unsigned)word(needs), word(feats)); }
        catch (const std::exception &) { std::fprintf(stderr, "line %d: unknown name or number in `%s %s`\n", n, needs.c_str(), feats.c_str()); return 2; }
        for (size_t i = 0; i < key.size(); ++i) std::printf("%s%llx", i ? " " : "", (unsigned long long)key[i]);
        std::printf("\n");
    }
    return 0;
}

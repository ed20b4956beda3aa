// CPU driver of ai00_server_amd/csrc/graph_cache.h for tests/test_gen_churn_cpu.py: a list of generation keys through the cache as
// gen_decode_steps puts them through it with a run of more than one step — find; on a miss should_capture (false: the first step runs
// directly) and then insert, whatever should_capture said (the steps behind the first go through the captured graph).
// usage: graph_cache_replay <capacity> <key file>; the file holds one key per line, its 64-bit words in hex separated by blanks.
// Prints one line per visit: "<visit> <r|d|c> <evicted handle or -1> <inserts so far>" — r: replayed from the cache; d: first step direct,
// then captured; c: known but not cached, captured at once.  A handle is the visit that inserted it.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../ai00_server_amd/csrc/graph_cache.h"

struct Recorder {
    std::vector<int> *log;
    void operator()(int h) const { log->push_back(h); }
};

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: graph_cache_replay <capacity> <key file>\n"); return 2; }
    std::ifstream in(argv[2]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::vector<int> log;
    long inserts = 0;
    {
        rwkv::GraphCache<std::vector<uint64_t>, int, Recorder> cache((size_t)std::stoul(argv[1]), Recorder{&log});
        std::string line;
        for (int visit = 0; std::getline(in, line); ++visit) {
            std::vector<uint64_t> key;
            std::istringstream ws(line);
            for (std::string w; ws >> w;) key.push_back(std::stoull(w, nullptr, 16));
            if (key.empty()) { std::fprintf(stderr, "line %d holds no key\n", visit); return 2; }
            const size_t before = log.size();
            char what = 'r';
            if (!cache.find(key)) {
                what = cache.should_capture(key) ? 'c' : 'd';
                cache.insert(key, visit);
                ++inserts;
            }
            std::printf("%d %c %d %ld\n", visit, what, log.size() > before ? log.back() : -1, inserts);
        }
    }
    std::printf("deleted %zu\n", log.size());                      // evictions and teardown together: every handle exactly once
    return 0;
}

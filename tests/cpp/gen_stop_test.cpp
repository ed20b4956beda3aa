// CPU driver of the stop-string matcher (no GPU, no HIP): reads scripted cases, runs every token through
//   k  the functions of ai00_server_amd/csrc/gen_stop.h in the order gen_post_kernel<., true> calls them — append into a staging copy of the
//      slot's buffer, one scan per "lane", the order-keeping butterfly over 8 lanes, decide, validate, trim — with the device's bounded buffer;
//   c  rwkv::StopMatcher (include/rwkv_scheduler.hpp) with the same bound
// and prints one line per token and side: `<k|c> <finish> <head or content, hex> <buffer afterwards, hex>` ("-" = empty).
// tests/test_gen_stop_cpu.py compares both with a literal transcription of run.rs.  Stand-alone on purpose: this is the program a
// sanitizer build (-fsanitize=address,undefined) runs.
//
// Input, one item per line:  case | stop <hex> | tail <hex> | max <n> | emitted <n> | tok <hex|-|?> <0|1>     ("?": unknown id; 1: a stop token)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../ai00_server_amd/csrc/gen_stop.h"
#include "../../include/rwkv_scheduler.hpp"

namespace {
using Bytes = std::vector<uint8_t>;

Bytes unhex(const std::string &h) {
    Bytes b;
    if (h == "-") return b;
    for (size_t i = 0; i + 1 < h.size(); i += 2) b.push_back((uint8_t)std::stoi(h.substr(i, 2), nullptr, 16));
    return b;
}
std::string hex(const uint8_t *p, size_t n) {
    if (!n) return "-";
    static const char *d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}

struct Device {                                                    // what a GenSlot / GenStop pair holds of this
    std::vector<Bytes> stops;
    unsigned char buf[rwkv::GEN_STOP_BUF];
    int buf_len = 0, emitted = 0, max_tokens = 1 << 30, finish = 0;

    void step(const Bytes &word, bool known, bool stop_token) {
        using namespace rwkv;
        unsigned char lds[GEN_STOP_BUF];
        const int wlen = known ? (int)word.size() : 0;
        const bool fits = buf_len + wlen <= GEN_STOP_BUF;
        const int n = fits ? buf_len + wlen : buf_len;
        std::memcpy(lds, buf, (size_t)buf_len);
        if (fits && wlen) std::memcpy(lds + buf_len, word.data(), (size_t)wlen);
        GenStopScan r[8];
        for (int lane = 0; lane < 8; ++lane)
            r[lane] = lane < (int)stops.size() ? gen_stop_scan(lds, n, stops[(size_t)lane].data(), (int)stops[(size_t)lane].size()) : GEN_STOP_NONE;
        const int partner[3][8] = {{1, 0, 3, 2, 5, 4, 7, 6}, {2, 3, 0, 1, 6, 7, 4, 5}, {7, 6, 5, 4, 3, 2, 1, 0}};   // quad_perm, quad_perm, row_half_mirror
        for (int s = 0; s < 3; ++s) {
            GenStopScan o[8];
            for (int lane = 0; lane < 8; ++lane) o[lane] = r[partner[s][lane]];
            for (int lane = 0; lane < 8; ++lane) r[lane] = (lane & (1 << s)) ? gen_stop_merge(o[lane], r[lane]) : gen_stop_merge(r[lane], o[lane]);
        }
        for (int lane = 1; lane < 8; ++lane)
            if (r[lane].safe != r[0].safe || r[lane].matched != r[0].matched) { std::printf("lanes disagree\n"); std::exit(3); }
        emitted += 1;
        finish = gen_stop_decide(stop_token || !known, fits, r[0].matched != 0, emitted >= max_tokens);
        const int safe = stops.empty() ? n : r[0].safe;            // (the kernel never runs this path for a slot without strings)
        std::string head = hex(lds, (size_t)safe);
        if (!finish) {
            const int keep = gen_stop_keep_from(lds, safe);
            if (keep == 0) head = "-";
            std::memmove(buf, lds + keep, (size_t)(n - keep));
            buf_len = n - keep;
        }
        std::printf("k %d %s %s\n", finish, finish == GEN_FIN_STOP || !finish ? head.c_str() : "-", hex(buf, (size_t)buf_len).c_str());
    }
};
}  // namespace

int main() {
    std::vector<std::string> stops;
    Bytes tail;
    int max_tokens = 1 << 30, emitted = 0;
    Device dev;
    rwkv::StopMatcher *m = nullptr;
    bool started = false, done = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, a;
        in >> op;
        if (op == "case") {
            delete m; m = nullptr;
            stops.clear(); tail.clear(); max_tokens = 1 << 30; emitted = 0; started = done = false;
            std::printf("case\n");
        } else if (op == "stop") { in >> a; const Bytes b = unhex(a); stops.emplace_back(b.begin(), b.end()); }
        else if (op == "tail") { in >> a; tail = unhex(a); }
        else if (op == "max") in >> max_tokens;
        else if (op == "emitted") in >> emitted;
        else if (op == "tok") {
            int st = 0;
            in >> a >> st;
            if (done) continue;
            if (!started) {
                if (stops.size() > (size_t)rwkv::GEN_MAX_STOP_STR || tail.size() > (size_t)rwkv::GEN_STOP_BUF) { std::printf("limits\n"); return 2; }
                dev = Device();
                for (const std::string &s : stops) dev.stops.emplace_back(s.begin(), s.end());
                if (!tail.empty()) std::memcpy(dev.buf, tail.data(), tail.size());
                dev.buf_len = (int)tail.size(); dev.max_tokens = max_tokens; dev.emitted = emitted;
                m = new rwkv::StopMatcher(stops, tail, (size_t)rwkv::GEN_STOP_BUF);
                started = true;
            }
            const bool known = a != "?";
            const Bytes word = known ? unhex(a) : Bytes();
            dev.step(word, known, st != 0);
            emitted += 1;
            const rwkv::StopMatcher::Step s = m->advance(known ? &word : nullptr, st != 0, emitted >= max_tokens);
            std::printf("c %d %s %s\n", s.finish, hex(s.content.data(), s.content.size()).c_str(), hex(m->tail().data(), m->tail().size()).c_str());
            done = dev.finish != 0;
        }
    }
    delete m;
    std::printf("gen_stop_test: ok\n");
    return 0;
}

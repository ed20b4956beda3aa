// probe_case_test.cpp — the container parser of the kernel probes (probe_case.h, and nothing else) as a stand-alone host program, built under
// -fsanitize=address,undefined by tests/test_probe_io_cpu.py.
//
//   probe_case_test <cases.bin> <program> <magic> <kinds> <max_params> <roles> <small_esize>
//
// One JSON line per case: name, kind, params, and per buffer [role, esize, flags, nbytes, off, CRC-32 of the host image after the pattern fill].
#include "probe_case.h"

static uint32_t crc32(const std::vector<uint8_t> &v) {
    static uint32_t table[256];
    if (!table[1])
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
    uint32_t c = 0xFFFFFFFFu;
    for (uint8_t b : v) c = table[(c ^ b) & 0xFF] ^ (c >> 8);
    return ~c;
}

int main(int argc, char **argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: probe_case_test <cases.bin> <program> <magic> <kinds> <max_params> <roles> <small_esize>\n"); return 2; }
    const ProbeSpec spec{argv[2], (int32_t)std::strtol(argv[3], nullptr, 0), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7])};
    for (const Case &c : read_case_file(argv[1], spec)) {
        std::printf("{\"name\": \"%s\", \"kind\": %d, \"params\": [", c.name.c_str(), c.kind);
        for (size_t i = 0; i < c.p.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)c.p[i]);
        std::printf("], \"bufs\": [");
        for (size_t i = 0; i < c.b.size(); ++i) {
            const Buf &x = c.b[i];
            std::printf("%s[%d, %d, %d, %lld, %lld, %u]", i ? ", " : "", x.role, x.esize, x.flags, (long long)x.nbytes, (long long)x.off, crc32(x.host));
        }
        std::printf("]}\n");
    }
    return 0;
}

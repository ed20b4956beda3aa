// probe_case.h — the case-file container of the role-buffer probes (row_probe, mix_probe, sample_probe): plain C++17, nothing of HIP and
// nothing of any kernel (DESIGN.md "Probe container" states the format and the order of work).  tests/probe_io.py writes the same format;
// tests/cpp/probe_case_test.cpp reads it under a sanitizer.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

constexpr uint32_t SENT32 = 0x7FC0DEADu;                              // a NaN as a float, an impossible token as an int
constexpr uint16_t SENT16 = 0x7EADu;                                  // a NaN as an f16
constexpr uint8_t SENT8 = 0xADu;

inline const char *probe_program = "probe";                           // the `<program>: ` of every message; read_case_file sets it from the spec

struct ProbeSpec {
    const char *program;
    int32_t magic;
    int kinds, max_params, roles;                                     // K_COUNT, the limit of a case's parameter count, R_COUNT
    int small_esize;                                                  // buffers hold 4-byte elements or these: 2 (f16) or 1 (bytes)
};

struct Buf {
    int role = 0, esize = 0, flags = 0;
    int64_t nbytes = 0, off = 0;
    std::vector<uint8_t> host;
    void *dev = nullptr;
};
// A probe that keeps more per case (mix_probe: its plans and tiled weights) derives from this.
struct Case {
    std::string name;
    int kind = 0;
    std::vector<int64_t> p;
    std::vector<Buf> b;
    const Buf *find(int role) const {
        for (const Buf &x : b) if (x.role == role) return &x;
        return nullptr;
    }
    template <class T> T *ptr(int role) const { const Buf *x = find(role); return x ? (T *)((char *)x->dev + x->off) : nullptr; }
    template <class T> const T *host(int role) const { const Buf *x = find(role); return x ? (const T *)(x->host.data() + x->off) : nullptr; }
};

[[noreturn]] inline void bad_file(const char *what) {
    std::fprintf(stderr, "%s: %s\n", probe_program, what);
    std::exit(2);
}
struct Reader {
    FILE *f;
    void get(void *dst, size_t bytes) {
        if (bytes && std::fread(dst, 1, bytes, f) != bytes) bad_file("case file ends early");
    }
    int32_t i32() { int32_t v; get(&v, 4); return v; }
    int64_t i64() { int64_t v; get(&v, 8); return v; }
};

[[noreturn]] inline void refuse(const Case &c, const std::string &why) {
    std::fprintf(stderr, "%s: case %s refused before any launch: %s\n", probe_program, c.name.c_str(), why.c_str());
    std::exit(4);
}
#define REQUIRE(c, cond) do { if (!(cond)) refuse(c, #cond); } while (0)

// `n` elements of `esize` bytes are reachable from the pointer of `role` (which must exist unless optional), with `guard` elements before and behind them
inline void need(const Case &c, int role, int64_t n, int esize, bool optional = false, int64_t guard = 0) {
    const Buf *x = c.find(role);
    if (!x) { if (optional) return; refuse(c, "missing buffer, role " + std::to_string(role)); }
    if (x->esize != esize || n < 0 || x->off < guard * esize || x->off + (n + guard) * esize > x->nbytes)
        refuse(c, "buffer of role " + std::to_string(role) + " is too small for " + std::to_string(n) + " elements" + (guard ? " between guard bands" : ""));
}
inline int64_t ceil16(int64_t t) { return (t + 15) / 16 * 16; }

// The whole case file, every header checked, the pattern filled into every buffer with flags & 2.  Ends the process with status 2 on any error.
template <class C = Case> std::vector<C> read_case_file(const char *path, const ProbeSpec &spec) {
    probe_program = spec.program;
    FILE *fi = std::fopen(path, "rb");
    if (!fi) { std::fprintf(stderr, "%s: cannot read %s\n", probe_program, path); std::exit(2); }
    Reader rd{fi};
    if (rd.i32() != spec.magic) bad_file("bad magic");
    const int ncases = rd.i32();
    if (ncases < 0 || ncases > 4096) bad_file("bad case count");
    std::vector<C> cases(ncases);
    for (C &c : cases) {
        const int nl = rd.i32();
        if (nl < 0 || nl > 256) bad_file("bad name length");
        c.name.resize(nl); rd.get(&c.name[0], nl);
        c.kind = rd.i32();
        const int np = rd.i32();
        if (c.kind < 0 || c.kind >= spec.kinds || np < 0 || np > spec.max_params) bad_file("bad case header");
        c.p.resize(np); rd.get(c.p.data(), (size_t)np * 8);
        const int nb = rd.i32();
        if (nb < 0 || nb > spec.roles) bad_file("bad buffer count");
        c.b.resize(nb);
        for (Buf &x : c.b) {
            x.role = rd.i32(); x.esize = rd.i32(); x.flags = rd.i32(); x.nbytes = rd.i64(); x.off = rd.i64();
            if (x.nbytes <= 0 || x.nbytes >= (int64_t)1 << 31 || (x.esize != spec.small_esize && x.esize != 4) || x.nbytes % x.esize) bad_file("bad buffer header");
            x.host.resize(x.nbytes);
            if (!(x.flags & 2)) rd.get(x.host.data(), x.nbytes);
            else if (x.esize == 4) for (int64_t i = 0; i < x.nbytes / 4; ++i) ((uint32_t *)x.host.data())[i] = SENT32;
            else if (x.esize == 2) for (int64_t i = 0; i < x.nbytes / 2; ++i) ((uint16_t *)x.host.data())[i] = SENT16;
            else std::memset(x.host.data(), SENT8, x.nbytes);
        }
    }
    std::fclose(fi);
    return cases;
}

// gemm_probe.hip — stand-alone driver of the GEMM kernels for tests/test_gpu_gemm_exact.py (DESIGN.md "GEMM probe").  Not part of
// librwkv_hip.so: it links the kernel objects the build leaves in ai00_server_amd/csrc and calls the engine's own planner and launchers
// (shape_of, plan_gemm / plan_decode / tile_geometry, fill_prob, launch_smallk / launch_gemm_tile / launch_gemm) on ONE launch per case.
//
//   gemm_probe <cases.bin> <results.bin>        one JSON line per case on stdout: the plan that ran, or "unsupported" with the reason
//
// cases.bin (little-endian; i32 = int32, f16 = raw half bits, f32 = float), tests/gemm_cases.py write_cases:
//   i32 magic 'GPRB', i32 ncases, then per case
//     i32[14] T hilo mode force_spb tile_shape ksplit xcd_map nprob ldx ldo ldh ldm nslab single
//             mode: -1 plan_gemm decides (tile_shape / xcd_map >= 0 go into its Knobs), 2: plan_decode(force_spb), 1: tile_geometry(tile_shape, ksplit)
//             single = 1: the case is one bare 16x16x32 MFMA on its first problem's operands (no kernel of the engine runs)
//     f16 xhi[ceil16(T) * ldx]  (+ f16 xlo[...] when hilo), already in B-fragment order (opd_off); rows T.. hold the caller's sentinel
//     f32 m0[T * ldm], f32 m1[T * ldm]  when ldm > 0
//     per problem  i32[12] rows K fmt xoff act post partial has_bias mcol ocol hcol has_lo   (ocol / hcol < 0: no fp32 / no operand output)
//                  f16 W[rows * K] raw row-major,  f32 bias[rows] when has_bias
// results.bin: per case  i32 status (0 ran, 1 unsupported: nothing more follows), then every buffer WHOLE, guard band included:
//     f32 out[nslab * T * ldo + GUARD] when ldo > 0;  f16 ohi[ceil16(T) * ldh + GUARD], f16 olo[...] when ldh > 0
//     per problem: the tiled payload bytes, then the scale bytes (quantised formats) the load-time kernel wrote
// Output buffers hold a NaN bit pattern before the launch (0x7FC0DEAD / 0x7EAD): what the launch does not own must still hold it afterwards.
// Every case is validated BEFORE anything is launched (bounds of every index the kernels form); every HIP call is checked and the first
// error ends the process with a non-zero status.
#include "gemm_probe_plan.h"
#include "probe_common.h"                                  // HIP_OK, Reader and the patterns; the file format above is this probe's own

using namespace rwkv;

constexpr int GUARD = 256;                                 // elements after every output buffer

__global__ void single_mfma_kernel(const _Float16 *a, const _Float16 *b, float *out) {      // a, b: one fragment tile each (lane l: 8 halfs at 8 l)
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*(const h8 *)(a + lane * 8), *(const h8 *)(b + lane * 8), acc, 0, 0, 0);
    for (int r = 0; r < 4; ++r) out[(lane & 15) * 16 + (lane >> 4) * 4 + r] = acc[r];        // out[t][row]
}

struct Prob {
    int rows, K, fmt, xoff, act, post, partial, has_bias, mcol, ocol, hcol, has_lo;
    std::vector<uint16_t> W;
    std::vector<float> bias;
};

static size_t payload_bytes(int fmt, int rows, int K) { return fmt == W_F16 ? (size_t)rows * K * 2 : fmt == W_INT8 ? (size_t)rows * K : (size_t)rows * K / 2; }
static size_t scale_bytes(int fmt, int rows, int K) { return fmt == W_F16 ? 0 : fmt == W_INT8 ? (size_t)rows * (K / 128) * 4 : (size_t)rows * (K / 64) * 2; }

template <class T> static T *dalloc(size_t n, std::vector<void *> &bufs) {
    void *p = nullptr;
    HIP_OK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
    bufs.push_back(p);
    return (T *)p;
}
template <class T> static T *dsent(size_t n, T pattern, std::vector<void *> &bufs) {
    T *p = dalloc<T>(n, bufs);
    std::vector<T> h(n, pattern);
    if (n) HIP_OK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
    return p;
}
template <class T> static T *dcopy(const std::vector<T> &h, std::vector<void *> &bufs) {
    T *p = dalloc<T>(h.size(), bufs);
    if (!h.empty()) HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
}
template <class T> static void put(FILE *f, const T *dev, size_t n) {
    std::vector<T> h(n);
    if (n) HIP_OK(hipMemcpy(h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost));
    if (n && std::fwrite(h.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "gemm_probe: cannot write the results\n"); std::exit(2); }
}

int main(int argc, char **argv) {
    probe_program = "gemm_probe";
    if (argc != 3) { std::fprintf(stderr, "usage: gemm_probe cases.bin results.bin\n"); return 2; }
    FILE *fin = std::fopen(argv[1], "rb"), *fout = std::fopen(argv[2], "wb");
    if (!fin || !fout) { std::fprintf(stderr, "gemm_probe: cannot open the files\n"); return 2; }
    Reader rd{fin};
    int head[2];
    rd.get(head, sizeof(head));
    if (head[0] != 0x42525047) { std::fprintf(stderr, "gemm_probe: not a case file\n"); return 2; }
    hipStream_t st;
    HIP_OK(hipStreamCreate(&st));
    for (int ci = 0; ci < head[1]; ++ci) {
        int c[14];
        rd.get(c, sizeof(c));
        const int T = c[0], mode = c[2], force_spb = c[3], tile_shape = c[4], ksplit_in = c[5], xcd = c[6], n = c[7];
        const int ldx = c[8], ldo = c[9], ldh = c[10], ldm = c[11], nslab = c[12], single = c[13];
        const bool hilo = c[1] != 0;
        if (T < 1 || T > 4096 || n < 1 || n > GEMM_MAXP || ldx < 32 || ldx % 32 || ldx > 65536 || ldo < 0 || ldh < 0 || ldm < 0 || nslab < 1 || nslab > 16) {
            std::fprintf(stderr, "gemm_probe: case %d: bad header\n", ci);
            return 2;
        }
        const int T16 = (T + 15) / 16 * 16;
        std::vector<uint16_t> xhi((size_t)T16 * ldx), xlo(hilo ? xhi.size() : 0);
        rd.get(xhi.data(), xhi.size() * 2);
        rd.get(xlo.data(), xlo.size() * 2);
        std::vector<float> m0((size_t)T * ldm), m1((size_t)T * ldm);
        rd.get(m0.data(), m0.size() * 4);
        rd.get(m1.data(), m1.size() * 4);
        std::vector<Prob> pr(n);
        for (Prob &p : pr) {
            rd.get(&p.rows, 12 * sizeof(int));
            if (p.rows < 1 || p.K < 1 || (long)p.rows * p.K > (64L << 20)) { std::fprintf(stderr, "gemm_probe: case %d: bad problem\n", ci); return 2; }
            p.W.resize((size_t)p.rows * p.K);
            rd.get(p.W.data(), p.W.size() * 2);
            p.bias.resize(p.has_bias ? p.rows : 0);
            rd.get(p.bias.data(), p.bias.size() * 4);
        }
        // ---- validation: every index a kernel forms from these fields stays inside the buffers allocated below ----
        std::string why;
        auto need = [&](bool ok, const char *what) { if (!ok && why.empty()) why = what; };
        for (const Prob &p : pr) {
            need(p.rows % 16 == 0, "rows % 16");
            need(p.fmt == W_F16 || p.fmt == W_INT8 || p.fmt == W_NF4, "fmt");
            need(p.K % (p.fmt == W_F16 ? 32 : 256) == 0, "K alignment of the format");
            need(p.xoff >= 0 && p.xoff % 32 == 0 && p.xoff + p.K <= ldx, "xoff + K inside ldx");
            need(p.act >= ACT_NONE && p.act <= ACT_DECAY7 && p.post >= POST_NONE && p.post <= POST_MIX, "epilogue");
            need(p.post == POST_NONE || (ldm > 0 && p.mcol >= 0 && p.mcol % 4 == 0 && p.mcol + p.rows <= ldm), "m0 / m1 columns inside ldm");
            need(p.ocol >= 0 || p.hcol >= 0, "no output");
            need(p.ocol < 0 || (p.ocol % 4 == 0 && p.ocol + p.rows <= ldo), "fp32 columns inside ldo");
            need(p.hcol < 0 || (p.hcol % 32 == 0 && p.hcol + p.rows <= ldh && ldh % 32 == 0), "operand columns inside ldh");
            need(!p.partial || (p.ocol >= 0 && p.hcol < 0 && p.act == ACT_NONE && p.post != POST_MIX && !p.has_bias), "a partial problem has a linear epilogue");
        }
        need(ldo % 4 == 0, "ldo % 4");
        if (single) need(n == 1 && T == 16 && pr[0].rows == 16 && pr[0].K == 32 && pr[0].fmt == W_F16 && pr[0].ocol == 0 && ldo == 16 && nslab == 1 && !hilo, "single-MFMA case");

        std::vector<void *> bufs;
        std::vector<DMat> mats(n);
        std::vector<ProbSpec> ps(n);
        ProbShape sh[GEMM_MAXP];
        // shapes first: the planner looks at nothing else (shape_of only tests the pointers for null; the real ones are filled in below)
        static float dummy_f;
        static _Float16 dummy_h;
        for (int i = 0; i < n; ++i) {
            mats[i].fmt = pr[i].fmt; mats[i].rows = pr[i].rows; mats[i].K = pr[i].K;
            ps[i].W = &mats[i]; ps[i].xoff = pr[i].xoff; ps[i].act = pr[i].act; ps[i].post = pr[i].post; ps[i].partial = pr[i].partial != 0;
            ps[i].bias = pr[i].has_bias ? &dummy_f : nullptr;
            ps[i].out = pr[i].ocol >= 0 ? &dummy_f : nullptr;
            ps[i].oh.hi = pr[i].hcol >= 0 ? &dummy_h : nullptr;
            sh[i] = shape_of(ps[i]);
        }
        const ProbeReq req{T, hilo ? 1 : 0, mode, force_spb, tile_shape, ksplit_in, xcd, n, nslab};
        ProbePlan plan;
        plan.why = why;
        if (why.empty()) probe_plan(req, sh, plan);
        if (!plan.why.empty()) {
            const int status = 1;
            std::fwrite(&status, 4, 1, fout);
            probe_print(stdout, ci, req, plan);
            std::fflush(stdout);
            continue;
        }
        GemmLaunch &Lh = plan.Lh;
        const GemmPlan pl = plan.pl;
        // ---- buffers ----
        _Float16 *d_xhi = (_Float16 *)dcopy(xhi, bufs), *d_xlo = hilo ? (_Float16 *)dcopy(xlo, bufs) : nullptr;
        float *d_m0 = ldm ? dcopy(m0, bufs) : nullptr, *d_m1 = ldm ? dcopy(m1, bufs) : nullptr;
        const size_t n_out = ldo ? (size_t)nslab * T * ldo + GUARD : 0, n_oh = ldh ? (size_t)T16 * ldh + GUARD : 0;
        uint32_t *d_out = n_out ? dsent<uint32_t>(n_out, SENT32, bufs) : nullptr;
        uint16_t *d_ohi = n_oh ? dsent<uint16_t>(n_oh, SENT16, bufs) : nullptr, *d_olo = n_oh ? dsent<uint16_t>(n_oh, SENT16, bufs) : nullptr;
        std::vector<unsigned char *> d_pay(n), d_sc(n);
        for (int i = 0; i < n; ++i) {
            const Prob &p = pr[i];
            const _Float16 *raw = (const _Float16 *)dcopy(p.W, bufs);
            d_pay[i] = dsent<unsigned char>(payload_bytes(p.fmt, p.rows, p.K), 0xA5, bufs);
            d_sc[i] = dsent<unsigned char>(scale_bytes(p.fmt, p.rows, p.K), 0xA5, bufs);
            if (p.fmt == W_F16) launch_tile_f16(raw, p.rows, p.rows, p.K, d_pay[i], st);
            else if (p.fmt == W_INT8) launch_quant_int8(raw, p.rows, p.K, d_pay[i], d_sc[i], st);
            else launch_quant_nf4(raw, p.rows, p.K, d_pay[i], d_sc[i], st);
            HIP_OK(hipGetLastError());
            mats[i].data = d_pay[i]; mats[i].scales = p.fmt == W_F16 ? nullptr : d_sc[i];
            mats[i].bytes = payload_bytes(p.fmt, p.rows, p.K) + scale_bytes(p.fmt, p.rows, p.K);
            ProbSpec &s = ps[i];
            s.x.hi = d_xhi; s.x.lo = d_xlo; s.x.ld = ldx;
            s.bias = p.has_bias ? dcopy(p.bias, bufs) : nullptr;
            s.m0 = p.post != POST_NONE ? d_m0 + p.mcol : nullptr; s.m1 = p.post == POST_MIX ? d_m1 + p.mcol : nullptr; s.ldm = ldm;
            s.out = p.ocol >= 0 ? (float *)d_out + p.ocol : nullptr; s.ldo = ldo;
            s.oh = Opd{};
            if (p.hcol >= 0) { s.oh.hi = (_Float16 *)d_ohi + (p.hcol >> 5) * 512; s.oh.lo = p.has_lo ? (_Float16 *)d_olo + (p.hcol >> 5) * 512 : nullptr; s.oh.ld = ldh; }
        }
        HIP_OK(hipStreamSynchronize(st));
        // ---- the launch ----
        if (single) {
            single_mfma_kernel<<<1, 64, 0, st>>>((const _Float16 *)d_pay[0], d_xhi, (float *)d_out);
        } else {
            for (int i = 0; i < n; ++i) fill_prob(Lh.p[i], ps[i], (long)T * ldo);
            if (pl.path == GEMM_SMALLK) launch_smallk(Lh, hilo, st);
            else if (pl.path == GEMM_TILE) launch_gemm_tile(Lh, pl.variant, hilo, st);
            else launch_gemm(Lh, hilo, st);
        }
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st));
        // ---- everything back, whole ----
        const int status = 0;
        std::fwrite(&status, 4, 1, fout);
        put(fout, d_out, n_out);
        put(fout, d_ohi, n_oh);
        put(fout, d_olo, n_oh);
        for (int i = 0; i < n; ++i) {
            put(fout, d_pay[i], payload_bytes(pr[i].fmt, pr[i].rows, pr[i].K));
            put(fout, d_sc[i], scale_bytes(pr[i].fmt, pr[i].rows, pr[i].K));
        }
        std::fflush(fout);
        for (void *p : bufs) HIP_OK(hipFree(p));
        // the line only after the case's results are in the file: the number of lines says which case was running when a process ended early
        if (single) std::printf("{\"case\": %d, \"status\": \"ran\", \"path\": \"single_mfma\"}\n", ci);
        else probe_print(stdout, ci, req, plan);
        std::fflush(stdout);
    }
    HIP_OK(hipStreamDestroy(st));
    std::fclose(fin);
    if (std::fclose(fout)) return 2;
    return 0;
}

// row_probe.hip — stand-alone driver of the row, WKV and state kernels for tests/test_gpu_row_exact.py (DESIGN.md "Row and recurrence probe").
// Not part of librwkv_hip.so: it links the kernel objects the build leaves in ai00_server_amd/csrc and calls only the public launchers
// (launch_wkv, launch_wkv4, launch_ln_shift, launch_embed, launch_ln_out, launch_state_pack), ONE launch per case.
//
//   row_probe <cases.bin> <results.bin>        one JSON line per case on stdout: the launcher arguments that went in
//
// The case file, the result file, the patterns and the order of work per case are those of every role-buffer probe: DESIGN.md "Probe container"
// (tests/cpp/probe_case.h, probe_common.h).  Here: elements of 2 | 4 bytes, `off` a multiple of 256, and the validation of every case BEFORE
// anything is launched: every index the kernel forms from the case's fields lies inside the buffer allocated for it.
#include "../../ai00_server_amd/csrc/rwkv_kernels.h"
#include "probe_common.h"

using namespace rwkv;

enum Kind { K_WKV = 0, K_WKV4, K_LN_SHIFT, K_EMBED, K_LN_OUT, K_STATE_PACK, K_COUNT };
enum Role {
    R_SEQ_SLOT = 0, R_SEQ_BEGIN, R_SEQ_LEN, R_STATE, R_R, R_K, R_V, R_G, R_WDEC, R_U, R_TD, R_D2, R_W7, R_A7, R_VG7, R_KK, R_KA, R_RK, R_VFIRST,
    R_LNW, R_LNB, R_YHI, R_YLO, R_XIN, R_XOUT, R_P, R_SX, R_SLOT, R_PREV, R_LAST, R_XX, R_DX, R_MU0, R_OHI0 = R_MU0 + 6, R_OLO0 = R_OHI0 + 6,
    R_EMB = R_OLO0 + 6, R_TOKEN, R_OUTROWS, R_SLAB, R_SXA, R_SXF, R_WKVST, R_COUNT
};
static const char *const PARAMS[K_COUNT][16] = {
    {"version", "H", "C", "n_seq", "dense", "slot_stride", "Dd", "layer", "ldh", "max_rows", "multi_row", "T", "nslots", nullptr},
    {"C", "n_seq", "dense", "slot_stride", "ldh", "multi_row", "T", "nslots", nullptr},
    {"T", "C", "np", "pstride", "sx_slot_stride", "dense", "mode", "nmix", "ldh", "nslots", nullptr},
    {"T", "C", "V", nullptr},
    {"n_out", "C", "np", "pstride", "ldh", "T", nullptr},
    {"L", "C", "H", "v4", "transposed", "to_slab", "layer_only", nullptr},
};
static const char *const KIND_NAME[K_COUNT] = {"wkv", "wkv4", "ln_shift", "embed", "ln_out", "state_pack"};

// the sequences of a WKV step: distinct slots inside [0, nslots), rows inside [0, T), no row in two sequences
static void check_seqs(const Case &c, int n_seq, int dense, int T, int nslots, bool one_row_each) {
    REQUIRE(c, n_seq >= 1 && T >= 1 && nslots >= 1);
    if (dense) { REQUIRE(c, n_seq <= T && n_seq <= nslots); return; }
    need(c, R_SEQ_SLOT, n_seq, 4); need(c, R_SEQ_BEGIN, n_seq, 4); need(c, R_SEQ_LEN, n_seq, 4);
    const int *sl = c.host<int>(R_SEQ_SLOT), *bg = c.host<int>(R_SEQ_BEGIN), *ln = c.host<int>(R_SEQ_LEN);
    std::vector<char> slot_used(nslots, 0), row_used(T, 0);
    for (int i = 0; i < n_seq; ++i) {
        REQUIRE(c, sl[i] >= 0 && sl[i] < nslots && !slot_used[sl[i]]);
        slot_used[sl[i]] = 1;
        REQUIRE(c, ln[i] >= 1 && bg[i] >= 0 && (int64_t)bg[i] + ln[i] <= T);
        if (one_row_each) REQUIRE(c, ln[i] == 1);
        for (int t = bg[i]; t < bg[i] + ln[i]; ++t) { REQUIRE(c, !row_used[t]); row_used[t] = 1; }
    }
}

static void validate(const Case &c) {
    const std::vector<int64_t> &p = c.p;
    for (const Buf &x : c.b) {
        REQUIRE(c, x.role >= 0 && x.role < R_COUNT && (x.esize == 2 || x.esize == 4) && x.off >= 0 && x.off % 256 == 0 && x.off <= x.nbytes);
        REQUIRE(c, x.nbytes < (int64_t)1 << 31);                       // activation accessors form 32-bit byte offsets
        int same = 0;
        for (const Buf &y : c.b) same += y.role == x.role;
        REQUIRE(c, same == 1);
    }
    switch (c.kind) {
    case K_WKV: {
        REQUIRE(c, p.size() == 13);
        const int ver = p[0], H = p[1], C = p[2], n_seq = p[3], dense = p[4], Dd = p[6], layer = p[7], ldh = p[8], max_rows = p[9], multi = p[10], T = p[11], nslots = p[12];
        const int64_t stride = p[5];
        REQUIRE(c, (ver == 5 || ver == 6 || ver == 7) && H >= 1 && C == 64 * H && ldh % 32 == 0 && ldh >= C && stride >= (int64_t)H * 4096 && max_rows >= 0);
        REQUIRE(c, !(multi && dense));                                 // wkv_chunk_kernel reads seq_* whatever `dense` says
        check_seqs(c, n_seq, dense, T, nslots, false);
        need(c, R_STATE, (int64_t)(nslots - 1) * stride + (int64_t)H * 4096, 4);
        for (int r : {R_R, R_K, R_V, R_G}) need(c, r, (int64_t)T * C, 4);
        need(c, R_LNW, C, 4); need(c, R_LNB, C, 4);
        if (ver != 7) { need(c, R_WDEC, C, 4); need(c, R_U, C, 4); }
        if (ver == 6) { REQUIRE(c, Dd % 32 == 0 && Dd >= 32 && Dd <= 128); need(c, R_TD, (int64_t)T * Dd, 4); need(c, R_D2, (int64_t)C * Dd, 2); }
        if (ver == 7) {
            for (int r : {R_W7, R_A7, R_VFIRST}) need(c, r, (int64_t)T * C, 4);
            for (int r : {R_KK, R_KA, R_RK}) need(c, r, C, 4);
            if (layer != 0) need(c, R_VG7, (int64_t)T * C, 4);
        }
        need(c, R_YHI, ceil16(T) * ldh, 2); need(c, R_YLO, ceil16(T) * ldh, 2, true);
        break;
    }
    case K_WKV4: {
        REQUIRE(c, p.size() == 8);
        const int C = p[0], n_seq = p[1], dense = p[2], ldh = p[4], multi = p[5], T = p[6], nslots = p[7];
        const int64_t stride = p[3];
        REQUIRE(c, C >= 64 && C % 64 == 0 && ldh % 32 == 0 && ldh >= C && stride >= 3LL * C);
        check_seqs(c, n_seq, dense, T, nslots, !multi);               // wkv4_kernel consumes one row per sequence
        need(c, R_STATE, (int64_t)(nslots - 1) * stride + 3LL * C, 4);
        for (int r : {R_R, R_K, R_V}) need(c, r, (int64_t)T * C, 4);
        need(c, R_WDEC, C, 4); need(c, R_U, C, 4);
        need(c, R_YHI, ceil16(T) * ldh, 2); need(c, R_YLO, ceil16(T) * ldh, 2, true);
        break;
    }
    case K_LN_SHIFT: {
        REQUIRE(c, p.size() == 10);
        const int T = p[0], C = p[1], np = p[2], dense = p[5], mode = p[6], nmix = p[7], ldh = p[8], nslots = p[9];
        const int64_t pstride = p[3], stride = p[4];
        REQUIRE(c, T >= 1 && C >= 4 && C % 4 == 0 && C <= 8192 && np >= 0 && np <= 8 && (mode == 0 || mode == 1) && nmix >= 0 && nmix <= 6);
        REQUIRE(c, ldh % 32 == 0 && ldh >= C && stride >= C && nslots >= 1 && pstride >= 0);
        need(c, R_XIN, (int64_t)T * C, 4); need(c, R_XOUT, (int64_t)T * C, 4, true); need(c, R_XX, (int64_t)T * C, 4, true); need(c, R_DX, (int64_t)T * C, 4, true);
        if (np > 0) need(c, R_P, (int64_t)(np - 1) * pstride + (int64_t)T * C, 4);
        need(c, R_LNW, C, 4); need(c, R_LNB, C, 4);
        need(c, R_SX, (int64_t)(nslots - 1) * stride + C, 4);
        for (int m = 0; m < nmix; ++m) { need(c, R_MU0 + m, C, 4); need(c, R_OHI0 + m, ceil16(T) * ldh, 2); need(c, R_OLO0 + m, ceil16(T) * ldh, 2, true); }
        if (dense) { REQUIRE(c, T <= nslots); break; }
        need(c, R_SLOT, T, 4); need(c, R_PREV, T, 4); need(c, R_LAST, T, 4);
        const int *sl = c.host<int>(R_SLOT), *pv = c.host<int>(R_PREV), *la = c.host<int>(R_LAST);
        std::vector<int> writers(nslots, 0);
        for (int t = 0; t < T; ++t) {
            REQUIRE(c, sl[t] >= 0 && sl[t] < nslots && pv[t] >= -1 && pv[t] < T && la[t] >= -1 && la[t] < T);
            if (pv[t] >= 0) REQUIRE(c, sl[pv[t]] == sl[t] && la[t] < 0);
            if (la[t] >= 0) { REQUIRE(c, sl[la[t]] == sl[t] && pv[t] < 0); ++writers[sl[t]]; }
        }
        for (int s = 0; s < nslots; ++s) REQUIRE(c, writers[s] <= 1);   // one block owns a slot's state write
        break;
    }
    case K_EMBED: {
        REQUIRE(c, p.size() == 3);
        const int T = p[0], C = p[1], V = p[2];
        REQUIRE(c, T >= 1 && C >= 4 && C % 4 == 0 && C <= 8192 && V >= 1);
        need(c, R_EMB, (int64_t)V * C, 2); need(c, R_LNW, C, 4); need(c, R_LNB, C, 4); need(c, R_TOKEN, T, 4); need(c, R_XOUT, (int64_t)T * C, 4);
        break;
    }
    case K_LN_OUT: {
        REQUIRE(c, p.size() == 6);
        const int n_out = p[0], C = p[1], np = p[2], ldh = p[4], T = p[5];
        const int64_t pstride = p[3];
        REQUIRE(c, n_out >= 1 && T >= 1 && C >= 4 && C % 4 == 0 && C <= 8192 && np >= 0 && np <= 8 && ldh % 32 == 0 && ldh >= C && pstride >= 0);
        need(c, R_XIN, (int64_t)T * C, 4);
        if (np > 0) need(c, R_P, (int64_t)(np - 1) * pstride + (int64_t)T * C, 4);
        need(c, R_LNW, C, 4); need(c, R_LNB, C, 4);
        need(c, R_OHI0, ceil16(n_out) * ldh, 2); need(c, R_OLO0, ceil16(n_out) * ldh, 2, true);
        if (c.find(R_OUTROWS)) {
            need(c, R_OUTROWS, n_out, 4);
            for (int o = 0; o < n_out; ++o) REQUIRE(c, c.host<int>(R_OUTROWS)[o] >= 0 && c.host<int>(R_OUTROWS)[o] < T);
        } else REQUIRE(c, n_out <= T);
        break;
    }
    case K_STATE_PACK: {
        REQUIRE(c, p.size() == 7);
        const int L = p[0], C = p[1], H = p[2], v4 = p[3], lo = p[6];
        REQUIRE(c, L >= 1 && C >= 1 && H >= 1 && (v4 || C == 64 * H) && lo >= -1 && lo < L && (p[4] == 0 || p[4] == 1) && (p[5] == 0 || p[5] == 1));
        const int64_t N = v4 ? 3 : 64;
        need(c, R_SLAB, lo >= 0 ? N * C : L * (N + 2) * C, 4);
        need(c, R_SXA, (int64_t)L * C, 4); need(c, R_SXF, (int64_t)L * C, 4);
        need(c, R_WKVST, v4 ? (int64_t)L * 3 * C : (int64_t)L * H * 4096, 4);
        break;
    }
    default: refuse(c, "unknown kind");
    }
}

static void launch(const Case &c, hipStream_t s) {
    const std::vector<int64_t> &p = c.p;
    RowMeta rm{c.ptr<int>(R_TOKEN), c.ptr<int>(R_SLOT), c.ptr<int>(R_PREV), c.ptr<int>(R_LAST), 0};
    switch (c.kind) {
    case K_WKV: {
        WkvArgs a{};
        a.version = p[0]; a.H = p[1]; a.C = p[2]; a.n_seq = p[3]; a.dense = p[4]; a.slot_stride = p[5]; a.Dd = p[6]; a.layer = p[7]; a.ldh = p[8]; a.max_rows = p[9];
        a.seq_slot = c.ptr<int>(R_SEQ_SLOT); a.seq_begin = c.ptr<int>(R_SEQ_BEGIN); a.seq_len = c.ptr<int>(R_SEQ_LEN);
        a.state = c.ptr<float>(R_STATE);
        a.r = c.ptr<float>(R_R); a.k = c.ptr<float>(R_K); a.v = c.ptr<float>(R_V); a.g = c.ptr<float>(R_G);
        a.wdec_or_decay = c.ptr<float>(R_WDEC); a.u = c.ptr<float>(R_U); a.td = c.ptr<float>(R_TD); a.D2 = c.ptr<_Float16>(R_D2);
        a.w7 = c.ptr<float>(R_W7); a.a7 = c.ptr<float>(R_A7); a.vg7 = c.ptr<float>(R_VG7);
        a.k_k = c.ptr<float>(R_KK); a.k_a = c.ptr<float>(R_KA); a.r_k = c.ptr<float>(R_RK); a.v_first = c.ptr<float>(R_VFIRST);
        a.lnx_w = c.ptr<float>(R_LNW); a.lnx_b = c.ptr<float>(R_LNB); a.yhi = c.ptr<_Float16>(R_YHI); a.ylo = c.ptr<_Float16>(R_YLO);
        launch_wkv(a, p[10] != 0, s);
        break;
    }
    case K_WKV4: {
        Wkv4Args a{};
        a.C = p[0]; a.n_seq = p[1]; a.dense = p[2]; a.slot_stride = p[3]; a.ldh = p[4];
        a.seq_slot = c.ptr<int>(R_SEQ_SLOT); a.seq_begin = c.ptr<int>(R_SEQ_BEGIN); a.seq_len = c.ptr<int>(R_SEQ_LEN);
        a.state = c.ptr<float>(R_STATE); a.r = c.ptr<float>(R_R); a.k = c.ptr<float>(R_K); a.v = c.ptr<float>(R_V);
        a.w = c.ptr<float>(R_WDEC); a.u = c.ptr<float>(R_U); a.yhi = c.ptr<_Float16>(R_YHI); a.ylo = c.ptr<_Float16>(R_YLO);
        launch_wkv4(a, p[5] != 0, s);
        break;
    }
    case K_LN_SHIFT: {
        LnShiftArgs a{};
        a.x_in = c.ptr<float>(R_XIN); a.x_out = c.ptr<float>(R_XOUT); a.P = c.ptr<float>(R_P); a.np = p[2]; a.pstride = p[3];
        a.lnw = c.ptr<float>(R_LNW); a.lnb = c.ptr<float>(R_LNB); a.sx = c.ptr<float>(R_SX); a.sx_slot_stride = p[4];
        a.rm = rm; a.rm.dense = p[5]; a.mode = p[6]; a.nmix = p[7]; a.ldh = p[8]; a.C = p[1];
        for (int m = 0; m < 6; ++m) { a.mu[m] = c.ptr<float>(R_MU0 + m); a.ohi[m] = c.ptr<_Float16>(R_OHI0 + m); a.olo[m] = c.ptr<_Float16>(R_OLO0 + m); }
        a.xx_out = c.ptr<float>(R_XX); a.dx_out = c.ptr<float>(R_DX);
        launch_ln_shift(a, (int)p[0], s);
        break;
    }
    case K_EMBED: {
        EmbedArgs a{};
        a.emb = c.ptr<_Float16>(R_EMB); a.lnw = c.ptr<float>(R_LNW); a.lnb = c.ptr<float>(R_LNB); a.token = c.ptr<int>(R_TOKEN); a.x = c.ptr<float>(R_XOUT);
        a.C = p[1]; a.V = p[2];
        launch_embed(a, (int)p[0], s);
        break;
    }
    case K_LN_OUT: {
        LnOutArgs a{};
        a.x_in = c.ptr<float>(R_XIN); a.P = c.ptr<float>(R_P); a.np = p[2]; a.pstride = p[3]; a.lnw = c.ptr<float>(R_LNW); a.lnb = c.ptr<float>(R_LNB);
        a.out_rows = c.ptr<int>(R_OUTROWS); a.ohi = c.ptr<_Float16>(R_OHI0); a.olo = c.ptr<_Float16>(R_OLO0); a.ldh = p[4]; a.C = p[1];
        launch_ln_out(a, (int)p[0], s);
        break;
    }
    default: {
        StatePackArgs a{};
        a.slab = c.ptr<float>(R_SLAB); a.sxa = c.ptr<float>(R_SXA); a.sxf = c.ptr<float>(R_SXF); a.wkv = c.ptr<float>(R_WKVST);
        a.L = p[0]; a.C = p[1]; a.H = p[2]; a.v4 = p[3]; a.transposed = p[4]; a.to_slab = p[5]; a.layer_only = p[6];
        launch_state_pack(a, s);
        break;
    }
    }
    launched(s);
}

static void fields(const Case &c) {
    std::printf(", \"launcher\": \"%s\"", KIND_NAME[c.kind]);
    for (size_t i = 0; i < c.p.size() && PARAMS[c.kind][i]; ++i) std::printf(", \"%s\": %lld", PARAMS[c.kind][i], (long long)c.p[i]);
}

int main(int argc, char **argv) {
    return probe_main<Case>(argc, argv, ProbeSpec{"row_probe", 0x42525052, K_COUNT, 16, R_COUNT, 2}, validate, launch, fields);
}

// rwkv_engine.cpp — host side of librwkv_hip.so: loader, engine, step planner, C ABI.
//
// Replaces, behind include/rwkv_abi.h, the web-rwkv objects ai00-core holds:
//   Context + ModelBuilder + vN::Bundle + TokioRuntime<Rnn>  (crates/ai00-core/src/lib.rs:391-516)
//   State {init,load,back,read,write}                         (run.rs:477, 1099-1106)
//   softmax::softmax                                          (run.rs:1179)
// No CPU fallback: every entry point that computes needs a gfx950 device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rwkv_abi.h"
#include "gemm_plan.h"
#include "gen_host.h"
#include "graph_cache.h"
#include "rwkv_dfa.h"
#include "rwkv_pda.h"
#include "safetensors.hpp"

using namespace rwkv;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
struct RwkvError : std::runtime_error {
    rwkv_status code;
    RwkvError(rwkv_status c, const std::string &m) : std::runtime_error(m), code(c) {}
};
#define HIP_CHECK(x)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (x);                                                                           \
        if (_e != hipSuccess)                                                                          \
            throw RwkvError(_e == hipErrorOutOfMemory ? RWKV_ERR_OOM : RWKV_ERR_DEVICE,                \
                            std::string(#x) + ": " + hipGetErrorString(_e));                           \
    } while (0)

template <class F>
static rwkv_status guard(F &&f) {
    try {
        f();
        return RWKV_OK;
    } catch (const RwkvError &e) {
        g_err = e.what();
        return e.code;
    } catch (const std::bad_alloc &) {
        g_err = "host out of memory";
        return RWKV_ERR_OOM;
    } catch (const std::exception &e) {
        g_err = e.what();
        return std::strncmp(e.what(), "safetensors:", 12) == 0 ? RWKV_ERR_FORMAT : RWKV_ERR_INVALID;
    }
}

// The one place a stream is put into capture mode: what `enqueue` puts on `st` becomes an executable graph.  If `enqueue` throws, the capture is
// ended and the half-built graph destroyed before the exception goes on, so the stream is never left capturing.
template <class F>
static hipGraphExec_t capture(hipStream_t st, F &&enqueue) {
    hipGraph_t g = nullptr;
    HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    try {
        enqueue();
    } catch (...) {
        (void)hipStreamEndCapture(st, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
    }
    HIP_CHECK(hipStreamEndCapture(st, &g));
    hipGraphExec_t exec = nullptr;
    const hipError_t err = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIP_CHECK(err);
    return exec;
}
struct GraphExecDeleter { void operator()(hipGraphExec_t x) const { if (x) (void)hipGraphExecDestroy(x); } };
template <class Key>
using GraphCacheOf = GraphCache<Key, hipGraphExec_t, GraphExecDeleter>;

// ------------------------------------------------------------------------------------------------
// model info (Loader::info, lib.rs:587)
// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// Prefab: the loaded (re-tiled / quantised / converted) model as one binary image, so that a later load skips the
// safetensors parse, the LoRA blend and the GPU re-tile / quantise passes.  Counterpart of `ModelSerialize::serialize`
// (lib.rs:131-154) and `LoadType::Prefab` (lib.rs:517-553, sniffed at lib.rs:585-588); the reference's CBOR image of
// web-rwkv's internal tensors is not reproducible here, this is our own versioned format:
//   header  { char magic[8] "RWKVHIP\0"; u32 version; u32 n_entries; rwkv_model_info info; i32 quant_layers, quant_type; }
//   entries { u32 kind (0 f32 vector, 1 raw f16, 2 tiled matrix); i32 fmt, rows, K; u32 counted; u32 name_len;
//             u64 n_elems, data_bytes, scale_bytes; name[name_len]; pad to 16; data; pad to 16; scales; pad to 16 }
// ------------------------------------------------------------------------------------------------
static const char kPrefabMagic[8] = {'R', 'W', 'K', 'V', 'H', 'I', 'P', 0};
constexpr uint32_t kPrefabVersion = 1;
struct PfEntryHead { uint32_t kind; int32_t fmt, rows, K; uint32_t counted, name_len; uint64_t n_elems, data_bytes, scale_bytes; };
struct PfHeader { char magic[8]; uint32_t version, n_entries; rwkv_model_info info; int32_t quant_layers, quant_type; };
struct PfEntry { PfEntryHead h; const uint8_t *data = nullptr, *scales = nullptr; };
// the dimension rules every loaded model must satisfy (kernel tiling), whether the header comes from tensor shapes or a prefab
static void validate_info(const rwkv_model_info &i) {
    if (i.version != 4 && i.version != 5 && i.version != 6 && i.version != 7) throw RwkvError(RWKV_ERR_UNSUPPORTED, "unsupported model version");
    if (i.num_layer <= 0 || i.num_layer > 4096 || i.num_emb <= 0 || i.num_hidden <= 0 || i.num_vocab <= 0 || i.num_head <= 0 ||
        i.num_vocab > (1 << 24) || i.num_hidden > (1 << 20))
        throw RwkvError(RWKV_ERR_FORMAT, "model dimensions out of range");
    if (i.version == 4) {                                        // V4 has no heads: reported as one head of num_emb channels
        if (i.num_head != 1 || i.head_size != i.num_emb) throw RwkvError(RWKV_ERR_FORMAT, "a V4 model has num_head 1 and head_size num_emb");
    } else if (i.head_size != 64 || (int64_t)i.num_emb != (int64_t)i.num_head * 64) throw RwkvError(RWKV_ERR_UNSUPPORTED, "head size must be 64");
    if (i.num_emb % 64 || i.num_hidden % 32 || i.num_vocab % 16)
        throw RwkvError(RWKV_ERR_UNSUPPORTED, "dims must satisfy C%64==0, F%32==0, V%16==0");
    if (i.num_emb > 8192) throw RwkvError(RWKV_ERR_UNSUPPORTED, "num_emb > 8192");
}
static bool prefab_sniff(const uint8_t *b, size_t n) { return b && n >= sizeof(PfHeader) && std::memcmp(b, kPrefabMagic, 8) == 0; }
struct Prefab {
    PfHeader hdr{};
    std::map<std::string, PfEntry> entries;
    static Prefab parse(const uint8_t *b, size_t n) {
        Prefab p;
        if (!prefab_sniff(b, n)) throw RwkvError(RWKV_ERR_FORMAT, "not a prefab image");
        std::memcpy(&p.hdr, b, sizeof(PfHeader));
        if (p.hdr.version != kPrefabVersion) throw RwkvError(RWKV_ERR_UNSUPPORTED, "prefab version mismatch");
        validate_info(p.hdr.info);
        size_t off = sizeof(PfHeader);
        // every length comes from the file: compare against what is LEFT (len > n - off), never off + len (which can wrap)
        auto take = [&](uint64_t len) -> const uint8_t * {            // `len` bytes at `off`, then `off` up to the next 16-byte FILE offset
            if (off > n || len > (uint64_t)(n - off)) throw RwkvError(RWKV_ERR_FORMAT, "prefab truncated");
            const uint8_t *q = b + off;
            const size_t end = off + (size_t)len;                     // <= n (an in-memory size): neither this nor + 15 can wrap
            off = std::min(n, (end + 15) & ~(size_t)15);              // padding cut off at the end of the file is harmless
            return q;
        };
        for (uint32_t i = 0; i < p.hdr.n_entries; ++i) {
            PfEntry e;
            const uint8_t *hp = take(sizeof(PfEntryHead));
            std::memcpy(&e.h, hp, sizeof(PfEntryHead));
            // the 16-byte padding applies after name / data / scales, not after the fixed head
            off = (size_t)(hp - b) + sizeof(PfEntryHead);
            if (e.h.name_len > 4096) throw RwkvError(RWKV_ERR_FORMAT, "prefab: entry name too long");
            std::string name((const char *)take(e.h.name_len), e.h.name_len);
            e.data = take(e.h.data_bytes);
            e.scales = e.h.scale_bytes ? take(e.h.scale_bytes) : nullptr;
            // payload sizes must be the ones save_prefab computes from the entry's own description
            const uint64_t ne = e.h.n_elems;
            if (e.h.kind == 0) { if (ne > (1ull << 40) || e.h.data_bytes != ne * 4 || e.h.scale_bytes) throw RwkvError(RWKV_ERR_FORMAT, "prefab: bad vector entry " + name); }
            else if (e.h.kind == 1) { if (ne > (1ull << 40) || e.h.data_bytes != ne * 2 || e.h.scale_bytes) throw RwkvError(RWKV_ERR_FORMAT, "prefab: bad fp16 entry " + name); }
            else if (e.h.kind == 2) {
                const int64_t rows = e.h.rows, K = e.h.K;
                bool ok = rows > 0 && K > 0 && rows % 16 == 0 && rows <= (1 << 24) && K <= (1 << 24);
                uint64_t db = 0, sb = 0;
                if (ok && e.h.fmt == W_F16) { ok = K % 32 == 0; db = (uint64_t)rows * K * 2; }
                else if (ok && e.h.fmt == W_INT8) { ok = K % 256 == 0; db = (uint64_t)rows * K; sb = (uint64_t)rows * (K / 128) * 4; }
                else if (ok && fmt_is_4bit(e.h.fmt)) { ok = K % 256 == 0; db = (uint64_t)rows * K / 2; sb = (uint64_t)rows * (K / 64) * 2; }
                else ok = false;
                if (!ok || e.h.data_bytes != db || e.h.scale_bytes != sb) throw RwkvError(RWKV_ERR_FORMAT, "prefab: bad matrix entry " + name);
            } else throw RwkvError(RWKV_ERR_FORMAT, "prefab: unknown entry kind");
            p.entries.emplace(std::move(name), e);
        }
        return p;
    }
    const PfEntry &get(const std::string &name, uint32_t kind) const {
        auto it = entries.find(name);
        if (it == entries.end() || it->second.h.kind != kind) throw RwkvError(RWKV_ERR_FORMAT, "prefab: missing entry " + name);
        return it->second;
    }
    bool has(const std::string &name) const { return entries.count(name) != 0; }
};

// V4 is taken on positive evidence only: none of the tensors a later version adds, time_first / time_decay as plain [C] vectors, and the five
// token-shift mixes of its time mix and channel mix
static bool looks_like_v4(const SafeTensors &st) {
    for (const char *n : {"att.ln_x.weight", "att.gate.weight", "att.time_mix_x", "att.x_r"})
        if (st.find(std::string("blocks.0.") + n)) return false;
    const StTensor *emb = st.find("emb.weight");
    if (!emb || emb->shape.size() != 2) return false;
    for (const char *n : {"att.time_first", "att.time_decay"}) {
        const StTensor *t = st.find(std::string("blocks.0.") + n);
        if (!t || (int64_t)t->numel() != (int64_t)emb->shape[1]) return false;
    }
    for (const char *n : {"att.time_mix_k", "att.time_mix_v", "att.time_mix_r", "ffn.time_mix_k", "ffn.time_mix_r"})
        if (!st.find(std::string("blocks.0.") + n)) return false;
    return true;
}

static rwkv_model_info detect_info(const SafeTensors &st) {
    rwkv_model_info i{};
    if (st.find("blocks.0.att.x_r")) i.version = 7;
    else if (st.find("blocks.0.att.time_mix_x")) i.version = 6;
    else if (st.find("blocks.0.att.ln_x.weight") && st.find("blocks.0.att.gate.weight")) {
        const StTensor &td = st.get("blocks.0.att.time_decay");
        if (td.shape.size() < 2 || td.shape.back() <= 1)
            throw RwkvError(RWKV_ERR_UNSUPPORTED, "RWKV v5.0/v5.1 checkpoints are not supported (need v5.2)");
        i.version = 5;
    } else if (looks_like_v4(st)) i.version = 4;
    else
        throw RwkvError(RWKV_ERR_UNSUPPORTED, "unsupported model version (v4 or unknown tensor naming)");
    int L = 0;
    while (st.find("blocks." + std::to_string(L) + ".ln1.weight")) ++L;
    const StTensor &emb = st.get("emb.weight");
    if (emb.shape.size() != 2) throw RwkvError(RWKV_ERR_FORMAT, "emb.weight must be 2-D");
    i.num_layer = L;
    i.num_vocab = (int)emb.shape[0];
    i.num_emb = (int)emb.shape[1];
    auto dim0 = [&](const char *name, size_t min_rank) -> int {
        const StTensor &t = st.get(name);
        if (t.shape.size() < min_rank || t.shape[0] <= 0 || t.shape[0] > (1 << 24)) throw RwkvError(RWKV_ERR_FORMAT, std::string(name) + ": unexpected shape");
        return (int)t.shape[0];
    };
    if (emb.shape[0] <= 0 || emb.shape[0] > (1 << 24) || emb.shape[1] <= 0 || emb.shape[1] > (1 << 20)) throw RwkvError(RWKV_ERR_FORMAT, "emb.weight: unexpected shape");
    i.num_hidden = dim0("blocks.0.ffn.key.weight", 2);
    i.num_head = i.version == 4 ? 1 : i.version == 7 ? dim0("blocks.0.att.r_k", 2) : dim0("blocks.0.att.time_first", 2);
    i.head_size = i.num_emb / std::max(1, i.num_head);
    validate_info(i);
    return i;
}

// ------------------------------------------------------------------------------------------------
// engine
// ------------------------------------------------------------------------------------------------
enum Family { FAM_GEMM = 0, FAM_HEAD = 1, FAM_ROW = 2, FAM_WKV = 3, FAM_SAMPLE = 4, FAM_COPY = 5 };
static const char *kFamilyNames[RWKV_PROFILE_FAMILIES] = {"gemm_layers", "gemm_head", "row_ln_shift", "wkv", "sample", "copy", "", ""};

struct LayerW {
    const float *ln1w, *ln1b, *ln2w, *ln2b, *lnxw, *lnxb;
    const float *mu[6];             // att mixes (v4: k,v,r; v5: k,v,r,g; v6: x,w,k,v,r,g; v7: r,w,k,v,a,g)
    const float *fmu[2];            // ffn mixes (v5/v6: k,r; v7: k)
    const DMat *Wr, *Wk, *Wv, *Wg, *Wo, *Fk, *Fv, *Fr;
    // v5/v6
    const float *wdec;              // v4: -exp(decay); v5: exp(-exp(decay)); v6: raw time_decay
    const float *u;
    const DMat *W1;                 // v6 time_mix_w1 [5Dm x C]
    const DMat *W2[5];              // v6 time_mix_w2 [C x Dm] x5
    const DMat *D1;                 // v6 time_decay_w1 [Dd x C]
    const _Float16 *D2;             // v6 time_decay_w2 raw [C][Dd]
    // v7
    const DMat *w1, *w2, *a1, *a2, *v1, *v2, *g1, *g2;
    const float *w0, *a0, *v0, *k_k, *k_a, *r_k;
};

struct StepPlan {
    bool dense = false;             // slots 0..T-1 active with one token each, every row emitted: row index == slot index
    int T = 0, n_seq = 0, n_out = 0;
    std::vector<int> token, slot, prev, last, seq_slot, seq_begin, seq_len, out_rows;
    std::vector<int> slot_consumed, slot_out_begin, slot_out_rows;   // per slot
    uint64_t id = 0;                // plans with the same id have identical metadata apart from the token ids
    int max_rows() const { return seq_len.empty() ? 0 : *std::max_element(seq_len.begin(), seq_len.end()); }   // most rows any sequence has
};

// Row metadata of a step: the one description of d_meta, and of each pinned staging buffer that is copied over it whole.
struct MetaView {
    int *token, *slot, *prev, *last, *out_rows;                 // [chunk] each: per row (out_rows: the rows that reach the head)
    int *seq_slot, *seq_begin, *seq_len;                        // [max_batch] each: per sequence of the step
    static size_t words(int chunk, int B) { return (size_t)chunk * 5 + (size_t)B * 3 + 16; }
    MetaView(int *base = nullptr, int chunk = 0, int B = 0)
        : token(base), slot(token + chunk), prev(slot + chunk), last(prev + chunk), out_rows(last + chunk),
          seq_slot(out_rows + chunk), seq_begin(seq_slot + B), seq_len(seq_begin + B) {}
};

// rwkv_infer_sample's pinned block: per-row parameters in [chunk], sparse logit adjustments in [ADJ_CAP] x 3, 8 bytes per row out [chunk] x 2
// (the kernels read the rows and write the outputs in place, through the block's device-visible alias: dv_*)
struct SampStage { SampleRow *rows; int *adj_row, *adj_tok; float *adj_val; int *out_tok; float *out_prob; const SampleRow *dv_rows; int *dv_out_tok; float *dv_out_prob; };

// which sampler kernels a set of rows needs: the NEEDS_* bits
static unsigned sampler_need(int kind, bool wide = false) { return wide ? NEEDS_WIDE : kind == RWKV_SAMPLER_MIROSTAT ? NEEDS_MIRO : NEEDS_NT; }
// Mirostat below 13 bits of surprise admits fewer than 2^13 tokens (p >= 2^-max_surprise each, plus one): nucleus_kernel's buffer is exact there
constexpr float MIRO_WIDE_SURPRISE = 13.0f;
constexpr int NARROW_TOP_K = 256;

struct rwkv_dstate {
    int device = 0;
    float *sxa = nullptr, *sxf = nullptr, *wkv = nullptr;
};

// An open watch (rwkv_gen_watch_open): one mapped, coherent host block laid out by gen_watch.h, which the steps write through its device
// alias.  read / head / cancel touch nothing but this block: no HIP call, no lock, nothing the infer thread holds.
struct rwkv_gen_watch {
    unsigned char *ring = nullptr;                             // records | head | cancel words
    int ring_steps = 0, B = 0;
    unsigned *cancel() const { return gen_watch_cancel_ptr(ring, ring_steps, B); }
};

// A cached (state, output) pair on the device (rwkv_gen_take_item / rwkv_gen_item_from_host; CachedItem, run.rs:201-223).  It owns its
// memory and belongs to no engine: `st` is the borrowed view rwkv_gen_item_state hands out, into `state`.
struct rwkv_gen_item {
    rwkv_dstate st;                                            // device; sxa | sxf | wkv inside `state` (internal layout, as a slot's)
    float *state = nullptr, *row = nullptr;                    // [2 * nsx + nw], [V] the RAW head row
    int version = 0, L = 0, C = 0, V = 0;
    long nsx = 0, nw = 0;
};
static void gen_item_destroy(rwkv_gen_item *it) {
    if (!it) return;
    (void)hipSetDevice(it->st.device);
    (void)hipFree(it->state); (void)hipFree(it->row);
    delete it;
}

// What the host keeps per slot of resident generation (rwkv_engine::gen_slots).  The has_stops / constraint / topn / capture words are host
// knowledge of what the slot's device entries hold: they select the kernels of a step (feats).
enum class GenConstraint : char { None, Dfa, Pda };            // a slot holds a byte automaton or a stack automaton, never both
struct GenSlotHost {
    GenSlot g{};                                               // mirror of d_gen[slot], read back after every run
    bool armed = false;
    std::vector<uint32_t> prompt;                              // rwkv_gen_arm_prompt: the slot's prompt tail, and how much of it the steps so far
    size_t ppos = 0;                                           //   have consumed (each mixed step's slice rides in its plan upload)
    float *shadow = nullptr;                                   // sxa | sxf | wkv of the step it finished in (dalloc, by the slot's first arm)
    GenConstraint constraint = GenConstraint::None;
    void *table = nullptr;                                     // the constraint's planes on the device (trans | flags, or next | act | flags); not in `allocs`
    bool has_stops = false;
    int topn = 0;                                              // places it lists, 0 = none (d_gen_topn_n holds the same)
    unsigned capture = 0, cap_done = 0, cap_taken = 0;         // RWKV_GEN_CAPTURE_* asked for / PROMPT written / handed over
    std::array<rwkv_gen_item *, 2> cap_item{nullptr, nullptr}; // the PROMPT and the FINISH item until they are taken
    float *inj_row = nullptr;                                  // [V] the row of the item that armed it (dalloc, by the slot's first rwkv_gen_arm_item)
    bool inj = false;                                          // its first draw, from that row, is still to come
    size_t prompt_left() const { return armed ? prompt.size() - ppos : 0; }
    uint64_t feats() const {                                   // what the slot adds to a step it has a row in
        return (has_stops ? FEAT_STOPS : 0) | (constraint == GenConstraint::Dfa ? FEAT_DFA : 0) | (constraint == GenConstraint::Pda ? FEAT_PDA : 0) |
               (topn ? FEAT_TOPN : 0) | (capture & ~cap_taken & RWKV_GEN_CAPTURE_FINISH ? FEAT_CAPTURE : 0);
    }
    void drop_items() { for (rwkv_gen_item *&it : cap_item) { gen_item_destroy(it); it = nullptr; } }   // asked for, never taken
    // What ends with a request (gen_arm, gen_disarm_slot); the device entries are rewritten by the next arm, nothing reads them before.
    // What stays: `g` (gen_arm overwrites it; a disarmed slot's finish word is the watch's to drop), `topn` (gen_arm clears it with the
    // device's word), `shadow` and `inj_row` (allocated once per slot), `table` (freed behind a stream synchronise only: gen_drop_table).
    void reset_request() {
        drop_items();
        capture = cap_done = cap_taken = 0;
        armed = has_stops = inj = false;
        constraint = GenConstraint::None;
        prompt.clear();
        ppos = 0;
    }
};

struct rwkv_engine {
    rwkv_model_info info{};
    int device = 0;
    int max_batch = 8, chunk = 128;
    bool hilo = false;
    // Operand promotion: in Precision::Fp16 the GEMM launches of the classes whose bit is set read hi + lo f16 operands like Precision::Fp32
    // does everywhere — the price of exactness is paid only where a model's error comes from (profiles/r5_fp16_error_attribution_*.jsonl:
    // V7's Wr / Wk / Wv inputs carry 4.7e-3 of its 4.9e-3 at 32 layers).  The mask is chosen from the model version (promote_for_version):
    // that IS RWKV_PRECISION_FP16 since ABI 7; RWKV_PRECISION_FP16_RAW is mask 0; RWKV_PROMOTE=<mask> is a dev override of either.
    enum OpdClass { CLS_ATT = 0, CLS_LORA2 = 1, CLS_WO = 2, CLS_FFN1 = 3, CLS_FV = 4, CLS_HEAD = 5, CLS_NONE = 31 };
    static int promote_for_version(int version) { return version == 7 ? 7 : 1; }   // V4 / V5 / V6: CLS_ATT; V7: CLS_ATT | CLS_LORA2 | CLS_WO
    int promote = 0;
    bool wide(int cls) const { return hilo || (cls < 31 && ((promote >> cls) & 1)); }
    int quant_layers = 0, quant_type = 0;
    hipStream_t s_main = nullptr, s_soft = nullptr;
    FILE *launch_log = nullptr;                                // RWKV_LAUNCH_LOG=<path> (dev): one JSON line per GEMM launch of layer 0 / the head
    int cur_layer = -1;                                        //   (grid, rows, K, stored bytes, flops): scripts/roofline_table.py joins it with rocprofv3's CSV
    hipStream_t s_copy = nullptr;                              // rwkv_state_back_layer_async: pack + device-to-host copy beside the compute stream
    hipEvent_t ev_copy_a = nullptr, ev_copy_b = nullptr;
    float *emb_stage = nullptr;                                // [max_batch][64 * C] (V4: [3 * C]): one packed layer slice per slot
    std::vector<void *> allocs, host_allocs;                   // dalloc / hostalloc
    std::map<std::string, DMat> mats;
    std::map<std::string, float *> vecs;
    std::map<std::string, _Float16 *> raws;
    std::map<std::string, std::pair<size_t, bool>> vec_meta, raw_meta;   // element count, counted-in-weight_bytes (prefab save)
    void save_prefab(const char *path);
    std::vector<LayerW> layers;
    const float *ln0w, *ln0b, *lnow, *lnob;
    const _Float16 *emb = nullptr;
    const DMat *head = nullptr;
    uint64_t weight_bytes = 0;
    int Dm = 0, Dd = 0, Dl = 0;     // LoRA dims (v6: Dm, Dd; v7: max of w/a/v/g dims)

    // state (internal layout)
    float *sxa = nullptr, *sxf = nullptr, *wkv = nullptr;
    long sx_slot_stride = 0, wkv_slot_stride = 0;
    // views (they own nothing): a slot's state, and a contiguous sxa | sxf | wkv block (a slot's shadow, an item's `state`)
    rwkv_dstate slot_state(int slot) const { return {device, sxa + slot * sx_slot_stride, sxf + slot * sx_slot_stride, wkv + slot * wkv_slot_stride}; }
    rwkv_dstate block_state(float *block) const { return {device, block, block + sx_slot_stride, block + 2 * sx_slot_stride}; }
    void copy_state(const rwkv_dstate &dst, const rwkv_dstate &src) {   // on s_main, not waited for
        HIP_CHECK(hipMemcpyAsync(dst.sxa, src.sxa, (size_t)sx_slot_stride * 4, hipMemcpyDeviceToDevice, s_main));
        HIP_CHECK(hipMemcpyAsync(dst.sxf, src.sxf, (size_t)sx_slot_stride * 4, hipMemcpyDeviceToDevice, s_main));
        HIP_CHECK(hipMemcpyAsync(dst.wkv, src.wkv, (size_t)wkv_slot_stride * 4, hipMemcpyDeviceToDevice, s_main));
    }
    // The state as the ABI shows it has slab_rows() rows of C floats per layer: the two shift rows around the layer's WKV rows.  V5 / V6 / V7: 64
    // WKV rows, the H 64 x 64 head matrices (wkv_layer_floats = H * 4096).  V4: three, aa / bb / pp (wkv_layer_floats = 3 * C).
    int slab_rows() const { return info.version == 4 ? 5 : 66; }
    long wkv_layer_floats() const { return (long)(slab_rows() - 2) * info.num_emb; }
    size_t state_len() const { return (size_t)info.num_layer * slab_rows() * info.num_emb; }
    void fill_init_state(float *dst) const {                     // the slab `state.init()` hands out
        std::fill(dst, dst + state_len(), 0.f);
        if (info.version != 4) return;
        const size_t C = (size_t)info.num_emb;
        for (int l = 0; l < info.num_layer; ++l) std::fill(dst + ((size_t)l * 5 + 3) * C, dst + ((size_t)l * 5 + 4) * C, V4_PP_INIT);
    }
    static constexpr float V4_PP_INIT = -1e30f;                  // [EXT] include/rwkv_abi.h
    float *slab_dev = nullptr;      // staging for pack/unpack
    float *slab_host = nullptr;     // pinned

    // scratch
    float *xA = nullptr, *xB = nullptr, *P = nullptr, *xx = nullptr, *dx = nullptr;
    float *fr = nullptr, *fk = nullptr, *fv = nullptr, *fg = nullptr, *ftd = nullptr, *frr = nullptr;
    float *fw7 = nullptr, *fa7 = nullptr, *fvg7 = nullptr, *vfirst = nullptr;
    float *logits = nullptr, *logits_host = nullptr;
    float *soft_in = nullptr, *soft_out = nullptr, *soft_host = nullptr;
    size_t soft_rows_cap = 0;
    // scoring (rwkv_infer_score on s_main, rwkv_score_rows on s_soft): one target in and one ln-probability out per logits row; pinned mirrors
    unsigned *d_score_tgt = nullptr, *h_score_tgt = nullptr, *d_soft_tgt = nullptr, *h_soft_tgt = nullptr;
    float *d_score_out = nullptr, *h_score_out = nullptr, *d_soft_score = nullptr, *h_soft_score = nullptr;
    // top-n lists (rwkv_infer_topn on s_main, rwkv_topn_rows on s_soft): TOPN_MAX ids and ln-probabilities per logits row; pinned mirrors
    unsigned *d_topn_ids = nullptr, *h_topn_ids = nullptr, *d_soft_topn_ids = nullptr, *h_soft_topn_ids = nullptr;
    float *d_topn_logp = nullptr, *h_topn_logp = nullptr, *d_soft_topn_logp = nullptr, *h_soft_topn_logp = nullptr;
    Opd opA[6], opM, opY, opK, opO, opL[4];
    long pstride = 0;
    // row meta (device + pinned host)
    int *d_meta = nullptr, *h_meta = nullptr;                  // h_meta: a ring of META_RING pinned staging buffers (state-only steps are not waited for)
    MetaView dm;                                               // the sections of d_meta
    static constexpr int META_RING = 4;
    hipEvent_t meta_ev[META_RING] = {nullptr, nullptr, nullptr, nullptr};
    int meta_next = 0;
    int *h_tok = nullptr, *dv_tok = nullptr;               // pinned token ids of a dense step and their device-visible alias
    StepPlan last_plan;                                    // plan cache: a serving loop repeats the same dense decode pattern
    std::vector<size_t> last_ntok;
    std::vector<int> last_opt;
    uint64_t plan_counter = 0, uploaded_id = 0;
    size_t meta_cap = 0;
    int *d_tok_feedback = nullptr, *d_hist = nullptr, *d_amax_i = nullptr;
    // sampling front-end: per-row params, sparse adjustments (row, token, value), outputs; pinned host mirror
    int *d_adj_row = nullptr, *d_adj_tok = nullptr;
    float *d_adj_val = nullptr;
    unsigned char *d_allow = nullptr, *h_allow = nullptr;   // formatter masks of the rows that carry one: [n][V] bytes, pinned mirror
    int *d_allow_row = nullptr;
    SampStage samp{};
    static constexpr size_t ADJ_CAP = 1 << 16;
    float *d_amax_v = nullptr;
    size_t hist_cap = 0;

    // profiling
    bool profiling = false;
    float prof_ms[RWKV_PROFILE_FAMILIES] = {0};
    int prof_n[RWKV_PROFILE_FAMILIES] = {0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    // captured steps (graph_cache.h holds the policy: captured on second sight, least recently used evicted)
    GraphCacheOf<uint64_t> graphs{64, {}};                     // run_plan: keyed by step shape
    std::optional<GraphCacheOf<int>> greedy_graphs;            // rwkv_decode_greedy: step + arg-max feedback, keyed by slot count; room for every count
    // device-resident sampled generation (rwkv_gen_*): per-slot contexts, dense penalty / bias rows, the step's SampleRow array and the
    // output ring live on the device; everything is allocated by the first rwkv_gen_arm
    static constexpr int GEN_RING_STEPS = 1024;                  // steps one enqueue covers (longer runs are split)
    std::vector<GenSlotHost> gen_slots;                          // [max_batch] by gen_init; empty: the engine never generated
    GenSlot *d_gen = nullptr;
    // stop STRINGS (rwkv_gen_set_token_bytes / _set_stops): the engine's token-bytes table and, beside d_gen, one GenStop per slot
    GenStop *d_gen_stop = nullptr;
    unsigned *d_tok_off = nullptr;                               // [n_tok + 1]; not in `allocs`: a new table replaces it
    unsigned char *d_tok_bytes = nullptr;
    int n_tok = 0;
    void gen_set_token_bytes(const uint8_t *bytes, const int32_t *lens, size_t n);
    void gen_set_stops(int slot, const rwkv_gen_stops &s);
    size_t gen_stop_tail(int slot, uint8_t *out, size_t cap);
    // the byte-automaton constraint (rwkv_gen_set_constraint): beside d_gen, one GenDfa per slot; the slot's table lives in a buffer of its own
    GenDfa *d_gen_dfa = nullptr;
    unsigned short *d_tok_end = nullptr;                         // [chunk][V] gen_mask -> gen_post; allocated by the first constraint
    uint8_t tok_single[256] = {};                                // the token table holds the single-byte token c (the liveness rule)
    void gen_set_constraint(int slot, const rwkv_dfa *dfa, int state, int halt_mode);
    int gen_constraint_state(int slot);
    // the stack-automaton constraint (rwkv_gen_set_pda): beside d_gen_dfa, one GenPda per slot; a slot holds a DFA or a stack constraint, never both
    GenPda *d_gen_pda = nullptr;
    void gen_set_pda(int slot, const rwkv_pda *pda, int state, const uint16_t *stack, int depth, int halt_mode);
    void gen_pda_config(int slot, int32_t *state, uint16_t *stack, size_t cap, int32_t *depth);
    // what both kinds share: the refusals, the table's upload into one buffer, the slot's entry, the swap (`fill`: the caller's own part)
    struct Plane { const void *src; size_t bytes; };
    template <class Entry, class Fill>
    void gen_install(int slot, GenConstraint kind, bool present, Entry *d_entries, Fill fill);
    void gen_drop_table(GenSlotHost &s) { if (s.table) { (void)hipFree(s.table); s.table = nullptr; } }   // behind a stream synchronise only
    float *d_gen_pen = nullptr, *d_gen_bias = nullptr, *d_gen_prob = nullptr;
    float **d_gen_shadow = nullptr;
    SampleRow *d_gen_rows = nullptr;
    int *d_gen_tok = nullptr, *d_gen_runstep = nullptr;
    int *d_gen_held = nullptr;                                   // [max_batch] the token a running slot consumes next (its last emitted one)
    unsigned *d_gen_out = nullptr, *h_gen_out = nullptr;         // [2][GEN_RING_STEPS][max_batch]: tokens, then probabilities
    // top-n lists of the raw rows (rwkv_gen_set_topn / rwkv_gen_run_topn): everything below is allocated by the first rwkv_gen_set_topn
    int *d_gen_topn_n = nullptr;                                 // [max_batch] GenSlotHost::topn, for gen_topn_kernel; assigned last: marks the block as complete
    unsigned *d_gen_top_ids = nullptr, *h_gen_top_ids = nullptr; // [GEN_RING_STEPS][max_batch][TOPN_MAX]
    float *d_gen_top_logp = nullptr, *h_gen_top_logp = nullptr;  // the same shape
    float *d_gen_tok_logp = nullptr, *h_gen_tok_logp = nullptr;  // [GEN_RING_STEPS][max_batch]
    float *d_gen_side_ms = nullptr, *d_gen_side_rows = nullptr;  // [max_batch][2], [max_batch][V]: the top-n kernel -> gen_post
    void gen_set_topn(int slot, int n);
    GraphCacheOf<std::vector<uint64_t>> gen_graphs{64, {}};      // one captured step per set of rows (slot mask + sampler kernels it needs)
    // the watch (rwkv_gen_watch_*, gen_watch.h): at most one.  Captured steps hold the ADDRESS of d_gen_watch, never the ring's: open
    // rewrites the descriptor, so a step captured under one watch publishes into the next; steps captured with no watch open do not
    // launch gen_publish at all (bit 36 of their key is clear) and stay what they were
    rwkv_gen_watch *gen_watch = nullptr;
    GenWatchDev *d_gen_watch = nullptr;                          // allocated by the first rwkv_gen_watch_open
    void gen_watch_open(int ring_steps, rwkv_gen_watch **out);
    void gen_watch_close(rwkv_gen_watch *w);
    bool gen_cancel_set(int slot) const { return gen_watch && __atomic_load_n(gen_watch->cancel() + slot, __ATOMIC_ACQUIRE) != 0; }
    void gen_cancel_clear(int slot) { if (gen_watch) __atomic_store_n(gen_watch->cancel() + slot, 0u, __ATOMIC_RELEASE); }
    // captures and items (rwkv_gen_set_capture / _take_item / _arm_item): beside d_gen, one GenCap per slot; a step launches the capture
    // kernel only when one of its slots captures (FEAT_CAPTURE)
    GenCap *d_gen_cap = nullptr;
    rwkv_gen_item *gen_item_new() const;
    bool gen_item_fits(const rwkv_gen_item *it) const {
        return it && it->st.device == device && it->version == info.version && it->L == info.num_layer && it->C == info.num_emb &&
               it->V == info.num_vocab && it->nsx == sx_slot_stride && it->nw == wkv_slot_stride;
    }
    void gen_cap_upload(int slot);
    void gen_set_capture(int slot, unsigned what);
    rwkv_gen_item *gen_take_item(int slot, unsigned which);
    void gen_arm_item(int slot, const rwkv_gen_item *it, const rwkv_gen_params &p);
    void gen_init();
    void gen_arm(int slot, const rwkv_gen_params &p, const uint32_t *prompt, size_t n_prompt, bool from_item = false);
    void gen_disarm_slot(int slot) {                             // callable on an engine that never generated (rwkv_state_load / _write)
        gen_cancel_clear(slot);
        if (!gen_slots.empty()) gen_slots[(size_t)slot].reset_request();
    }
    bool gen_is_armed(int slot) const { return !gen_slots.empty() && gen_slots[(size_t)slot].armed; }
    bool gen_is_live(int slot) const { return gen_is_armed(slot) && !gen_slots[(size_t)slot].g.finish; }   // armed and unfinished
    size_t gen_prompt_left(int slot) const { return gen_slots.empty() ? 0 : gen_slots[(size_t)slot].prompt_left(); }
    GenArgs gen_args(int n_rows, uint64_t feats) const;
    unsigned gen_needs(const std::vector<int> &slots) const { unsigned k = 0; for (int b : slots) k |= sampler_need(gen_slots[(size_t)b].g.kind, gen_slots[(size_t)b].g.wide != 0); return k; }
    // the FEAT_* word of a step over these slots' rows: what each slot adds, and the open watch
    uint64_t gen_feats(const std::vector<int> &slots) const { uint64_t f = gen_watch ? FEAT_WATCH : 0; for (int b : slots) f |= gen_slots[(size_t)b].feats(); return f; }
    void gen_sample(const GenArgs &a, unsigned needs);
    void gen_step(const StepPlan &pl, unsigned needs, uint64_t feats);
    void gen_decode_steps(const std::vector<int> &rows, int n);
    void gen_mixed_step(const std::vector<int> &dec, const std::vector<int> &pro, const std::vector<int> &inj, std::vector<int> &remain);
    void gen_run(int n_steps, uint32_t *out_tokens, float *out_probs, int32_t *n_emitted, int32_t *finish, int n_top = 0,
                 float *out_tok_logp = nullptr, uint32_t *out_top_ids = nullptr, float *out_top_logp = nullptr);
    Knobs kn;                                                    // experiment switches, frozen at creation (rwkv_kernels.h)

    template <class T>
    T *dalloc(size_t n) {
        void *p = nullptr;
        HIP_CHECK(hipMalloc(&p, std::max<size_t>(n * sizeof(T), 16)));
        allocs.push_back(p);
        return (T *)p;
    }
    template <class T>
    T *hostalloc(size_t n, unsigned flags = hipHostMallocDefault) {   // pinned; freed by the destructor like dalloc's
        void *p = nullptr;
        HIP_CHECK(hipHostMalloc(&p, n * sizeof(T), flags));
        host_allocs.push_back(p);
        return (T *)p;
    }
    Opd alloc_opd(int ld) {
        Opd o;
        ld = (ld + 31) / 32 * 32;                                      // whole k-tiles
        o.ld = ld;
        const size_t cap = (size_t)((chunk + 15) / 16 * 16) * ld;      // whole (16 token x 32 k) tiles
        o.hi = dalloc<_Float16>(cap);
        o.lo = (hilo || promote) ? dalloc<_Float16>(cap) : nullptr;
        HIP_CHECK(hipMemset(o.hi, 0, cap * 2));                        // lanes of a partly filled token tile are read (never used)
        if (o.lo) HIP_CHECK(hipMemset(o.lo, 0, cap * 2));
        return o;
    }
    ~rwkv_engine() {
        (void)hipSetDevice(device);
        if (s_main) (void)hipStreamSynchronize(s_main);
        if (s_soft) (void)hipStreamSynchronize(s_soft);
        if (s_copy) (void)hipStreamSynchronize(s_copy);
        graphs.clear(); gen_graphs.clear(); greedy_graphs.reset();   // while the streams they were captured on still exist
        if (gen_watch) { (void)hipHostFree(gen_watch->ring); delete gen_watch; gen_watch = nullptr; }   // the destructor closes an open watch
        for (auto ev : prof_ev) (void)hipEventDestroy(ev);
        for (void *p : allocs) (void)hipFree(p);
        for (GenSlotHost &s : gen_slots) { gen_drop_table(s); s.drop_items(); }
        if (d_tok_end) (void)hipFree(d_tok_end);
        if (d_tok_off) (void)hipFree(d_tok_off);
        if (d_tok_bytes) (void)hipFree(d_tok_bytes);
        for (void *p : host_allocs) (void)hipHostFree(p);
        for (auto ev : meta_ev) if (ev) (void)hipEventDestroy(ev);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (s_main) (void)hipStreamDestroy(s_main);
        if (s_soft) (void)hipStreamDestroy(s_soft);
        if (s_copy) (void)hipStreamDestroy(s_copy);
        if (launch_log) std::fclose(launch_log);
        if (ev_copy_a) (void)hipEventDestroy(ev_copy_a);
        if (ev_copy_b) (void)hipEventDestroy(ev_copy_b);
        if (emb_stage) (void)hipFree(emb_stage);
    }

    // ---- launch wrapper: optional per-family hipEvent timing on the compute stream.  Event pairs are recorded
    // around every launch WITHOUT host synchronisation (the stream stays busy like in the captured step); the
    // elapsed times are read back once the step has drained (prof_collect).
    std::vector<hipEvent_t> prof_ev;
    std::vector<int> prof_fam;
    template <class F>
    void launch(int fam, F &&f) {
        if (profiling) {
            const size_t i = prof_fam.size();
            if (prof_ev.size() < 2 * (i + 1)) {
                hipEvent_t a, b;
                HIP_CHECK(hipEventCreate(&a));
                HIP_CHECK(hipEventCreate(&b));
                prof_ev.push_back(a);
                prof_ev.push_back(b);
            }
            HIP_CHECK(hipEventRecord(prof_ev[2 * i], s_main));
            f();
            HIP_CHECK(hipEventRecord(prof_ev[2 * i + 1], s_main));
            prof_fam.push_back(fam);
        } else {
            f();
        }
    }
    void prof_collect() {
        HIP_CHECK(hipStreamSynchronize(s_main));
        for (size_t i = 0; i < prof_fam.size(); ++i) {
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, prof_ev[2 * i], prof_ev[2 * i + 1]));
            prof_ms[prof_fam[i]] += ms;
            prof_n[prof_fam[i]] += 1;
        }
        prof_fam.clear();
    }

    void load(const rwkv_load_desc &d);
    int gemm(std::vector<ProbSpec> &ps, int T, int fam, const ShiftCommit *commit = nullptr, int cls = CLS_NONE);
    void log_gemm(const std::vector<ProbSpec> &ps, int T, int fam, const char *kind, int variant, int grid, int ksplit, int threads);
    void log_row(const char *kernel, int T, long grid, double bytes);   // RWKV_LAUNCH_LOG: algorithmic bytes of a non-GEMM launch of layer 0 / 1
    int step_max_rows = 0;                                // most rows any sequence has in the step being enqueued (run_plan)
    float *lnp_xx_att = nullptr;                          // normalised rows published by the V6 mix's LN-prologue launch (for the commit)
    void plan_step(const rwkv_slot_input *in, StepPlan &pl, int reserve = 0);   // reserve: rows of the chunk that are spoken for (gen_mixed_step)
    void upload_plan(const StepPlan &pl, const std::vector<int> &pseudo = {});
    void run_layers(int T, int n_seq, int n_out, const int *d_token, bool dense);
    void infer(const rwkv_slot_input *in, rwkv_slot_output *out);
    void run_plan(const StepPlan &pl);
    void infer_sample(const rwkv_slot_input *in, const rwkv_sample_params *sp, uint32_t *out_tokens, float *out_probs,
                      uint8_t *emitted, size_t *n_consumed);
    void infer_score(const rwkv_slot_input *in, const uint32_t *const *targets, float *const *out_logp, size_t *n_consumed);
    void infer_topn(const rwkv_slot_input *in, int n, uint32_t *const *out_ids, float *const *out_logp, const uint32_t *const *targets,
                    float *const *out_tok_logp, size_t *n_rows, size_t *n_consumed);
    // the input of a step in which each of `slots` feeds one token and asks for its row (`Last`); tokens[i] belongs to slots[i], and steps whose
    // ids come from the device (the feedback buffer, held tokens) pass nullptr: the plan then carries a zero nobody reads
    std::vector<rwkv_slot_input> one_token_each(const std::vector<int> &slots, const uint32_t *tokens) const {
        static const uint32_t none = 0;
        std::vector<rwkv_slot_input> in((size_t)max_batch, rwkv_slot_input{nullptr, 0, RWKV_OPTION_LAST, 0});
        for (size_t i = 0; i < slots.size(); ++i) in[(size_t)slots[i]] = rwkv_slot_input{tokens ? tokens + i : &none, 1, RWKV_OPTION_LAST, 0};
        return in;
    }
};

// ------------------------------------------------------------------------------------------------
// loader
// ------------------------------------------------------------------------------------------------
// the tensor names `LoraBlend::full` matches: blocks.<digits>.<anything>
static bool lora_scope(const std::string &name) {
    if (name.compare(0, 7, "blocks.") != 0) return false;
    size_t i = 7;
    while (i < name.size() && name[i] >= '0' && name[i] <= '9') ++i;
    return i > 7 && i + 1 < name.size() && name[i] == '.';
}

static bool is_quant_target(int version, const std::string &suffix) {
    static const char *att56[] = {"att.receptance.weight", "att.key.weight", "att.value.weight", "att.output.weight", "att.gate.weight"};
    static const char *att7[] = {"att.receptance.weight", "att.key.weight", "att.value.weight", "att.output.weight"};   // V4's as well: no gate
    static const char *ffn56[] = {"ffn.key.weight", "ffn.value.weight", "ffn.receptance.weight"};
    static const char *ffn7[] = {"ffn.key.weight", "ffn.value.weight"};
    if (version == 7) {
        for (auto s : att7) if (suffix == s) return true;
        for (auto s : ffn7) if (suffix == s) return true;
    } else if (version == 4) {
        for (auto s : att7) if (suffix == s) return true;
        for (auto s : ffn56) if (suffix == s) return true;
    } else {
        for (auto s : att56) if (suffix == s) return true;
        for (auto s : ffn56) if (suffix == s) return true;
    }
    return false;
}

void rwkv_engine::save_prefab(const char *path) {
    FILE *f = std::fopen(path, "wb");
    if (!f) throw RwkvError(RWKV_ERR_INVALID, std::string("cannot open ") + path);
    struct Closer { FILE *f; ~Closer() { std::fclose(f); } } closer{f};
    auto put = [&](const void *p, size_t n) { if (n && std::fwrite(p, 1, n, f) != n) throw RwkvError(RWKV_ERR_INVALID, "short write"); };
    size_t pos = 0;
    auto putp = [&](const void *p, size_t n) {                 // payload + pad to 16
        static const char zeros[16] = {0};
        put(p, n);
        pos += n;
        const size_t padn = ((pos + 15) & ~(size_t)15) - pos;
        put(zeros, padn);
        pos += padn;
    };
    PfHeader h{};
    std::memcpy(h.magic, kPrefabMagic, 8);
    h.version = kPrefabVersion;
    h.n_entries = (uint32_t)(vecs.size() + raws.size() + mats.size());
    h.info = info; h.quant_layers = quant_layers; h.quant_type = quant_type;
    put(&h, sizeof(h));
    pos = sizeof(h);
    std::vector<uint8_t> host;
    auto entry = [&](const std::string &name, uint32_t kind, int fmt, int rows, int K, bool counted, uint64_t n_elems,
                     const void *dev_data, size_t data_bytes, const void *dev_scales, size_t scale_bytes) {
        PfEntryHead e{};
        e.kind = kind; e.fmt = fmt; e.rows = rows; e.K = K; e.counted = counted ? 1 : 0; e.name_len = (uint32_t)name.size();
        e.n_elems = n_elems; e.data_bytes = data_bytes; e.scale_bytes = scale_bytes;
        put(&e, sizeof(e));
        pos += sizeof(e);
        putp(name.data(), name.size());
        host.resize(std::max(data_bytes, scale_bytes));
        HIP_CHECK(hipMemcpy(host.data(), dev_data, data_bytes, hipMemcpyDeviceToHost));
        putp(host.data(), data_bytes);
        if (scale_bytes) {
            HIP_CHECK(hipMemcpy(host.data(), dev_scales, scale_bytes, hipMemcpyDeviceToHost));
            putp(host.data(), scale_bytes);
        }
    };
    HIP_CHECK(hipSetDevice(device));
    for (auto &kv : vecs) entry(kv.first, 0, 0, 0, 0, true, vec_meta.at(kv.first).first, kv.second, vec_meta.at(kv.first).first * 4, nullptr, 0);
    for (auto &kv : raws) entry(kv.first, 1, 0, 0, 0, raw_meta.at(kv.first).second, raw_meta.at(kv.first).first, kv.second, raw_meta.at(kv.first).first * 2, nullptr, 0);
    for (auto &kv : mats) {
        const DMat &m = kv.second;
        const size_t db = m.fmt == W_F16 ? (size_t)m.rows * m.K * 2 : m.fmt == W_INT8 ? (size_t)m.rows * m.K : (size_t)m.rows * m.K / 2;
        const size_t sb = m.fmt == W_F16 ? 0 : m.fmt == W_INT8 ? (size_t)m.rows * (m.K / 128) * 4 : (size_t)m.rows * (m.K / 64) * 2;
        entry(kv.first, 2, m.fmt, m.rows, m.K, true, m.bytes, m.data, db, m.scales, sb);
    }
}

void rwkv_engine::load(const rwkv_load_desc &d) {
    if (const char *lp = std::getenv("RWKV_LAUNCH_LOG")) if (*lp) launch_log = std::fopen(lp, "a");
    const bool pf = prefab_sniff(d.st_bytes, d.st_len);      // lib.rs:585-588: the file is sniffed, not named
    Prefab prefab;
    SafeTensors st;
    if (pf) { prefab = Prefab::parse(d.st_bytes, d.st_len); info = prefab.hdr.info; }
    else { st = SafeTensors::parse(d.st_bytes, d.st_len); info = detect_info(st); }
    const int L = info.num_layer, C = info.num_emb, F = info.num_hidden, V = info.num_vocab, H = info.num_head;
    max_batch = d.max_batch > 0 ? d.max_batch : 8;
    chunk = d.token_chunk_size > 0 ? d.token_chunk_size : 128;
    kn = Knobs::from_env();                                  // frozen for the engine's lifetime (and for every graph it captures)
    use_knobs(kn);
    if (d.precision != RWKV_PRECISION_FP16 && d.precision != RWKV_PRECISION_FP32 && d.precision != RWKV_PRECISION_FP16_RAW)
        throw RwkvError(RWKV_ERR_INVALID, "precision must be RWKV_PRECISION_FP16, _FP32 or _FP16_RAW");
    hilo = d.precision == RWKV_PRECISION_FP32;
    promote = hilo ? 0 : (d.precision == RWKV_PRECISION_FP16 ? promote_for_version(info.version) : 0);
    if (!hilo && kn.promote >= 0) promote = kn.promote & 63;   // dev override (A/B runs, the error-attribution experiments)
    quant_layers = std::max(0, std::min(d.quant_layers, L));
    quant_type = d.quant_type;
    if (pf) {                                                // a prefab is already quantised / blended: its settings win
        quant_layers = prefab.hdr.quant_layers; quant_type = prefab.hdr.quant_type;
        if (d.n_lora) throw RwkvError(RWKV_ERR_UNSUPPORTED, "LoRA adapters cannot be applied to a prefab image");
    }
    if (quant_type != RWKV_QUANT_NONE && quant_type != RWKV_QUANT_INT8 && quant_type != RWKV_QUANT_NF4 && quant_type != RWKV_QUANT_SF4)
        throw RwkvError(RWKV_ERR_UNSUPPORTED, "quant_type must be None, Int8, NF4 or SF4");
    if (quant_type != RWKV_QUANT_NONE && quant_layers > 0 && (C % 256 || F % 256))
        throw RwkvError(RWKV_ERR_UNSUPPORTED, "quantisation needs num_emb and num_hidden to be multiples of 256");

    HIP_CHECK(hipStreamCreateWithFlags(&s_main, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&s_soft, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreate(&ev0));
    HIP_CHECK(hipEventCreate(&ev1));

    // LoRA adapters parsed once (LoraBlend::full(alpha), lib.rs:466-482): W += alpha * B * A^T for every
    // matrix that has `<name minus .weight>.lora.0` ([in, r], transposed on conversion) and `.lora.1` ([out, r]).
    std::vector<std::pair<SafeTensors, float>> loras;
    for (size_t i = 0; i < d.n_lora; ++i)
        loras.emplace_back(SafeTensors::parse(d.lora[i].st_bytes, d.lora[i].st_len), d.lora[i].alpha);

    size_t raw_cap = 0;
    if (!pf) for (auto &kv : st.tensors) raw_cap = std::max(raw_cap, kv.second.nbytes);
    _Float16 *raw = nullptr;                                   // temp upload buffer
    HIP_CHECK(hipMalloc((void **)&raw, std::max<size_t>(raw_cap, 16)));
    struct RawGuard { void *p; ~RawGuard() { (void)hipFree(p); } } rg{raw};
    _Float16 *lbuf = nullptr;
    size_t lbuf_cap = 0;
    struct LGuard { _Float16 **p; ~LGuard() { if (*p) (void)hipFree(*p); } } lg{&lbuf};

    auto upload_raw = [&](const StTensor &t) {
        if (t.dtype != "F16") throw RwkvError(RWKV_ERR_UNSUPPORTED, "tensor dtype must be F16 (convert_safetensors.py:64)");
        HIP_CHECK(hipMemcpyAsync(raw, t.data, t.nbytes, hipMemcpyHostToDevice, s_main));
    };
    // `want` = the element count the kernels will read (0: unchecked): a short tensor must fail the load, not a kernel
    auto load_vec = [&](const std::string &name, int op = 0, size_t want = 0) -> const float * {
        if (pf) {
            const PfEntry &e = prefab.get(name, 0);
            if (want && e.h.n_elems != want) throw RwkvError(RWKV_ERR_FORMAT, name + ": unexpected size");
            float *v = dalloc<float>((size_t)e.h.n_elems);
            HIP_CHECK(hipMemcpy(v, e.data, e.h.n_elems * 4, hipMemcpyHostToDevice));
            vecs[name] = v; vec_meta[name] = {(size_t)e.h.n_elems, true};
            weight_bytes += (uint64_t)e.h.n_elems * 2;
            return v;
        }
        const StTensor &t = st.get(name);
        if (want && (size_t)t.numel() != want) throw RwkvError(RWKV_ERR_FORMAT, name + ": unexpected size");
        upload_raw(t);
        float *v = dalloc<float>((size_t)t.numel());
        // `LoraBlend::full(alpha)` (lib.rs:466-482).  web-rwkv is not vendored in the reference tree; restated from its loader
        // (runtime/loader.rs, 0.10.x) and UNPINNED: `full` is the single pattern `blocks\.([0-9]+)\.([0-9a-zA-Z\.\_]+)`, so only
        // per-block tensors blend (emb, head, ln_out do not; blocks.0.ln0 does), and a VECTOR the LoRA file holds under the model's
        // own name (time_mix_*, time_decay, time_first, LayerNorm weights ...: fine-tuned whole, not low-rank) is blended
        // v = alpha * l + (1 - alpha) * v — `factor = [alpha, 1 - alpha]` of its `load_vector_*`; alpha = 1 replaces it —
        // in fp32 before the load-time transform.  Matrices: W += alpha * B A^T (`factor = [alpha, 1]`), load_mat below.
        bool blended = false;
        for (auto &lp : loras) {
            const StTensor *l = lora_scope(name) ? lp.first.find(name) : nullptr;
            if (!l) continue;
            if (l->dtype != "F16" || l->numel() != t.numel()) throw RwkvError(RWKV_ERR_FORMAT, name + ": LoRA tensor does not match the model's");
            if (!blended) { launch_f16_to_f32(raw, v, t.numel(), 0, s_main); blended = true; }
            HIP_CHECK(hipStreamSynchronize(s_main));                                // `raw` is free again
            HIP_CHECK(hipMemcpyAsync(raw, l->data, l->nbytes, hipMemcpyHostToDevice, s_main));
            launch_vec_blend(v, raw, t.numel(), lp.second, s_main);
        }
        if (blended) { if (op) launch_vec_op(v, t.numel(), op, s_main); }
        else launch_f16_to_f32(raw, v, t.numel(), op, s_main);
        HIP_CHECK(hipStreamSynchronize(s_main));
        vecs[name] = v; vec_meta[name] = {(size_t)t.numel(), true};
        weight_bytes += (uint64_t)t.numel() * 2;
        return v;
    };
    auto load_raw16 = [&](const std::string &name, bool count, size_t want = 0) -> const _Float16 * {
        if (pf) {
            const PfEntry &e = prefab.get(name, 1);
            if (want && e.h.n_elems != want) throw RwkvError(RWKV_ERR_FORMAT, name + ": unexpected size");
            _Float16 *v = dalloc<_Float16>((size_t)e.h.n_elems);
            HIP_CHECK(hipMemcpy(v, e.data, e.h.n_elems * 2, hipMemcpyHostToDevice));
            raws[name] = v; raw_meta[name] = {(size_t)e.h.n_elems, count};
            if (count) weight_bytes += (uint64_t)e.h.n_elems * 2;
            return v;
        }
        const StTensor &t = st.get(name);
        if (t.dtype != "F16") throw RwkvError(RWKV_ERR_UNSUPPORTED, "tensor dtype must be F16");
        if (want && (size_t)t.numel() != want) throw RwkvError(RWKV_ERR_FORMAT, name + ": unexpected size");
        _Float16 *v = dalloc<_Float16>((size_t)t.numel());
        HIP_CHECK(hipMemcpy(v, t.data, t.nbytes, hipMemcpyHostToDevice));
        raws[name] = v; raw_meta[name] = {(size_t)t.numel(), count};
        if (count) weight_bytes += (uint64_t)t.nbytes;
        return v;
    };
    // matrix [.., rows, K] (leading dims folded into `index`)
    // want_rows / want_K: the shape the forward pass assumes (0: taken from the tensor, e.g. LoRA ranks); rows are checked
    // after padding to whole 16-row strips
    auto load_mat = [&](const std::string &name, int fmt, int index = -1, const std::string &key = "", int want_rows = 0, int want_K = 0) -> const DMat * {
        auto check_shape = [&](int rows16, int K) {
            if ((want_rows && rows16 != (want_rows + 15) / 16 * 16) || (want_K && K != want_K))
                throw RwkvError(RWKV_ERR_FORMAT, name + ": unexpected matrix shape");
        };
        if (pf) {
            const std::string &k = key.empty() ? name : key;
            const PfEntry &e = prefab.get(k, 2);
            check_shape(e.h.rows, e.h.K);
            if (e.h.fmt != fmt) throw RwkvError(RWKV_ERR_FORMAT, name + ": stored format differs from the image header's quantisation");
            DMat m;
            m.fmt = e.h.fmt; m.rows = e.h.rows; m.K = e.h.K; m.bytes = e.h.n_elems;
            void *p = dalloc<uint8_t>((size_t)e.h.data_bytes);
            HIP_CHECK(hipMemcpy(p, e.data, e.h.data_bytes, hipMemcpyHostToDevice));
            m.data = p;
            if (e.h.scale_bytes) {
                void *sc = dalloc<uint8_t>((size_t)e.h.scale_bytes);
                HIP_CHECK(hipMemcpy(sc, e.scales, e.h.scale_bytes, hipMemcpyHostToDevice));
                m.scales = sc;
            }
            weight_bytes += m.bytes;
            return &mats.emplace(k, m).first->second;
        }
        const StTensor &t = st.get(name);
        if (t.shape.size() < 2) throw RwkvError(RWKV_ERR_FORMAT, name + ": expected a matrix");
        if (t.shape.back() <= 0 || t.shape.back() > (1 << 24) || t.shape[t.shape.size() - 2] <= 0 || t.shape[t.shape.size() - 2] > (1 << 24))
            throw RwkvError(RWKV_ERR_FORMAT, name + ": unexpected matrix shape");
        const int K = (int)t.shape.back(), rows = (int)t.shape[t.shape.size() - 2];
        check_shape((rows + 15) / 16 * 16, K);
        {
            size_t lead = 1;
            for (size_t i = 0; i + 2 < t.shape.size(); ++i) lead *= (size_t)t.shape[i];
            if (index >= 0 ? (size_t)index >= lead : lead != 1) throw RwkvError(RWKV_ERR_FORMAT, name + ": unexpected leading dimensions");
        }
        upload_raw(t);
        const _Float16 *src = raw + (index >= 0 ? (size_t)index * rows * K : 0);
        if (index < 0) {
            // LoRA blend on the raw fp16 matrix (fp32 math, one rounding back to fp16)
            const std::string stem = name.size() > 7 && name.substr(name.size() - 7) == ".weight" ? name.substr(0, name.size() - 7) : name;
            for (auto &lp : loras) {
                if (!lora_scope(name)) break;                                   // LoraBlend::full matches `blocks.N.*` only (see load_vec)
                const StTensor *A = lp.first.find(stem + ".lora.0"), *B = lp.first.find(stem + ".lora.1");
                if (!A || !B) continue;
                if (A->shape.size() != 2 || B->shape.size() != 2 || A->shape[0] != K || B->shape[0] != rows || A->shape[1] != B->shape[1])
                    throw RwkvError(RWKV_ERR_FORMAT, "LoRA shape mismatch for " + stem);
                const int r = (int)A->shape[1];
                size_t need = (size_t)(K + rows) * r * 2;
                if (need > lbuf_cap) {
                    if (lbuf) (void)hipFree(lbuf);
                    lbuf = nullptr;
                    HIP_CHECK(hipMalloc((void **)&lbuf, need));
                    lbuf_cap = need;
                }
                HIP_CHECK(hipMemcpyAsync(lbuf, A->data, A->nbytes, hipMemcpyHostToDevice, s_main));
                HIP_CHECK(hipMemcpyAsync(lbuf + (size_t)K * r, B->data, B->nbytes, hipMemcpyHostToDevice, s_main));
                launch_lora_blend(raw, lbuf + (size_t)K * r, lbuf, rows, K, r, lp.second, s_main);
            }
        }
        if (K % 32) throw RwkvError(RWKV_ERR_UNSUPPORTED, name + ": inner dim must be a multiple of 32");
        DMat m;
        m.fmt = fmt;
        m.K = K;
        m.rows = (rows + 15) / 16 * 16;
        if (fmt != W_F16 && (K % 256 || rows % 16)) throw RwkvError(RWKV_ERR_UNSUPPORTED, name + ": cannot quantise (dims)");
        if (fmt == W_F16) {
            size_t n = (size_t)m.rows * K * 2;
            void *p = dalloc<uint8_t>(n);
            launch_tile_f16(src, rows, m.rows, K, p, s_main);
            m.data = p;
            m.bytes = (uint64_t)rows * K * 2;
        } else if (fmt == W_INT8) {
            void *p = dalloc<uint8_t>((size_t)m.rows * K);
            void *sc = dalloc<uint8_t>((size_t)m.rows * (K / 128) * 4);
            launch_quant_int8(src, m.rows, K, p, sc, s_main);
            m.data = p; m.scales = sc;
            m.bytes = (uint64_t)m.rows * K + (uint64_t)m.rows * (K / 128) * 4;
        } else {
            void *p = dalloc<uint8_t>((size_t)m.rows * K / 2);
            void *sc = dalloc<uint8_t>((size_t)m.rows * (K / 64) * 2);
            if (fmt == W_SF4) launch_quant_sf4(src, m.rows, K, p, sc, s_main);   // NF4's bytes and sizes, the other code book
            else launch_quant_nf4(src, m.rows, K, p, sc, s_main);
            m.data = p; m.scales = sc;
            m.bytes = (uint64_t)m.rows * K / 2 + (uint64_t)m.rows * (K / 64) * 2;
        }
        HIP_CHECK(hipStreamSynchronize(s_main));
        weight_bytes += m.bytes;
        auto it = mats.emplace(key.empty() ? name : key, m).first;
        return &it->second;
    };

    const size_t nC = (size_t)C;
    emb = load_raw16("emb.weight", false, (size_t)V * C);     // embedding table: only B rows touched per step
    ln0w = load_vec("blocks.0.ln0.weight", 0, nC);
    ln0b = load_vec("blocks.0.ln0.bias", 0, nC);
    lnow = load_vec("ln_out.weight", 0, nC);
    lnob = load_vec("ln_out.bias", 0, nC);
    head = load_mat("head.weight", W_F16, -1, "", V, C);
    if (head->rows != V) throw RwkvError(RWKV_ERR_FORMAT, "head.weight rows != vocab");

    layers.resize(L);
    for (int l = 0; l < L; ++l) {
        LayerW &w = layers[l];
        std::memset(&w, 0, sizeof(w));
        const std::string p = "blocks." + std::to_string(l) + ".";
        const int qf = (quant_type != RWKV_QUANT_NONE && l < quant_layers) ? (quant_type == RWKV_QUANT_INT8 ? W_INT8 : quant_type == RWKV_QUANT_SF4 ? W_SF4 : W_NF4) : W_F16;
        auto qfmt = [&](const char *suffix) { return is_quant_target(info.version, suffix) ? qf : W_F16; };
        // every vector is [C] (time_decay / time_first / r_k are [H, 64]); every matrix is checked against the shape the
        // forward pass assumes, so a truncated or inconsistent checkpoint fails here with RWKV_ERR_FORMAT
        w.ln1w = load_vec(p + "ln1.weight", 0, nC); w.ln1b = load_vec(p + "ln1.bias", 0, nC);
        w.ln2w = load_vec(p + "ln2.weight", 0, nC); w.ln2b = load_vec(p + "ln2.bias", 0, nC);
        if (info.version != 4) { w.lnxw = load_vec(p + "att.ln_x.weight", 0, nC); w.lnxb = load_vec(p + "att.ln_x.bias", 0, nC); }
        w.Wr = load_mat(p + "att.receptance.weight", qfmt("att.receptance.weight"), -1, "", C, C);
        w.Wk = load_mat(p + "att.key.weight", qfmt("att.key.weight"), -1, "", C, C);
        w.Wv = load_mat(p + "att.value.weight", qfmt("att.value.weight"), -1, "", C, C);
        w.Wo = load_mat(p + "att.output.weight", qfmt("att.output.weight"), -1, "", C, C);
        w.Fk = load_mat(p + "ffn.key.weight", qfmt("ffn.key.weight"), -1, "", F, C);
        w.Fv = load_mat(p + "ffn.value.weight", qfmt("ffn.value.weight"), -1, "", C, F);
        if (info.version != 7) {
            if (info.version != 4) w.Wg = load_mat(p + "att.gate.weight", qfmt("att.gate.weight"), -1, "", C, C);
            w.Fr = load_mat(p + "ffn.receptance.weight", qfmt("ffn.receptance.weight"), -1, "", C, C);
            w.fmu[0] = load_vec(p + "ffn.time_mix_k", 0, nC);
            w.fmu[1] = load_vec(p + "ffn.time_mix_r", 0, nC);
            w.u = load_vec(p + "att.time_first", 0, nC);
        }
        if (info.version == 4) {
            const char *n3[] = {"k", "v", "r"};
            for (int i = 0; i < 3; ++i) w.mu[i] = load_vec(p + "att.time_mix_" + n3[i], 0, nC);
            w.wdec = load_vec(p + "att.time_decay", 2, nC);  // -exp(decay), static per channel
        } else if (info.version == 5) {
            const char *n4[] = {"k", "v", "r", "g"};
            for (int i = 0; i < 4; ++i) w.mu[i] = load_vec(p + "att.time_mix_" + n4[i], 0, nC);
            w.wdec = load_vec(p + "att.time_decay", 1, nC);  // exp(-exp(decay)), static per channel
        } else if (info.version == 6) {
            const char *n6[] = {"x", "w", "k", "v", "r", "g"};
            for (int i = 0; i < 6; ++i) w.mu[i] = load_vec(p + "att.time_mix_" + n6[i], 0, nC);
            w.wdec = load_vec(p + "att.time_decay", 0, nC);
            int dm_l;
            if (!pf) {
                const StTensor &w2 = st.get(p + "att.time_mix_w2");
                if (w2.shape.size() != 3 || w2.shape[0] != 5 || w2.shape[1] != C || w2.shape[2] <= 0 || w2.shape[2] > 4096)
                    throw RwkvError(RWKV_ERR_FORMAT, "time_mix_w2 must be [5,C,Dm]");
                dm_l = (int)w2.shape[2];
            } else {
                dm_l = prefab.get(p + "att.time_mix_w2#0", 2).h.K;
            }
            if (l > 0 && dm_l != Dm) throw RwkvError(RWKV_ERR_FORMAT, "time_mix LoRA dim differs between layers");
            Dm = dm_l;
            w.W1 = load_mat(p + "att.time_mix_w1", W_F16, -1, "", 5 * Dm, C);
            for (int c = 0; c < 5; ++c) w.W2[c] = load_mat(p + "att.time_mix_w2", W_F16, c, p + "att.time_mix_w2#" + std::to_string(c), C, Dm);
            // the decay LoRA rank as the FILE states it (load_mat pads rows to whole strips): the WKV kernels read [T][Dd] / [C][Dd] rows in four
            // parts of whole 8-element vectors (rwkv_kernels.hip wkv_kernel), so the rank must be a multiple of 32, and ftd holds 128 columns
            if (!pf) {
                const StTensor &d1 = st.get(p + "att.time_decay_w1");
                const long dd = d1.shape.size() == 2 ? (long)d1.shape[0] : -1;
                if (dd < 0) throw RwkvError(RWKV_ERR_FORMAT, p + "att.time_decay_w1: expected a matrix");
                if (dd < 32 || dd > 128 || dd % 32)
                    throw RwkvError(RWKV_ERR_UNSUPPORTED, "time_decay LoRA dim must be 32, 64, 96 or 128 (" + p + "att.time_decay_w1 has " + std::to_string(dd) + ")");
            }
            w.D1 = load_mat(p + "att.time_decay_w1", W_F16, -1, "", 0, C);
            if (l > 0 && w.D1->rows != Dd) throw RwkvError(RWKV_ERR_FORMAT, "time_decay LoRA dim differs between layers");
            Dd = w.D1->rows;
            if (Dd > 128 || Dd % 32) throw RwkvError(RWKV_ERR_UNSUPPORTED, "time_decay LoRA dim must be 32, 64, 96 or 128");
            w.D2 = load_raw16(p + "att.time_decay_w2", true, (size_t)C * Dd);
        } else {
            const char *n7[] = {"r", "w", "k", "v", "a", "g"};
            for (int i = 0; i < 6; ++i) w.mu[i] = load_vec(p + "att.x_" + n7[i], 0, nC);
            w.fmu[0] = load_vec(p + "ffn.x_k", 0, nC);
            w.w0 = load_vec(p + "att.w0", 0, nC); w.a0 = load_vec(p + "att.a0", 0, nC);
            w.k_k = load_vec(p + "att.k_k", 0, nC); w.k_a = load_vec(p + "att.k_a", 0, nC); w.r_k = load_vec(p + "att.r_k", 0, nC);
            // LoRA pairs: stage 1 is [D, C] with a free rank D, stage 2 must be [C, D] of the same rank
            auto lora_pair = [&](const char *n1, const char *n2, const DMat *&m1, const DMat *&m2) {
                m1 = load_mat(p + n1, W_F16, -1, "", 0, C);
                m2 = load_mat(p + n2, W_F16, -1, "", C, 0);
                if (m2->K > m1->rows || m2->K % 32) throw RwkvError(RWKV_ERR_FORMAT, p + n2 + ": LoRA rank mismatch");
            };
            lora_pair("att.w1", "att.w2", w.w1, w.w2);
            lora_pair("att.a1", "att.a2", w.a1, w.a2);
            lora_pair("att.g1", "att.g2", w.g1, w.g2);
            if (l > 0 || (pf ? prefab.has(p + "att.v0") : st.find(p + "att.v0") != nullptr)) {
                w.v0 = load_vec(p + "att.v0", 0, nC);
                lora_pair("att.v1", "att.v2", w.v1, w.v2);
            }
            for (const DMat *m : {w.w1, w.a1, w.v1, w.g1}) if (m) Dl = std::max(Dl, m->rows);
        }
    }

    // ---- state + scratch
    sx_slot_stride = (long)L * C;
    wkv_slot_stride = (long)L * wkv_layer_floats();
    sxa = dalloc<float>((size_t)max_batch * sx_slot_stride);
    sxf = dalloc<float>((size_t)max_batch * sx_slot_stride);
    wkv = dalloc<float>((size_t)max_batch * wkv_slot_stride);
    HIP_CHECK(hipMemset(sxa, 0, (size_t)max_batch * sx_slot_stride * 4));
    HIP_CHECK(hipMemset(sxf, 0, (size_t)max_batch * sx_slot_stride * 4));
    HIP_CHECK(hipMemset(wkv, 0, (size_t)max_batch * wkv_slot_stride * 4));
    if (info.version == 4) {                                   // a slot nobody loaded holds the initial state: pp = V4_PP_INIT
        std::vector<float> pp((size_t)C, V4_PP_INIT);
        for (int b = 0; b < max_batch; ++b)
            for (int l = 0; l < L; ++l)
                HIP_CHECK(hipMemcpy(wkv + (size_t)b * wkv_slot_stride + ((size_t)l * 3 + 2) * C, pp.data(), (size_t)C * 4, hipMemcpyHostToDevice));
    }
    const size_t slab = state_len();
    slab_dev = dalloc<float>(slab);
    slab_host = hostalloc<float>(slab);

    const size_t TC = (size_t)chunk * C;
    pstride = (long)TC;
    xA = dalloc<float>(TC); xB = dalloc<float>(TC); P = dalloc<float>(TC * 8);
    xx = dalloc<float>(TC); dx = dalloc<float>(TC);
    lnp_xx_att = dalloc<float>((size_t)LNP_MAX_T * C);
    fr = dalloc<float>(TC); fk = dalloc<float>(TC); fv = dalloc<float>(TC); fg = dalloc<float>(TC); frr = dalloc<float>(TC);
    ftd = dalloc<float>((size_t)chunk * 128);
    if (info.version == 7) {
        fw7 = dalloc<float>(TC); fa7 = dalloc<float>(TC); fvg7 = dalloc<float>(TC); vfirst = dalloc<float>(TC);
    }
    for (auto &o : opA) o = alloc_opd(C);
    opY = alloc_opd(C);
    opO = alloc_opd(C);
    opK = alloc_opd(F);
    opM = alloc_opd(std::max(16, info.version == 6 ? 5 * Dm : 16));
    for (auto &o : opL) o = alloc_opd(std::max(16, Dl));
    logits = dalloc<float>((size_t)chunk * V);
    logits_host = hostalloc<float>((size_t)chunk * V);
    meta_cap = MetaView::words(chunk, max_batch);
    d_meta = dalloc<int>(meta_cap);
    dm = MetaView(d_meta, chunk, max_batch);
    h_meta = hostalloc<int>(meta_cap * META_RING);
    for (auto &ev : meta_ev) HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    h_tok = hostalloc<int>((size_t)max_batch, hipHostMallocMapped | hipHostMallocCoherent);   // uncached on the device: always the host's latest store
    HIP_CHECK(hipHostGetDevicePointer((void **)&dv_tok, h_tok, 0));
    d_tok_feedback = dalloc<int>(chunk);
    soft_rows_cap = (size_t)std::max(1, max_batch);
    soft_in = dalloc<float>(soft_rows_cap * V);
    soft_out = dalloc<float>(soft_rows_cap * V);
    soft_host = hostalloc<float>(soft_rows_cap * V);
    d_score_tgt = dalloc<unsigned>(chunk); d_score_out = dalloc<float>(chunk);
    h_score_tgt = hostalloc<unsigned>(chunk); h_score_out = hostalloc<float>(chunk);
    d_soft_tgt = dalloc<unsigned>(soft_rows_cap); d_soft_score = dalloc<float>(soft_rows_cap);
    h_soft_tgt = hostalloc<unsigned>(soft_rows_cap); h_soft_score = hostalloc<float>(soft_rows_cap);
    d_topn_ids = dalloc<unsigned>((size_t)chunk * TOPN_MAX); d_topn_logp = dalloc<float>((size_t)chunk * TOPN_MAX);
    h_topn_ids = hostalloc<unsigned>((size_t)chunk * TOPN_MAX); h_topn_logp = hostalloc<float>((size_t)chunk * TOPN_MAX);
    d_soft_topn_ids = dalloc<unsigned>(soft_rows_cap * TOPN_MAX); d_soft_topn_logp = dalloc<float>(soft_rows_cap * TOPN_MAX);
    h_soft_topn_ids = hostalloc<unsigned>(soft_rows_cap * TOPN_MAX); h_soft_topn_logp = hostalloc<float>(soft_rows_cap * TOPN_MAX);
    d_adj_row = dalloc<int>(ADJ_CAP); d_adj_tok = dalloc<int>(ADJ_CAP); d_adj_val = dalloc<float>(ADJ_CAP);
    d_allow = dalloc<unsigned char>((size_t)max_batch * V); d_allow_row = dalloc<int>(max_batch);
    h_allow = hostalloc<unsigned char>((size_t)max_batch * V + (size_t)max_batch * 4 + 16);
    // the sampling block: the offsets that place its sections also size it (the last section's end)
    const size_t o_adj = (size_t)chunk * sizeof(SampleRow), o_out = o_adj + ADJ_CAP * 12, samp_bytes = o_out + (size_t)chunk * 8;
    unsigned char *h_samp = hostalloc<unsigned char>(samp_bytes);
    unsigned char *dv_samp = nullptr;
    HIP_CHECK(hipHostGetDevicePointer((void **)&dv_samp, h_samp, 0));
    int *adj = (int *)(h_samp + o_adj), *out = (int *)(h_samp + o_out), *dv_out = (int *)(dv_samp + o_out);
    samp = SampStage{(SampleRow *)h_samp, adj, adj + ADJ_CAP, (float *)(adj + 2 * ADJ_CAP), out, (float *)(out + chunk),
                     (const SampleRow *)dv_samp, dv_out, (float *)(dv_out + chunk)};
    greedy_graphs.emplace((size_t)max_batch, GraphExecDeleter{});
    d_amax_v = dalloc<float>((size_t)chunk * 32);
    d_amax_i = dalloc<int>((size_t)chunk * 32);
    HIP_CHECK(hipDeviceSynchronize());
}

// ------------------------------------------------------------------------------------------------
// GEMM launch: gemm_plan.h decides (path, tile shape, K split, block geometry); this logs and launches
// ------------------------------------------------------------------------------------------------
int rwkv_engine::gemm(std::vector<ProbSpec> &ps, int T, int fam, const ShiftCommit *commit, int cls) {
    const bool hilo = wide(cls);                                 // shadows the engine-wide flag: this launch's operand width
    if (hilo) for (auto &sp : ps) if (!sp.x.lo) throw RwkvError(RWKV_ERR_INVALID, "gemm: a hi + lo launch needs the lo part of every operand");
    if (ps.empty() || ps.size() > GEMM_MAXP) throw RwkvError(RWKV_ERR_INVALID, "gemm: bad problem count");
    const int n = (int)ps.size();
    ProbShape sh[GEMM_MAXP];
    for (int i = 0; i < n; ++i) sh[i] = shape_of(ps[i]);
    GemmLaunch Lh;
    const GemmPlan pl = plan_gemm(Lh, sh, n, T, hilo, commit && commit->src, kn);
    if (!pl.ksplit) throw RwkvError(RWKV_ERR_UNSUPPORTED, "cannot split inner dimension");
    for (int i = 0; i < n; ++i) fill_prob(Lh.p[i], ps[i], pstride);
    if (pl.path == GEMM_DECODE && commit) Lh.commit = *commit;
    log_gemm(ps, T, fam, kGemmPathNames[pl.path], pl.variant, pl.grid, pl.ksplit, pl.threads);
    if (pl.path == GEMM_SMALLK) launch(fam, [&] { launch_smallk(Lh, hilo, s_main); });
    else if (pl.path == GEMM_TILE) launch(fam, [&] { launch_gemm_tile(Lh, pl.variant, hilo, s_main); });
    else launch(fam, [&] { launch_gemm(Lh, hilo, s_main); });
    return pl.ksplit;
}

// RWKV_LAUNCH_LOG (dev): what a launch of layer 0 (or the head) streams and computes, so that a profile can be priced without guessing which
// grid size is which launch: {"kind","variant","T","grid","ksplit","rows","bytes","flops","mats"}
void rwkv_engine::log_row(const char *kernel, int T, long grid, double bytes) {
    if (!launch_log || cur_layer > 1) return;
    std::fprintf(launch_log, "{\"kind\": \"row\", \"kernel\": \"%s\", \"T\": %d, \"grid\": %ld, \"bytes\": %.0f}\n", kernel, T, grid, bytes);
    std::fflush(launch_log);
}
void rwkv_engine::log_gemm(const std::vector<ProbSpec> &ps, int T, int fam, const char *kind, int variant, int grid, int ksplit, int threads) {
    if (!launch_log || (cur_layer > 1 && fam != FAM_HEAD)) return;       // layers 0 and 1 (V7's layer 0 has no value-residual LoRA) + the head
    uint64_t bytes = 0;
    double flops = 0;
    long rows = 0;
    std::string names;
    for (auto &sp : ps) {
        bytes += sp.W->bytes;
        rows += sp.W->rows;
        flops += 2.0 * T * (double)sp.W->rows * sp.W->K;
        for (auto &kv : mats)
            if (&kv.second == sp.W) { names += (names.empty() ? "" : "+") + kv.first; break; }
    }
    std::fprintf(launch_log, "{\"kind\": \"%s\", \"variant\": %d, \"T\": %d, \"grid\": %d, \"threads\": %d, \"ksplit\": %d, \"rows\": %ld, \"bytes\": %llu, \"flops\": %.0f, \"mats\": \"%s\"}\n",
                 kind, variant, T, grid, threads, ksplit, rows, (unsigned long long)bytes, flops, names.c_str());
    std::fflush(launch_log);
}

// ------------------------------------------------------------------------------------------------
// step planning (RnnInput::new(batches, token_chunk_size), run.rs:1132) — which tokens ride this call
// ------------------------------------------------------------------------------------------------
// water-filling of the chunk budget across slots with pending tokens: short (decode) requests are never starved by
// a long prefill (any split is result-equivalent: slots are independent, RNN chunking is exact)
static void water_fill(long budget, const std::vector<size_t> &pending, std::vector<int> &take_out) {
    const int B = (int)pending.size();
    take_out.assign(B, 0);
    std::vector<int> act;
    for (int b = 0; b < B; ++b) if (pending[b] > 0) act.push_back(b);
    while (budget > 0 && !act.empty()) {
        const long share = std::max<long>(1, budget / (long)act.size());
        std::vector<int> next;
        for (int b : act) {
            if (budget <= 0) break;
            const long pend = (long)std::min<size_t>(pending[b], (size_t)1 << 40);   // a count, whatever the caller put there
            const long want = pend - take_out[b];
            const long take = std::min({want, share, budget});
            take_out[b] += (int)take;
            budget -= take;
            if (take_out[b] < pend) next.push_back(b);
        }
        act.swap(next);
    }
}

void rwkv_engine::plan_step(const rwkv_slot_input *in, StepPlan &pl, int reserve) {
    const int B = max_batch;
    // A decode loop hands the same pattern (the same slots, one token each, every row emitted) step after step: the plan of
    // the previous call is reused with the new token ids (dense: row index == slot index).
    if (last_plan.dense && (int)last_ntok.size() == B) {
        bool same = true;
        for (int b = 0; b < B && same; ++b) same = in[b].n_tokens == last_ntok[b] && (in[b].n_tokens == 0 || in[b].option == last_opt[b]);
        if (same) {
            pl = last_plan;
            for (int r = 0; r < pl.T; ++r) pl.token[r] = (int)in[r].tokens[0];
            return;
        }
    }
    pl.slot_consumed.assign(B, 0);
    pl.slot_out_begin.assign(B, 0);
    pl.slot_out_rows.assign(B, 0);
    std::vector<size_t> pending(B);
    for (int b = 0; b < B; ++b) pending[b] = in[b].n_tokens;
    water_fill(chunk - reserve, pending, pl.slot_consumed);
    pl.token.clear(); pl.slot.clear(); pl.prev.clear(); pl.last.clear();
    pl.seq_slot.clear(); pl.seq_begin.clear(); pl.seq_len.clear(); pl.out_rows.clear();
    for (int b = 0; b < B; ++b) {
        const int n = pl.slot_consumed[b];
        if (!n) continue;
        const int begin = (int)pl.token.size();
        pl.seq_slot.push_back(b); pl.seq_begin.push_back(begin); pl.seq_len.push_back(n);
        pl.slot_out_begin[b] = (int)pl.out_rows.size();
        const bool exhausted = (size_t)n == in[b].n_tokens;
        for (int i = 0; i < n; ++i) {
            pl.token.push_back((int)in[b].tokens[i]);
            pl.slot.push_back(b);
            pl.prev.push_back(i == 0 ? -1 : begin + i - 1);
            pl.last.push_back(i == 0 ? begin + n - 1 : -1);
            if (in[b].option == RWKV_OPTION_FULL || (in[b].option == RWKV_OPTION_LAST && exhausted && i == n - 1)) pl.out_rows.push_back(begin + i);
        }
        pl.slot_out_rows[b] = (int)pl.out_rows.size() - pl.slot_out_begin[b];
    }
    pl.T = (int)pl.token.size();
    pl.n_seq = (int)pl.seq_slot.size();
    pl.n_out = (int)pl.out_rows.size();
    const int no_dense = kn.no_dense;                           // A/B switch
    pl.dense = !no_dense && pl.T > 0 && pl.n_seq == pl.T && pl.n_out == pl.T;
    for (int i = 0; i < pl.n_seq && pl.dense; ++i) pl.dense = pl.seq_slot[i] == i;
    pl.id = ++plan_counter;
    last_plan = pl;
    last_ntok.assign(B, 0);
    last_opt.assign(B, 0);
    for (int b = 0; b < B; ++b) { last_ntok[b] = in[b].n_tokens; last_opt[b] = in[b].option; }
}

// pseudo: slots that have a logits row but no step row (rwkv_gen_arm_item's first draw).  Their rows stand behind the plan's in `slot`
// and `out_rows`, where the sampler stage finds them; the forward pass keeps seeing T rows.  T + pseudo.size() <= chunk (plan_step's reserve).
void rwkv_engine::upload_plan(const StepPlan &pl, const std::vector<int> &pseudo) {
    // a staging buffer is free again when the copy that read it has run (a step that emits nothing returns without waiting for the device,
    // so the previous copies may still be queued: four buffers, each guarded by the event recorded behind its copy)
    const int slot = meta_next;
    meta_next = (meta_next + 1) % META_RING;
    HIP_CHECK(hipEventSynchronize(meta_ev[slot]));
    const MetaView h(h_meta + (size_t)slot * meta_cap, chunk, max_batch);
    std::memcpy(h.token, pl.token.data(), pl.T * 4);
    std::memcpy(h.slot, pl.slot.data(), pl.T * 4);
    std::memcpy(h.prev, pl.prev.data(), pl.T * 4);
    std::memcpy(h.last, pl.last.data(), pl.T * 4);
    std::memcpy(h.out_rows, pl.out_rows.data(), pl.n_out * 4);
    std::memcpy(h.seq_slot, pl.seq_slot.data(), pl.n_seq * 4);
    std::memcpy(h.seq_begin, pl.seq_begin.data(), pl.n_seq * 4);
    std::memcpy(h.seq_len, pl.seq_len.data(), pl.n_seq * 4);
    for (size_t j = 0; j < pseudo.size(); ++j) { h.slot[(size_t)pl.T + j] = pseudo[j]; h.out_rows[(size_t)pl.n_out + j] = pl.T + (int)j; }
    HIP_CHECK(hipMemcpyAsync(d_meta, h.token, meta_cap * 4, hipMemcpyHostToDevice, s_main));
    HIP_CHECK(hipEventRecord(meta_ev[slot], s_main));
    uploaded_id = pl.id;
}

// ------------------------------------------------------------------------------------------------
// the forward pass: enqueue every kernel of one step on s_main
// ------------------------------------------------------------------------------------------------
void rwkv_engine::run_layers(int T, int n_seq, int n_out, const int *d_token, bool dense) {
    const int C = info.num_emb, V = info.num_vocab, H = info.num_head, L = info.num_layer;
    const RowMeta rm{d_token, dm.slot, dm.prev, dm.last, dense ? 1 : 0};

    float *cur = xA, *oth = xB;
    int np = 0;
    {
        EmbedArgs e{emb, ln0w, ln0b, d_token, cur, C, V};
        launch(FAM_ROW, [&] { launch_embed(e, T, s_main); });
    }
    for (int l = 0; l < L; ++l) {
        const LayerW &w = layers[l];
        cur_layer = l;
        // ---- time mix
        LnShiftArgs a{};
        a.x_in = cur; a.x_out = oth; a.P = P; a.np = np; a.pstride = pstride;
        a.lnw = w.ln1w; a.lnb = w.ln1b;
        a.sx = sxa + (long)l * C; a.sx_slot_stride = sx_slot_stride;
        a.rm = rm; a.C = C; a.ldh = C;
        std::vector<ProbSpec> ps;
        auto prob = [&](const DMat *W, const Opd &x, int act, float *out, int ldo) {
            ProbSpec s; s.W = W; s.x = x; s.act = act; s.out = out; s.ldo = ldo; return s;
        };
        // an operand as ITS CONSUMER's class sees it: the lo part exists only for launches that read hi + lo (Precision::Fp32, or promoted)
        auto as = [&](const Opd &o, int cls) { Opd r = o; if (!wide(cls)) r.lo = nullptr; return r; };
        const Opd aA[6] = {as(opA[0], CLS_ATT), as(opA[1], CLS_ATT), as(opA[2], CLS_ATT), as(opA[3], CLS_ATT), as(opA[4], CLS_ATT), as(opA[5], CLS_ATT)};
        const Opd aL[4] = {as(opL[0], CLS_LORA2), as(opL[1], CLS_LORA2), as(opL[2], CLS_LORA2), as(opL[3], CLS_LORA2)};
        const Opd aF[2] = {as(opA[0], CLS_FFN1), as(opA[1], CLS_FFN1)};
        const Opd aY = as(opY, CLS_WO), aK = as(opK, CLS_FV), aZ = as(opA[0], CLS_NONE), aM = as(opM, CLS_NONE);
        // single-token steps: the LayerNorm + token shift rides as a prologue of the GEMM that consumes it, and the launch
        // after that commits the shift state (LnProArgs / ShiftCommit in rwkv_kernels.h)
        auto ln_pro = [&](const LnShiftArgs &r, float *xx_pub) {
            LnProArgs lp{};
            lp.x_in = r.x_in; lp.x_out = r.x_out; lp.P = r.P; lp.np = r.np; lp.pstride = r.pstride;
            lp.lnw = r.lnw; lp.lnb = r.lnb; lp.sx = r.sx; lp.sx_slot_stride = r.sx_slot_stride; lp.rm = r.rm;
            lp.mode = r.mode; lp.xx_out = xx_pub; lp.C = C;
            return lp;
        };
        auto commit_of = [&](const LnShiftArgs &r, const float *xx_pub) {
            ShiftCommit cm{};
            cm.src = xx_pub; cm.sx = r.sx; cm.sx_slot_stride = r.sx_slot_stride; cm.rm = r.rm; cm.T = T; cm.C = C;
            return cm;
        };
        // RWKV_LAUNCH_LOG: what a row-kernel launch moves (its rows and their partial slabs in, state row in and out, residual and operands out)
        auto log_ln = [&](const LnShiftArgs &r) {
            int nlo = 0;
            for (int m = 0; m < r.nmix; ++m) nlo += r.olo[m] ? 1 : 0;
            log_row("ln_shift_kernel", T, T, (double)T * C * (4.0 * (4 + r.np + (r.xx_out ? 1 : 0) + (r.dx_out ? 1 : 0)) + 2.0 * (r.nmix + nlo)) + 4.0 * C * (2 + r.nmix));
        };
        bool att_fused = false;                                    // a commit of the time-mix shift state is pending
        if (info.version == 4) {
            a.mode = 0; a.nmix = 3;
            for (int i = 0; i < 3; ++i) { a.mu[i] = w.mu[i]; a.ohi[i] = aA[i].hi; a.olo[i] = aA[i].lo; }
            ps = {prob(w.Wk, aA[0], ACT_NONE, fk, C), prob(w.Wv, aA[1], ACT_NONE, fv, C), prob(w.Wr, aA[2], ACT_SIGMOID, fr, C)};
            { launch(FAM_ROW, [&] { launch_ln_shift(a, T, s_main); }); log_ln(a); }
            gemm(ps, T, FAM_GEMM, nullptr, CLS_ATT);
        } else if (info.version == 5) {
            a.mode = 0; a.nmix = 4;
            for (int i = 0; i < 4; ++i) { a.mu[i] = w.mu[i]; a.ohi[i] = aA[i].hi; a.olo[i] = aA[i].lo; }
            ps = {prob(w.Wk, aA[0], ACT_NONE, fk, C), prob(w.Wv, aA[1], ACT_NONE, fv, C),
                  prob(w.Wr, aA[2], ACT_NONE, fr, C), prob(w.Wg, aA[3], ACT_SILU, fg, C)};
            { launch(FAM_ROW, [&] { launch_ln_shift(a, T, s_main); }); log_ln(a); }
            gemm(ps, T, FAM_GEMM, nullptr, CLS_ATT);
        } else if (info.version == 6) {
            a.mode = 1; a.nmix = 1; a.mu[0] = w.mu[0]; a.ohi[0] = aZ.hi; a.olo[0] = aZ.lo;
            a.xx_out = xx; a.dx_out = dx;
            const int no_fuse = kn.no_v6_fuse, no_ln_fuse = kn.no_ln_fuse;
            att_fused = !no_fuse && !no_ln_fuse && v6_mix_ln_supported(T, C, Dm, hilo, np);
            if (!att_fused) { launch(FAM_ROW, [&] { launch_ln_shift(a, T, s_main); }); log_ln(a); }
            if ((v6_mix_supported(T, C, Dm) || v6_mix_wide_supported(T, C, Dm)) && !no_fuse) {
                // fused: x_c = xx + dx * (mu_c + W2_c tanh(W1_c z)) in one launch
                V6MixArgs m{};
                m.W1 = w.W1->data;
                for (int c = 0; c < 5; ++c) { m.W2[c] = w.W2[c]->data; m.mu[c] = w.mu[1 + c]; m.ohi[c] = aA[1 + c].hi; m.olo[c] = aA[1 + c].lo; }
                m.zhi = aZ.hi; m.zlo = aZ.lo; m.ldz = C;
                m.xx = xx; m.dx = dx; m.ldh = C; m.T = T; m.C = C; m.Dm = Dm;
                m.mg_hi = aM.hi; m.mg_lo = aM.lo;               // scratch of the two-launch form (T x 5 Dm halves, like the unfused path's operand)
                // fp32 partials of the K-sliced first stage: the partial-slab buffer, free between the ln_shift that summed the previous layer's
                // Fv slabs and this layer's Wo launch (<= 16 slices x 5 x T x Dm floats of its 8 x T x C)
                if ((long)16 * 5 * Dm <= (long)8 * C) { m.mp = P; m.ksp_max = kn.v6_ksp_max; m.ksp_blocks = kn.v6_ksp_blocks; m.ksp_min_t = kn.v6_ksp_min_t; }
                if (att_fused) { m.lnp = ln_pro(a, lnp_xx_att); m.mu_x = w.mu[0]; }
                launch(FAM_GEMM, [&] { launch_v6_mix(m, hilo, s_main); });
                // LoRA matrices once, z / xx / dx in, five operands out (+ the LayerNorm prologue's row traffic on single-token steps)
                if (const int nsl = v6_mix_split(m, hilo)) {
                    // two launches: phase 1 reads W1 and z and leaves m (f16, or fp32 partials per K slice); the apply launch reads m, W2, xx / dx, mu
                    const double mbytes = nsl > 1 ? (double)nsl * 5 * T * Dm * 4 : (double)5 * T * Dm * 2 * (m.mg_lo ? 2 : 1);
                    log_row("v6_mix_kernel", T, nsl * 5 * (T / 32), 5.0 * Dm * C * 2 + (double)T * C * 2.0 + mbytes);
                    const long ag = (long)((C / 16 + 7) / 8) * (T / 32);                // (launch_v6_mix: 16-token tiles below one block per CU)
                    log_row("v6_mix_apply_kernel", T, ag < 256 ? (long)((C / 16 + 7) / 8) * ((T + 15) / 16) : ag, 5.0 * Dm * C * 2 + mbytes + (double)T * C * (8.0 + 10.0 * (m.olo[0] ? 2 : 1)) + 20.0 * C);
                } else
                log_row("v6_mix_kernel", T, 0, 2.0 * (5.0 * Dm * C * 2) + (double)T * C * (2.0 + 8.0 + 10.0 * (m.olo[0] ? 2 : 1)) + 20.0 * C +
                                                   (att_fused ? (double)T * C * 4.0 * (4 + np) : 0.0));
            } else {
                {   // m = tanh(W1 z)  ->  operand [T][5*Dm]
                    ProbSpec s = prob(w.W1, aZ, ACT_TANH, nullptr, 0);
                    s.oh = aM;
                    ps = {s};
                    gemm(ps, T, FAM_GEMM);
                }
                ps.clear();
                for (int c = 0; c < 5; ++c) {   // x_c = xx + dx * (mu_c + W2_c m_c),  c in (w,k,v,r,g)
                    ProbSpec s = prob(w.W2[c], aM, ACT_NONE, nullptr, 0);
                    s.xoff = c * Dm;
                    s.bias = w.mu[1 + c]; s.post = POST_MIX; s.m0 = xx; s.m1 = dx; s.ldm = C;
                    s.oh = aA[1 + c];
                    ps.push_back(s);
                }
                gemm(ps, T, FAM_GEMM);
            }
            ps = {prob(w.Wk, aA[2], ACT_NONE, fk, C), prob(w.Wv, aA[3], ACT_NONE, fv, C),
                  prob(w.Wr, aA[4], ACT_NONE, fr, C), prob(w.Wg, aA[5], ACT_SILU, fg, C),
                  prob(w.D1, aA[1], ACT_TANH, ftd, Dd)};
            if (att_fused) { ShiftCommit cm = commit_of(a, lnp_xx_att); gemm(ps, T, FAM_GEMM, &cm, CLS_ATT); att_fused = false; }
            else gemm(ps, T, FAM_GEMM, nullptr, CLS_ATT);
        } else {
            a.mode = 1; a.nmix = 6;
            for (int i = 0; i < 6; ++i) { a.mu[i] = w.mu[i]; a.ohi[i] = aA[i].hi; a.olo[i] = aA[i].lo; }
            // opA: 0=r 1=w 2=k 3=v 4=a 5=g
            ps = {prob(w.Wr, aA[0], ACT_NONE, fr, C), prob(w.Wk, aA[2], ACT_NONE, fk, C), prob(w.Wv, aA[3], ACT_NONE, fv, C)};
            { ProbSpec s = prob(w.w1, aA[1], ACT_TANH, nullptr, 0); s.oh = aL[0]; ps.push_back(s); }
            { ProbSpec s = prob(w.a1, aA[4], ACT_NONE, nullptr, 0); s.oh = aL[1]; ps.push_back(s); }
            { ProbSpec s = prob(w.g1, aA[5], ACT_SIGMOID, nullptr, 0); s.oh = aL[2]; ps.push_back(s); }
            if (l > 0) { ProbSpec s = prob(w.v1, aA[3], ACT_NONE, nullptr, 0); s.oh = aL[3]; ps.push_back(s); }
            { launch(FAM_ROW, [&] { launch_ln_shift(a, T, s_main); }); log_ln(a); }
            gemm(ps, T, FAM_GEMM, nullptr, CLS_ATT);
            ps.clear();
            { ProbSpec s = prob(w.w2, aL[0], ACT_DECAY7, fw7, C); s.bias = w.w0; ps.push_back(s); }
            { ProbSpec s = prob(w.a2, aL[1], ACT_SIGMOID, fa7, C); s.bias = w.a0; ps.push_back(s); }
            { ProbSpec s = prob(w.g2, aL[2], ACT_NONE, fg, C); ps.push_back(s); }
            if (l > 0) { ProbSpec s = prob(w.v2, aL[3], ACT_SIGMOID, fvg7, C); s.bias = w.v0; ps.push_back(s); }
            gemm(ps, T, FAM_GEMM, nullptr, CLS_LORA2);
        }
        std::swap(cur, oth);
        if (info.version == 4) {
            Wkv4Args k{};
            k.C = C; k.n_seq = n_seq;
            k.seq_slot = dm.seq_slot; k.seq_begin = dm.seq_begin; k.seq_len = dm.seq_len; k.dense = dense ? 1 : 0;
            k.state = wkv + (long)l * wkv_layer_floats(); k.slot_stride = wkv_slot_stride;
            k.r = fr; k.k = fk; k.v = fv; k.w = w.wdec; k.u = w.u;
            k.yhi = aY.hi; k.ylo = aY.lo; k.ldh = C;
            launch(FAM_WKV, [&] { launch_wkv4(k, T > n_seq, s_main); });
            // three state rows in and out per sequence, r / k / v of every row in, the Wo operand out
            log_row(T > n_seq ? "wkv4_chunk_kernel" : "wkv4_kernel", T, T > n_seq ? (long)n_seq * (C / 64) : (long)n_seq * ((C + 255) / 256),
                    (double)n_seq * C * 24.0 + 8.0 * C + (double)T * C * 12.0 + (double)T * C * 2.0 * (k.ylo ? 2 : 1));
        } else {
            WkvArgs k{};
            k.version = info.version; k.H = H; k.C = C; k.n_seq = n_seq;
            k.seq_slot = dm.seq_slot; k.seq_begin = dm.seq_begin; k.seq_len = dm.seq_len; k.dense = dense ? 1 : 0;
            k.state = wkv + (long)l * H * 4096; k.slot_stride = wkv_slot_stride;
            k.r = fr; k.k = fk; k.v = fv; k.g = fg;
            k.wdec_or_decay = w.wdec; k.u = w.u; k.td = ftd; k.D2 = w.D2; k.Dd = Dd;
            k.w7 = fw7; k.a7 = fa7; k.vg7 = fvg7; k.k_k = w.k_k; k.k_a = w.k_a; k.r_k = w.r_k;
            k.v_first = vfirst; k.layer = l;
            k.lnx_w = w.lnxw; k.lnx_b = w.lnxb;
            k.yhi = aY.hi; k.ylo = aY.lo; k.ldh = C;
            k.max_rows = step_max_rows;
            launch(FAM_WKV, [&] { launch_wkv(k, T > n_seq, s_main); });
            // state tiles in and out (2 x 16 KiB per (slot, head)), the projections of every row in, the gated output operand out
            log_row(T > n_seq ? "wkv_chunk_kernel" : "wkv_kernel", T, (long)n_seq * H,
                    (double)n_seq * H * 32768.0 + (double)T * C * 4.0 * (info.version == 7 ? (l > 0 ? 8 : 6) : 4) +
                        (info.version == 6 ? (double)T * Dd * 4.0 + (double)C * Dd * 2.0 : 0.0) + (double)T * C * 2.0 * (k.ylo ? 2 : 1));
        }
        {
            ProbSpec s = prob(w.Wo, aY, ACT_NONE, P, C);
            s.partial = true;
            ps = {s};
            np = gemm(ps, T, FAM_GEMM, nullptr, CLS_WO);
        }
        // ---- channel mix
        LnShiftArgs f{};
        f.x_in = cur; f.x_out = oth; f.P = P; f.np = np; f.pstride = pstride;
        f.lnw = w.ln2w; f.lnb = w.ln2b;
        f.sx = sxf + (long)l * C; f.sx_slot_stride = sx_slot_stride;
        f.rm = rm; f.C = C; f.ldh = C;
        f.mode = info.version <= 5 ? 0 : 1;
        f.nmix = info.version == 7 ? 1 : 2;
        for (int i = 0; i < f.nmix; ++i) { f.mu[i] = w.fmu[i]; f.ohi[i] = aF[i].hi; f.olo[i] = aF[i].lo; }
        {
            ProbSpec s = prob(w.Fk, aF[0], ACT_RELU2, nullptr, 0);
            s.oh = aK;
            ps = {s};
            if (info.version != 7) { ProbSpec r = prob(w.Fr, aF[1], ACT_SIGMOID, frr, C); ps.push_back(r); }
            { launch(FAM_ROW, [&] { launch_ln_shift(f, T, s_main); }); log_ln(f); }
            gemm(ps, T, FAM_GEMM, nullptr, CLS_FFN1);
            std::swap(cur, oth);
        }
        {
            ProbSpec s = prob(w.Fv, aK, ACT_NONE, P, C);
            s.partial = true;
            if (info.version != 7) { s.post = POST_MUL; s.m0 = frr; s.ldm = C; }
            ps = {s};
            np = gemm(ps, T, FAM_GEMM, nullptr, CLS_FV);
        }
    }
    if (n_out > 0) {
        Opd aO = opO;
        if (!wide(CLS_HEAD)) aO.lo = nullptr;
        LnOutArgs o{cur, P, np, pstride, lnow, lnob, dense ? nullptr : dm.out_rows, aO.hi, aO.lo, C, C};
        launch(FAM_ROW, [&] { launch_ln_out(o, n_out, s_main); });
        std::vector<ProbSpec> ps(1);
        ps[0].W = head; ps[0].x = aO; ps[0].out = logits; ps[0].ldo = V;
        gemm(ps, n_out, FAM_HEAD, nullptr, CLS_HEAD);
    } else if (np > 0) {
        // nothing consumes the pending partial sums: fine, the residual stream dies with the step
    }
}

// upload the row metadata and enqueue the step (graph replay when this shape was seen before)
void rwkv_engine::run_plan(const StepPlan &pl) {
    // Dense steps read their token ids from pinned host memory through its device-visible alias (one uncached read per row in
    // the embedding kernel) and nothing else changes between two steps of the same plan, so a repeated dense plan needs no
    // host-to-device copy at all; everything else uploads its metadata.
    if (pl.dense) std::memcpy(h_tok, pl.token.data(), (size_t)pl.T * 4);
    if (!pl.dense || pl.id != uploaded_id) upload_plan(pl);
    const int *tok_ptr = pl.dense ? dv_tok : dm.token;
    step_max_rows = pl.max_rows();
    const bool short_rows = step_max_rows <= 8;                  // picks the WKV form: part of the graph's identity
    const uint64_t key = ((uint64_t)pl.dense << 63) | ((uint64_t)short_rows << 62) | ((uint64_t)pl.T << 40) | ((uint64_t)pl.n_seq << 20) | (uint64_t)pl.n_out;
    auto enqueue = [&] { run_layers(pl.T, pl.n_seq, pl.n_out, tok_ptr, pl.dense); };
    if (profiling) return enqueue();                            // timed launch by launch: event pairs, no graph
    hipGraphExec_t *exec = graphs.find(key);
    if (!exec) {
        // a shape's first step runs directly (graph_cache.h says why; the launchers' one-time attribute calls also happen here, outside a capture)
        if (!graphs.should_capture(key)) return enqueue();
        exec = &graphs.insert(key, capture(s_main, enqueue));
    }
    HIP_CHECK(hipGraphLaunch(*exec, s_main));
}

void rwkv_engine::infer_sample(const rwkv_slot_input *in, const rwkv_sample_params *sp, uint32_t *out_tokens, float *out_probs,
                               uint8_t *emitted, size_t *n_consumed) {
    HIP_CHECK(hipSetDevice(device));
    if (info.num_vocab > 65536) throw RwkvError(RWKV_ERR_UNSUPPORTED, "on-device sampling needs num_vocab <= 65536");
    std::vector<rwkv_slot_input> last(in, in + max_batch);
    for (int b = 0; b < max_batch; ++b) {
        last[b].option = RWKV_OPTION_LAST;
        if (emitted) emitted[b] = 0;
        if (n_consumed) n_consumed[b] = 0;
        if (in[b].n_tokens && !in[b].tokens) throw RwkvError(RWKV_ERR_INVALID, "slot has n_tokens>0 but tokens==NULL");
        if (in[b].n_tokens) gen_disarm_slot(b);
    }
    StepPlan pl;
    plan_step(last.data(), pl);
    if (pl.T == 0) return;
    // pack per-row sampler params + sparse adjustments (rows are in out_rows order == ascending slot order)
    size_t nadj = 0;
    unsigned needs = 0;
    int n_allow = 0;
    int *h_allow_row = (int *)(h_allow + (size_t)max_batch * info.num_vocab);
    for (int b = 0; b < max_batch; ++b) {
        if (pl.slot_out_rows[b] == 0) continue;
        const int r = pl.slot_out_begin[b];
        const rwkv_sample_params &p = sp[b];
        if (p.kind != RWKV_SAMPLER_MIROSTAT && !(p.temperature > 0.f)) throw RwkvError(RWKV_ERR_INVALID, "temperature must be > 0");
        if (p.n_adj && (!p.adj_tokens || !p.adj_values)) throw RwkvError(RWKV_ERR_INVALID, "null adjustment arrays");
        if (nadj + p.n_adj > ADJ_CAP) throw RwkvError(RWKV_ERR_INVALID, "too many logit adjustments");
        if (p.kind < RWKV_SAMPLER_NUCLEUS || p.kind > RWKV_SAMPLER_MIROSTAT) throw RwkvError(RWKV_ERR_UNSUPPORTED, "unknown sampler kind");
        const bool wide = p.kind == RWKV_SAMPLER_MIROSTAT ? p.tau >= MIRO_WIDE_SURPRISE : p.top_k > NARROW_TOP_K;
        needs |= sampler_need(p.kind, wide);
        samp.rows[r] = SampleRow{p.top_p, std::min(p.top_k, info.num_vocab), p.temperature, p.uniform, p.kind | (wide ? SAMPLE_WIDE : 0), p.tau};
        if (p.allow) {                                             // formatter mask: staged row by row, one H2D copy for all
            std::memcpy(h_allow + (size_t)n_allow * info.num_vocab, p.allow, (size_t)info.num_vocab);
            h_allow_row[n_allow++] = r;
        }
        for (size_t i = 0; i < p.n_adj; ++i, ++nadj) { samp.adj_row[nadj] = r; samp.adj_tok[nadj] = (int)p.adj_tokens[i]; samp.adj_val[nadj] = p.adj_values[i]; }
    }
    // The sampler kernel reads its per-row parameters from, and writes its 8 bytes per row to, pinned host memory directly (samp.dv_*): no copy sits
    // in front of the step or between it and the host seeing its tokens.  (Measured against an H2D copy of the parameters: no difference beyond noise.)
    run_plan(pl);
    if (pl.n_out > 0) {
        if (nadj) {
            HIP_CHECK(hipMemcpyAsync(d_adj_row, samp.adj_row, nadj * 4, hipMemcpyHostToDevice, s_main));
            HIP_CHECK(hipMemcpyAsync(d_adj_tok, samp.adj_tok, nadj * 4, hipMemcpyHostToDevice, s_main));
            HIP_CHECK(hipMemcpyAsync(d_adj_val, samp.adj_val, nadj * 4, hipMemcpyHostToDevice, s_main));
            launch_logit_adjust(logits, info.num_vocab, d_adj_row, d_adj_tok, d_adj_val, (int)nadj, s_main);
        }
        if (n_allow) {                                             // after the adjustments: -inf + bias stays -inf (run.rs:676-683)
            HIP_CHECK(hipMemcpyAsync(d_allow, h_allow, (size_t)n_allow * info.num_vocab, hipMemcpyHostToDevice, s_main));
            HIP_CHECK(hipMemcpyAsync(d_allow_row, h_allow_row, (size_t)n_allow * 4, hipMemcpyHostToDevice, s_main));
            launch_logit_mask(logits, info.num_vocab, d_allow_row, d_allow, n_allow, s_main);
        }
        launch_nucleus(logits, pl.n_out, info.num_vocab, samp.dv_rows, needs & NEEDS_NT, needs & NEEDS_MIRO, needs & NEEDS_WIDE, samp.dv_out_tok, samp.dv_out_prob, s_main);
        HIP_CHECK(hipStreamSynchronize(s_main));
        for (int b = 0; b < max_batch; ++b) {
            if (pl.slot_out_rows[b] == 0) continue;
            const int r = pl.slot_out_begin[b];
            if (out_tokens) out_tokens[b] = (uint32_t)samp.out_tok[r];
            if (out_probs) out_probs[b] = samp.out_prob[r];
            if (emitted) emitted[b] = 1;
        }
    } else {
        HIP_CHECK(hipStreamSynchronize(s_main));
    }
    if (n_consumed) for (int b = 0; b < max_batch; ++b) n_consumed[b] = (size_t)pl.slot_consumed[b];
}

void rwkv_engine::infer(const rwkv_slot_input *in, rwkv_slot_output *out) {
    HIP_CHECK(hipSetDevice(device));
    (void)hipGetLastError();                                   // start clean: the poll behind a row-less step must only see THIS call's errors
                                                               // (a handled, non-sticky failure of an earlier call — a probe — stays recorded otherwise)
    for (int b = 0; b < max_batch; ++b) {
        out[b].n_rows = 0;
        out[b].n_consumed = 0;
        if (in[b].n_tokens && !in[b].tokens) throw RwkvError(RWKV_ERR_INVALID, "slot has n_tokens>0 but tokens==NULL");
        if (in[b].option != RWKV_OPTION_LAST && in[b].option != RWKV_OPTION_FULL && in[b].option != RWKV_OPTION_NONE)
            throw RwkvError(RWKV_ERR_INVALID, "bad RnnOption");
        if (in[b].n_tokens) gen_disarm_slot(b);                  // the caller moves the slot's state itself: its generation context is void
    }
    StepPlan pl;
    plan_step(in, pl);
    if (pl.T == 0) return;
    for (int b = 0; b < max_batch; ++b)
        if (pl.slot_out_rows[b] > 0 && (!out[b].logits || out[b].logits_capacity_rows < (size_t)pl.slot_out_rows[b]))
            throw RwkvError(RWKV_ERR_INVALID, "logits buffer too small for slot " + std::to_string(b));
    run_plan(pl);
    const int V = info.num_vocab;
    // Logits go straight into the caller's buffers when those are pinned host memory (rwkv_host_alloc, or anything registered
    // with the HIP runtime): destinations that are contiguous in output-row order are merged, so a caller that hands one pinned
    // block for all slots gets ONE device-to-host copy and no host-side memcpy.  Pageable destinations take the staged path.
    struct Seg { float *dst; size_t row0, rows; };
    std::vector<Seg> segs;
    for (int b = 0; b < max_batch; ++b) {
        out[b].n_consumed = (size_t)pl.slot_consumed[b];
        out[b].n_rows = (size_t)pl.slot_out_rows[b];
        if (pl.slot_out_rows[b] == 0) continue;
        const size_t r0 = (size_t)pl.slot_out_begin[b], n = (size_t)pl.slot_out_rows[b];
        if (!segs.empty() && segs.back().dst + segs.back().rows * V == out[b].logits && segs.back().row0 + segs.back().rows == r0) segs.back().rows += n;
        else segs.push_back(Seg{out[b].logits, r0, n});
    }
    bool direct = !segs.empty();
    for (const Seg &g : segs) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, g.dst) != hipSuccess) { (void)hipGetLastError(); direct = false; break; }
        if (at.type != hipMemoryTypeHost) { direct = false; break; }
    }
    if (direct) {
        for (const Seg &g : segs)
            HIP_CHECK(hipMemcpyAsync(g.dst, logits + g.row0 * V, g.rows * V * 4, hipMemcpyDeviceToHost, s_main));
        HIP_CHECK(hipStreamSynchronize(s_main));
        return;
    }
    // A step that emits no row (state-only requests: RWKV_OPTION_NONE, or `Last` slots that still have tokens pending) hands nothing back
    // but `n_consumed`, which the plan already knows: it is NOT waited for.  The next call's host work (plan, metadata staging, launch)
    // overlaps this step on the device; every call that reads device data (`state.back / read / write`, a step with rows) is ordered
    // behind it on the stream and waits as before.  A LAUNCH error (bad configuration, a sticky device fault from an earlier step) is reported
    // by this call: the error state is polled after the enqueue; an asynchronous fault of THIS step surfaces at the next wait, and the slot states
    // it touched are undefined from then on (the caller has already advanced by n_consumed: include/rwkv_abi.h).
    if (pl.n_out == 0) {
        HIP_CHECK(hipPeekAtLastError());
        return;
    }
    HIP_CHECK(hipMemcpyAsync(logits_host, logits, (size_t)pl.n_out * V * 4, hipMemcpyDeviceToHost, s_main));
    HIP_CHECK(hipStreamSynchronize(s_main));
    for (const Seg &g : segs) std::memcpy(g.dst, logits_host + g.row0 * V, g.rows * V * 4);
}

// rwkv_infer_score: the step rwkv_infer would run with RWKV_OPTION_FULL on the scored slots (same plan, same step shape, same captured graph),
// then score_rows_kernel over the n_out rows of `logits`; 4 bytes per row come back instead of the row (perplexity run.rs:699-755, Choose 936-982)
void rwkv_engine::infer_score(const rwkv_slot_input *in, const uint32_t *const *targets, float *const *out_logp, size_t *n_consumed) {
    HIP_CHECK(hipSetDevice(device));
    (void)hipGetLastError();                                   // as in infer(): the poll below must only see THIS call's errors
    const uint32_t V = (uint32_t)info.num_vocab;
    std::vector<rwkv_slot_input> full(in, in + max_batch);
    for (int b = 0; b < max_batch; ++b) {                      // every refusal comes before anything is launched or disarmed
        n_consumed[b] = 0;
        if (in[b].n_tokens && !in[b].tokens) throw RwkvError(RWKV_ERR_INVALID, "slot has n_tokens>0 but tokens==NULL");
        if (!targets[b]) {
            if (in[b].n_tokens && in[b].option != RWKV_OPTION_NONE)
                throw RwkvError(RWKV_ERR_INVALID, "a slot without targets must be state-only (RWKV_OPTION_NONE) in rwkv_infer_score");
            continue;
        }
        full[b].option = RWKV_OPTION_FULL;
        if (!in[b].n_tokens) continue;
        if (!out_logp || !out_logp[b]) throw RwkvError(RWKV_ERR_INVALID, "scored slot " + std::to_string(b) + " has no out_logp buffer");
        for (size_t i = 0; i < in[b].n_tokens; ++i)
            if (targets[b][i] >= V && targets[b][i] != RWKV_SCORE_SKIP)
                throw RwkvError(RWKV_ERR_INVALID, "target " + std::to_string(targets[b][i]) + " of slot " + std::to_string(b) + " is not a token of this vocabulary");
    }
    for (int b = 0; b < max_batch; ++b) if (in[b].n_tokens) gen_disarm_slot(b);
    StepPlan pl;
    plan_step(full.data(), pl);
    if (pl.T == 0) return;
    for (int b = 0; b < max_batch; ++b)                        // a Full slot emits one row per consumed token: rows and targets line up
        if (targets[b]) std::memcpy(h_score_tgt + pl.slot_out_begin[b], targets[b], (size_t)pl.slot_out_rows[b] * 4);
    run_plan(pl);
    for (int b = 0; b < max_batch; ++b) n_consumed[b] = (size_t)pl.slot_consumed[b];
    if (pl.n_out == 0) {                                       // only state-only slots rode: not waited for, like a row-less rwkv_infer
        HIP_CHECK(hipPeekAtLastError());
        return;
    }
    HIP_CHECK(hipMemcpyAsync(d_score_tgt, h_score_tgt, (size_t)pl.n_out * 4, hipMemcpyHostToDevice, s_main));
    launch(FAM_SAMPLE, [&] { launch_score_rows(logits, d_score_tgt, d_score_out, pl.n_out, (int)V, s_main); });
    HIP_CHECK(hipMemcpyAsync(h_score_out, d_score_out, (size_t)pl.n_out * 4, hipMemcpyDeviceToHost, s_main));
    HIP_CHECK(hipPeekAtLastError());
    HIP_CHECK(hipStreamSynchronize(s_main));
    for (int b = 0; b < max_batch; ++b)
        if (targets[b] && pl.slot_out_rows[b]) std::memcpy(out_logp[b], h_score_out + pl.slot_out_begin[b], (size_t)pl.slot_out_rows[b] * 4);
}

// rwkv_infer_topn: rwkv_infer's step (the caller's options, hence its plan, step shape and captured graph), then topn_rows_kernel over the n_out
// rows of `logits`: n ids and n ln-probabilities per row come back instead of the row.  Slots with targets are scored as well, by the launch
// rwkv_infer_score makes, on the same block (the `echo` case: the realised token's ln-probability beside the alternatives, in one pass).
static_assert(RWKV_TOPN_MAX == TOPN_MAX && RWKV_TOPN_NONE == TOPN_NONE, "rwkv_abi.h and rwkv_kernels.h disagree");
void rwkv_engine::infer_topn(const rwkv_slot_input *in, int n, uint32_t *const *out_ids, float *const *out_logp, const uint32_t *const *targets,
                             float *const *out_tok_logp, size_t *n_rows, size_t *n_consumed) {
    HIP_CHECK(hipSetDevice(device));
    (void)hipGetLastError();                                   // as in infer(): the poll below must only see THIS call's errors
    const uint32_t V = (uint32_t)info.num_vocab;
    bool any_targets = false;
    for (int b = 0; b < max_batch; ++b) {                      // every refusal comes before anything is launched or disarmed
        n_rows[b] = 0;
        n_consumed[b] = 0;
        if (in[b].n_tokens && !in[b].tokens) throw RwkvError(RWKV_ERR_INVALID, "slot has n_tokens>0 but tokens==NULL");
        if (in[b].option != RWKV_OPTION_LAST && in[b].option != RWKV_OPTION_FULL && in[b].option != RWKV_OPTION_NONE)
            throw RwkvError(RWKV_ERR_INVALID, "bad RnnOption");
        const bool scored = targets && targets[b];
        if (!out_ids[b]) {
            if (in[b].n_tokens && in[b].option != RWKV_OPTION_NONE)
                throw RwkvError(RWKV_ERR_INVALID, "a slot without out_ids must be state-only (RWKV_OPTION_NONE) in rwkv_infer_topn");
            if (scored) throw RwkvError(RWKV_ERR_INVALID, "targets on slot " + std::to_string(b) + ", which lists nothing");
            continue;
        }
        if (!out_logp[b]) throw RwkvError(RWKV_ERR_INVALID, "listing slot " + std::to_string(b) + " has no out_logp buffer");
        if (!scored) continue;
        if (in[b].n_tokens && in[b].option != RWKV_OPTION_FULL)
            throw RwkvError(RWKV_ERR_INVALID, "targets need RWKV_OPTION_FULL (one row per token) on slot " + std::to_string(b));
        if (in[b].n_tokens && (!out_tok_logp || !out_tok_logp[b])) throw RwkvError(RWKV_ERR_INVALID, "scored slot " + std::to_string(b) + " has no out_tok_logp buffer");
        for (size_t i = 0; i < in[b].n_tokens; ++i)
            if (targets[b][i] >= V && targets[b][i] != RWKV_SCORE_SKIP)
                throw RwkvError(RWKV_ERR_INVALID, "target " + std::to_string(targets[b][i]) + " of slot " + std::to_string(b) + " is not a token of this vocabulary");
        any_targets |= in[b].n_tokens > 0;
    }
    for (int b = 0; b < max_batch; ++b) if (in[b].n_tokens) gen_disarm_slot(b);
    StepPlan pl;
    plan_step(in, pl);
    if (pl.T == 0) return;
    if (any_targets) {
        for (int r = 0; r < pl.n_out; ++r) h_score_tgt[r] = RWKV_SCORE_SKIP;   // rows of slots without targets are not scored
        for (int b = 0; b < max_batch; ++b)                    // a Full slot emits one row per consumed token: rows and targets line up
            if (targets[b] && pl.slot_out_rows[b]) std::memcpy(h_score_tgt + pl.slot_out_begin[b], targets[b], (size_t)pl.slot_out_rows[b] * 4);
    }
    run_plan(pl);
    for (int b = 0; b < max_batch; ++b) n_consumed[b] = (size_t)pl.slot_consumed[b];
    if (pl.n_out == 0) {                                       // no slot reached a row: not waited for, like a row-less rwkv_infer
        HIP_CHECK(hipPeekAtLastError());
        return;
    }
    const size_t cells = (size_t)pl.n_out * (size_t)n;
    launch(FAM_SAMPLE, [&] { launch_topn_rows(logits, n, d_topn_ids, d_topn_logp, pl.n_out, (int)V, s_main); });
    HIP_CHECK(hipMemcpyAsync(h_topn_ids, d_topn_ids, cells * 4, hipMemcpyDeviceToHost, s_main));
    HIP_CHECK(hipMemcpyAsync(h_topn_logp, d_topn_logp, cells * 4, hipMemcpyDeviceToHost, s_main));
    if (any_targets) {
        HIP_CHECK(hipMemcpyAsync(d_score_tgt, h_score_tgt, (size_t)pl.n_out * 4, hipMemcpyHostToDevice, s_main));
        launch(FAM_SAMPLE, [&] { launch_score_rows(logits, d_score_tgt, d_score_out, pl.n_out, (int)V, s_main); });
        HIP_CHECK(hipMemcpyAsync(h_score_out, d_score_out, (size_t)pl.n_out * 4, hipMemcpyDeviceToHost, s_main));
    }
    HIP_CHECK(hipPeekAtLastError());
    HIP_CHECK(hipStreamSynchronize(s_main));
    for (int b = 0; b < max_batch; ++b) {
        const size_t rows = (size_t)pl.slot_out_rows[b], r0 = (size_t)pl.slot_out_begin[b];
        if (!rows) continue;
        n_rows[b] = rows;
        std::memcpy(out_ids[b], h_topn_ids + r0 * n, rows * n * 4);
        std::memcpy(out_logp[b], h_topn_logp + r0 * n, rows * n * 4);
        if (targets && targets[b]) std::memcpy(out_tok_logp[b], h_score_out + r0, rows * 4);
    }
}

// ------------------------------------------------------------------------------------------------
// device-resident sampled generation (rwkv_gen_arm / _run, include/rwkv_abi.h): `process` (run.rs:788-1020) with the samplers on the device
// ------------------------------------------------------------------------------------------------
static_assert(RWKV_GEN_MAX_STOP_STR == GEN_MAX_STOP_STR && RWKV_GEN_STOP_LEN == GEN_STOP_LEN && RWKV_GEN_STOP_BUF == GEN_STOP_BUF &&
              RWKV_GEN_TOKEN_LEN == GEN_TOKEN_LEN && RWKV_GEN_HANDBACK == GEN_FIN_HANDBACK && RWKV_GEN_STOP == GEN_FIN_STOP &&
              RWKV_GEN_LENGTH == GEN_FIN_LENGTH, "include/rwkv_abi.h and csrc/gen_stop.h spell the same limits");
static_assert(RWKV_GEN_CANCELLED == GEN_FIN_CANCELLED && RWKV_GEN_WATCH_MAX_STEPS == GEN_WATCH_MAX_STEPS,
              "include/rwkv_abi.h and csrc/gen_watch.h spell the same limits");
void rwkv_engine::gen_init() {
    if (d_gen) return;
    const size_t B = (size_t)max_batch, V = (size_t)info.num_vocab;
    gen_slots.assign(B, GenSlotHost{});
    d_gen_dfa = dalloc<GenDfa>(B);
    HIP_CHECK(hipMemset(d_gen_dfa, 0, B * sizeof(GenDfa)));
    d_gen_pda = dalloc<GenPda>(B);
    HIP_CHECK(hipMemset(d_gen_pda, 0, B * sizeof(GenPda)));
    d_gen_stop = dalloc<GenStop>(B);
    HIP_CHECK(hipMemset(d_gen_stop, 0, B * sizeof(GenStop)));
    d_gen_held = dalloc<int>(B);
    HIP_CHECK(hipMemset(d_gen_held, 0, B * sizeof(int)));
    d_gen_pen = dalloc<float>(B * V);
    d_gen_bias = dalloc<float>(B * V);
    d_gen_shadow = dalloc<float *>(B);
    d_gen_rows = dalloc<SampleRow>((size_t)chunk);
    HIP_CHECK(hipMemset(d_gen_rows, 0, (size_t)chunk * sizeof(SampleRow)));   // a rider's row may be one no step has written yet: top_k 0 is inert
    d_gen_tok = dalloc<int>((size_t)chunk);
    d_gen_prob = dalloc<float>((size_t)chunk);
    d_gen_runstep = dalloc<int>(1);
    d_gen_out = dalloc<unsigned>(2 * (size_t)GEN_RING_STEPS * B);
    h_gen_out = hostalloc<unsigned>(2 * (size_t)GEN_RING_STEPS * B);
    HIP_CHECK(hipMemset(d_gen_shadow, 0, B * sizeof(float *)));
    d_gen_cap = dalloc<GenCap>(B);
    HIP_CHECK(hipMemset(d_gen_cap, 0, B * sizeof(GenCap)));
    d_gen = dalloc<GenSlot>(B);                                   // last: marks the block as complete
    HIP_CHECK(hipMemset(d_gen, 0, B * sizeof(GenSlot)));
}

void rwkv_engine::gen_arm(int slot, const rwkv_gen_params &p, const uint32_t *prompt, size_t n_prompt, bool from_item) {
    HIP_CHECK(hipSetDevice(device));
    const size_t V = (size_t)info.num_vocab;
    if (V > 65536) throw RwkvError(RWKV_ERR_UNSUPPORTED, "on-device sampling needs num_vocab <= 65536");
    if (p.allow) throw RwkvError(RWKV_ERR_UNSUPPORTED, "a formatter mask needs the host between tokens: use rwkv_infer_sample");
    if (p.kind < RWKV_SAMPLER_NUCLEUS || p.kind > RWKV_SAMPLER_MIROSTAT) throw RwkvError(RWKV_ERR_UNSUPPORTED, "unknown sampler kind");
    const bool miro = p.kind == RWKV_SAMPLER_MIROSTAT;
    if (!miro && p.top_k > NARROW_TOP_K && !(p.reserved & RWKV_GEN_WIDE_TOP_K))
        throw RwkvError(RWKV_ERR_UNSUPPORTED, "top_k > 256 in resident generation needs RWKV_GEN_WIDE_TOP_K in `reserved`");
    if (p.n_stop > RWKV_GEN_MAX_STOP) throw RwkvError(RWKV_ERR_UNSUPPORTED, "at most RWKV_GEN_MAX_STOP stop tokens");
    if (!miro && !(p.temperature > 0.f)) throw RwkvError(RWKV_ERR_INVALID, "temperature must be > 0");
    if (p.max_tokens <= 0) throw RwkvError(RWKV_ERR_INVALID, "max_tokens must be > 0");
    if (!prompt && !from_item && p.first_token >= V) throw RwkvError(RWKV_ERR_INVALID, "first_token out of range");
    for (size_t i = 0; i < n_prompt; ++i) if (prompt[i] >= V) throw RwkvError(RWKV_ERR_INVALID, "prompt token out of range");
    if ((p.n_penalty && (!p.penalty_tokens || !p.penalty_values)) || (p.n_bias && (!p.bias_tokens || !p.bias_values)) || (p.n_stop && !p.stop_tokens))
        throw RwkvError(RWKV_ERR_INVALID, "null penalty / bias / stop array");
    gen_init();
    const size_t b = (size_t)slot;
    GenSlotHost &s = gen_slots[b];
    if (!s.shadow) {                                               // the slot's first arm: room for its state at the step it will finish in
        s.shadow = dalloc<float>((size_t)(2 * sx_slot_stride + wkv_slot_stride));
        HIP_CHECK(hipMemcpy(d_gen_shadow + b, &s.shadow, sizeof(float *), hipMemcpyHostToDevice));
    }
    GenSlot g{};
    g.top_p = p.top_p; g.top_k = miro ? 1 : std::min(p.top_k, info.num_vocab); g.temperature = miro ? 1.0f : p.temperature; g.tau = p.tau; g.kind = p.kind;
    g.presence = p.presence_penalty; g.frequency = p.frequency_penalty; g.decay = p.penalty_decay;
    g.miro_target = p.miro_target; g.miro_rate = p.miro_rate;
    // wide for the slot's whole life: max_surprise starts at p.tau and every update caps it at 4 * target (mirostat.rs:87), and below
    // 8192 candidates sample_wide_kernel returns nucleus_kernel's bits, so the run equals the per-token loop that routes by the current value
    g.wide = (miro ? std::max(p.tau, 4.0f * p.miro_target) >= MIRO_WIDE_SURPRISE : p.top_k > NARROW_TOP_K) ? SAMPLE_WIDE : 0;
    g.seed = p.seed; g.stream = p.stream; g.draws = 0;
    g.max_tokens = p.max_tokens; g.emitted = 0; g.finish = RWKV_GEN_RUNNING; g.freeze_at = -1;
    g.n_stop = (int)p.n_stop;
    for (size_t i = 0; i < p.n_stop; ++i) g.stop[i] = p.stop_tokens[i];
    std::vector<unsigned> pen(V, GEN_ABSENT);                      // dense rows: 256 KiB each at the World vocabulary, once per request
    std::vector<float> bias(V, 0.f);
    if (!miro)
        for (size_t i = 0; i < p.n_penalty; ++i)
            if (p.penalty_tokens[i] < V) std::memcpy(&pen[p.penalty_tokens[i]], &p.penalty_values[i], 4);
    for (size_t i = 0; i < p.n_bias; ++i)
        if (p.bias_tokens[i] < V && p.bias_values[i] != 0.f) { bias[p.bias_tokens[i]] += p.bias_values[i]; g.has_bias = 1; }
    HIP_CHECK(hipMemcpyAsync(d_gen_pen + b * V, pen.data(), V * 4, hipMemcpyHostToDevice, s_main));
    HIP_CHECK(hipMemcpyAsync(d_gen_bias + b * V, bias.data(), V * 4, hipMemcpyHostToDevice, s_main));
    HIP_CHECK(hipMemcpyAsync(d_gen + b, &g, sizeof(GenSlot), hipMemcpyHostToDevice, s_main));
    HIP_CHECK(hipMemsetAsync(&d_gen_stop[b].n_str, 0, 2 * sizeof(int), s_main));   // re-arming clears the stop strings and their buffer
    HIP_CHECK(hipMemsetAsync(d_gen_dfa + b, 0, sizeof(GenDfa), s_main));             // ... and the constraint
    HIP_CHECK(hipMemsetAsync(d_gen_pda + b, 0, sizeof(GenPda), s_main));             // ... of either kind
    HIP_CHECK(hipMemsetAsync(d_gen_cap + b, 0, sizeof(GenCap), s_main));             // ... and what it captured or started from
    const int first = prompt || from_item ? 0 : (int)p.first_token;   // with a prompt, or an item, the slot's first draw fills it
    HIP_CHECK(hipMemcpyAsync(d_gen_held + b, &first, sizeof(int), hipMemcpyHostToDevice, s_main));
    HIP_CHECK(hipStreamSynchronize(s_main));
    s.g = g;
    if (s.topn) {                                                  // re-arming: the slot lists nothing until rwkv_gen_set_topn says so again
        s.topn = 0;
        HIP_CHECK(hipMemset(d_gen_topn_n + b, 0, sizeof(int)));
    }
    gen_drop_table(s);                                             // behind the synchronize: no step is in flight
    s.reset_request();                                             // an item nobody took goes with the request that asked for it
    s.prompt.assign(prompt, prompt + n_prompt);
    s.armed = true;
    gen_cancel_clear(slot);                                        // a flag set for the request that held the slot before is not this one's
}

// The token-bytes table of the stop-string matcher: what `tokenizer.decode(&[token])` (run.rs:856) yields per id.  Captured steps hold the
// table's pointers, so a new table drops them; it is refused while a slot still matches against the old one.
void rwkv_engine::gen_set_token_bytes(const uint8_t *bytes, const int32_t *lens, size_t n) {
    HIP_CHECK(hipSetDevice(device));
    if (!lens || n == 0 || n >= 0x7fffffffu) throw RwkvError(RWKV_ERR_INVALID, "token table: null lens or no tokens");
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        if (lens[i] < -1) throw RwkvError(RWKV_ERR_INVALID, "token table: negative length");
        if (lens[i] > RWKV_GEN_TOKEN_LEN) throw RwkvError(RWKV_ERR_UNSUPPORTED, "token table: a token is longer than RWKV_GEN_TOKEN_LEN");
        if (lens[i] > 0) total += (size_t)lens[i];
    }
    if (total && !bytes) throw RwkvError(RWKV_ERR_INVALID, "token table: null bytes");
    if (total >= GEN_TOK_UNKNOWN) throw RwkvError(RWKV_ERR_UNSUPPORTED, "token table: more than 2 GiB of bytes");
    for (const GenSlotHost &s : gen_slots) if (s.has_stops) throw RwkvError(RWKV_ERR_INVALID, "token table: a slot has stop strings set");
    for (const GenSlotHost &s : gen_slots) if (s.constraint == GenConstraint::Dfa) throw RwkvError(RWKV_ERR_INVALID, "token table: a slot has a constraint set");
    for (const GenSlotHost &s : gen_slots) if (s.constraint == GenConstraint::Pda) throw RwkvError(RWKV_ERR_INVALID, "token table: a slot has a stack constraint set");
    std::vector<unsigned> off(n + 1);
    size_t pos = 0;
    for (size_t i = 0; i < n; ++i) {
        off[i] = (unsigned)pos | (lens[i] < 0 ? GEN_TOK_UNKNOWN : 0u);
        if (lens[i] > 0) pos += (size_t)lens[i];
    }
    off[n] = (unsigned)pos;
    HIP_CHECK(hipStreamSynchronize(s_main));
    gen_graphs.clear();
    if (d_tok_off) { (void)hipFree(d_tok_off); d_tok_off = nullptr; }
    if (d_tok_bytes) { (void)hipFree(d_tok_bytes); d_tok_bytes = nullptr; }
    n_tok = 0;
    HIP_CHECK(hipMalloc((void **)&d_tok_off, (n + 1) * sizeof(unsigned)));
    HIP_CHECK(hipMalloc((void **)&d_tok_bytes, std::max<size_t>(total, 16)));
    HIP_CHECK(hipMemcpy(d_tok_off, off.data(), (n + 1) * sizeof(unsigned), hipMemcpyHostToDevice));
    if (total) HIP_CHECK(hipMemcpy(d_tok_bytes, bytes, total, hipMemcpyHostToDevice));
    n_tok = (int)n;
    std::memset(tok_single, 0, sizeof(tok_single));
    for (size_t i = 0, at = 0; i < n; ++i) {
        if (lens[i] == 1 && i > 0) tok_single[bytes[at]] = 1;        // token 0 is never allowed (gen_dfa.h)
        if (lens[i] > 0) at += (size_t)lens[i];
    }
}

// What rwkv_gen_set_constraint and rwkv_gen_set_pda share.  An armed, unfinished slot; with a table (`present`): no constraint of the other
// kind, a token table, then fill(h, upload): the caller's own checks and its entry, where upload({plane, ...}) puts the planes one behind
// the other into one fresh buffer and returns it.  Between runs: the stream is idle, so the old table can go at once.  NULL through the
// call of the OTHER kind rewrites that kind's (already zero) entry and leaves the slot's constraint and its table alone.
template <class Entry, class Fill>
void rwkv_engine::gen_install(int slot, GenConstraint kind, bool present, Entry *d_entries, Fill fill) {
    HIP_CHECK(hipSetDevice(device));
    if (!gen_is_live(slot)) throw RwkvError(RWKV_ERR_INVALID, "a constraint needs an armed, unfinished slot");
    GenSlotHost &s = gen_slots[(size_t)slot];
    Entry h{};
    void *buf = nullptr;                                           // the fresh table: upload (below) fills it, a failed entry copy frees it, the swap keeps it
    if (present) {
        if (s.constraint != GenConstraint::None && s.constraint != kind)
            throw RwkvError(RWKV_ERR_INVALID, std::string("constraint: the slot has a ") + (s.constraint == GenConstraint::Pda ? "stack" : "DFA") + " constraint set (a slot holds one kind)");
        if (!d_tok_off) throw RwkvError(RWKV_ERR_INVALID, "a constraint needs the token table: rwkv_gen_set_token_bytes");
        fill(h, [&](std::initializer_list<Plane> planes) {
            size_t total = 0, at = 0;
            for (const Plane &p : planes) total += p.bytes;
            HIP_CHECK(hipMalloc(&buf, total));
            for (const Plane &p : planes) {
                if (hipMemcpy((char *)buf + at, p.src, p.bytes, hipMemcpyHostToDevice) != hipSuccess) {
                    (void)hipFree(buf);
                    throw RwkvError(RWKV_ERR_DEVICE, "constraint: copying the table failed");
                }
                at += p.bytes;
            }
            return (const char *)buf;
        });
    }
    HIP_CHECK(hipStreamSynchronize(s_main));
    if (hipMemcpy(d_entries + slot, &h, sizeof(Entry), hipMemcpyHostToDevice) != hipSuccess) {
        if (buf) (void)hipFree(buf);
        throw RwkvError(RWKV_ERR_DEVICE, "constraint: copying the slot's entry failed");
    }
    if (!present && s.constraint != kind) return;
    gen_drop_table(s);
    s.table = buf;
    s.constraint = present ? kind : GenConstraint::None;
}

// The byte-automaton constraint (rwkv_gen_set_constraint): the table goes to the device, the GenDfa of the slot points at it.
void rwkv_engine::gen_set_constraint(int slot, const rwkv_dfa *dfa, int state, int halt_mode) {
    gen_install(slot, GenConstraint::Dfa, dfa != nullptr, d_gen_dfa, [&](GenDfa &h, auto upload) {
        if (state < 1 || state >= dfa->n_states) throw RwkvError(RWKV_ERR_INVALID, "constraint: state 0 (dead) or out of range");
        if (halt_mode != RWKV_DFA_HALT_FINAL && halt_mode != RWKV_DFA_HALT_ACCEPT) throw RwkvError(RWKV_ERR_INVALID, "constraint: unknown halt mode");
        if (!dfa_never_stuck(*dfa, state, halt_mode, tok_single))
            throw RwkvError(RWKV_ERR_UNSUPPORTED, "constraint: a reachable state has no single-byte token that leads on (a row could be masked whole)");
        const size_t tbytes = (size_t)dfa->n_states * 256 * sizeof(uint16_t), fbytes = (size_t)dfa->n_states;
        if (!d_tok_end) HIP_CHECK(hipMalloc((void **)&d_tok_end, (size_t)chunk * (size_t)info.num_vocab * sizeof(unsigned short)));
        const char *buf = upload({{dfa->trans.data(), tbytes}, {dfa->flags.data(), fbytes}});
        h.trans = (const unsigned short *)buf; h.flags = (const unsigned char *)buf + tbytes;
        h.state = state; h.mode = halt_mode;
    });
}

int rwkv_engine::gen_constraint_state(int slot) {
    HIP_CHECK(hipSetDevice(device));
    if (!gen_is_armed(slot)) throw RwkvError(RWKV_ERR_INVALID, "slot is not armed");
    if (gen_slots[(size_t)slot].constraint != GenConstraint::Dfa) return 0;
    GenDfa h{};
    HIP_CHECK(hipMemcpyAsync(&h, d_gen_dfa + slot, sizeof(GenDfa), hipMemcpyDeviceToHost, s_main));
    HIP_CHECK(hipStreamSynchronize(s_main));
    return h.state;
}

// The stack-automaton constraint (rwkv_gen_set_pda): the two planes and the flags go to the device, the GenPda of the slot points at them
// and carries the configuration.
void rwkv_engine::gen_set_pda(int slot, const rwkv_pda *pda, int state, const uint16_t *stack, int depth, int halt_mode) {
    gen_install(slot, GenConstraint::Pda, pda != nullptr, d_gen_pda, [&](GenPda &h, auto upload) {
        if (state < 1 || state >= pda->n_states) throw RwkvError(RWKV_ERR_INVALID, "constraint: state 0 (dead) or out of range");
        if (depth < 0 || depth > pda->max_depth || (depth && !stack)) throw RwkvError(RWKV_ERR_INVALID, "constraint: depth outside 0 .. max_depth, or a null stack");
        for (int i = 0; i < depth; ++i)
            if (stack[i] < 1 || stack[i] >= pda->n_states) throw RwkvError(RWKV_ERR_INVALID, "constraint: a stack entry is no live state of the table");
        if (halt_mode != RWKV_PDA_HALT_FINAL && halt_mode != RWKV_PDA_HALT_ACCEPT) throw RwkvError(RWKV_ERR_INVALID, "constraint: unknown halt mode");
        if (!pda_never_stuck(*pda, state, stack, depth, tok_single))
            throw RwkvError(RWKV_ERR_UNSUPPORTED, "constraint: a reachable state has no single-byte token with a plain transition that leads on (a row could be masked whole)");
        const size_t tbytes = (size_t)pda->n_states * 256 * sizeof(uint16_t), fbytes = (size_t)pda->n_states;
        const char *buf = upload({{pda->next.data(), tbytes}, {pda->act.data(), tbytes}, {pda->flags.data(), fbytes}});
        h.next = (const unsigned short *)buf; h.act = (const unsigned short *)(buf + tbytes); h.flags = (const unsigned char *)buf + 2 * tbytes;
        h.state = state; h.depth = depth; h.mode = halt_mode; h.max_depth = pda->max_depth;
        for (int i = 0; i < depth; ++i) h.stack[i] = stack[i];
    });
}

void rwkv_engine::gen_pda_config(int slot, int32_t *state, uint16_t *stack, size_t cap, int32_t *depth) {
    HIP_CHECK(hipSetDevice(device));
    if (!gen_is_armed(slot)) throw RwkvError(RWKV_ERR_INVALID, "slot is not armed");
    *state = 0;
    *depth = 0;
    if (gen_slots[(size_t)slot].constraint != GenConstraint::Pda) return;
    GenPda h{};
    HIP_CHECK(hipMemcpyAsync(&h, d_gen_pda + slot, sizeof(GenPda), hipMemcpyDeviceToHost, s_main));
    HIP_CHECK(hipStreamSynchronize(s_main));
    *state = h.state;
    *depth = std::min(std::max(h.depth, 0), (int)GEN_PDA_MAX_DEPTH);
    for (size_t i = 0; i < std::min((size_t)*depth, cap); ++i) stack[i] = h.stack[i];
}

// `GenerateRequest::stop` (run.rs:899-932) of an armed, unfinished slot, and the bytes the caller's matcher holds after the tokens it handled itself
void rwkv_engine::gen_set_stops(int slot, const rwkv_gen_stops &s) {
    HIP_CHECK(hipSetDevice(device));
    const size_t b = (size_t)slot;
    if (!gen_is_live(slot)) throw RwkvError(RWKV_ERR_INVALID, "stop strings need an armed, unfinished slot");
    if ((s.n && (!s.strs || !s.lens)) || (s.n_tail && !s.tail)) throw RwkvError(RWKV_ERR_INVALID, "null stop-string array");
    if (s.n > RWKV_GEN_MAX_STOP_STR) throw RwkvError(RWKV_ERR_UNSUPPORTED, "at most RWKV_GEN_MAX_STOP_STR stop strings");
    if (s.n_tail > RWKV_GEN_STOP_BUF) throw RwkvError(RWKV_ERR_UNSUPPORTED, "the tail is longer than RWKV_GEN_STOP_BUF");
    for (size_t i = 0; i < s.n; ++i) {
        if (s.lens[i] > RWKV_GEN_STOP_LEN) throw RwkvError(RWKV_ERR_UNSUPPORTED, "a stop string is longer than RWKV_GEN_STOP_LEN");
        if (s.lens[i] && !s.strs[i]) throw RwkvError(RWKV_ERR_INVALID, "null stop string");
    }
    if (s.n && !d_tok_off) throw RwkvError(RWKV_ERR_INVALID, "stop strings need the token table: rwkv_gen_set_token_bytes");
    std::vector<GenStop> h(1);
    std::memset(h.data(), 0, sizeof(GenStop));
    for (size_t i = 0; i < s.n; ++i) {
        h[0].len[i] = (unsigned short)s.lens[i];
        if (s.lens[i]) std::memcpy(h[0].str[i], s.strs[i], s.lens[i]);
    }
    h[0].n_str = (int)s.n;
    h[0].buf_len = (int)s.n_tail;
    if (s.n_tail) std::memcpy(h[0].buf, s.tail, s.n_tail);
    HIP_CHECK(hipMemcpyAsync(d_gen_stop + b, h.data(), sizeof(GenStop), hipMemcpyHostToDevice, s_main));
    HIP_CHECK(hipStreamSynchronize(s_main));
    gen_slots[b].has_stops = s.n != 0;
}

size_t rwkv_engine::gen_stop_tail(int slot, uint8_t *out, size_t cap) {
    HIP_CHECK(hipSetDevice(device));
    const size_t b = (size_t)slot;
    if (!gen_is_armed(slot)) throw RwkvError(RWKV_ERR_INVALID, "slot is not armed");
    std::vector<GenStop> h(1);
    HIP_CHECK(hipMemcpyAsync(h.data(), d_gen_stop + b, sizeof(GenStop), hipMemcpyDeviceToHost, s_main));
    HIP_CHECK(hipStreamSynchronize(s_main));
    const size_t len = (size_t)std::min(std::max(h[0].buf_len, 0), (int)GEN_STOP_BUF);
    if (out && cap) std::memcpy(out, h[0].buf, std::min(len, cap));
    return len;
}

// The places an armed, unfinished slot lists per emitted token (rwkv_gen_set_topn).  Between runs: the stream is idle.
void rwkv_engine::gen_set_topn(int slot, int n) {
    HIP_CHECK(hipSetDevice(device));
    const size_t b = (size_t)slot, B = (size_t)max_batch, V = (size_t)info.num_vocab;
    if (!gen_is_live(slot)) throw RwkvError(RWKV_ERR_INVALID, "top-n lists need an armed, unfinished slot");
    if (n < 0 || n > RWKV_TOPN_MAX) throw RwkvError(RWKV_ERR_INVALID, "n must be 0.." + std::to_string(RWKV_TOPN_MAX) + ", got " + std::to_string(n));
    if (!d_gen_topn_n) {
        if (n == 0) return;
        const size_t ring = (size_t)GEN_RING_STEPS * B;
        d_gen_top_ids = dalloc<unsigned>(ring * TOPN_MAX); h_gen_top_ids = hostalloc<unsigned>(ring * TOPN_MAX);
        d_gen_top_logp = dalloc<float>(ring * TOPN_MAX); h_gen_top_logp = hostalloc<float>(ring * TOPN_MAX);
        d_gen_tok_logp = dalloc<float>(ring); h_gen_tok_logp = hostalloc<float>(ring);
        d_gen_side_ms = dalloc<float>(B * 2);
        d_gen_side_rows = dalloc<float>(B * V);
        int *topn_n = dalloc<int>(B);
        HIP_CHECK(hipMemset(topn_n, 0, B * sizeof(int)));
        d_gen_topn_n = topn_n;                                     // last: marks the block as complete
    }
    HIP_CHECK(hipStreamSynchronize(s_main));
    HIP_CHECK(hipMemcpy(d_gen_topn_n + b, &n, sizeof(int), hipMemcpyHostToDevice));
    gen_slots[b].topn = n;
}

// A watch: the block is mapped and coherent like h_tok (uncached on the device: a store is the host's to see at once, a load is the
// host's latest store).  Between runs: the stream is idle, so the descriptor may be rewritten under the captured steps that read it.
void rwkv_engine::gen_watch_open(int ring_steps, rwkv_gen_watch **out) {
    HIP_CHECK(hipSetDevice(device));
    if (gen_watch) throw RwkvError(RWKV_ERR_INVALID, "the engine already has a watch open");
    if (ring_steps < 1 || ring_steps > RWKV_GEN_WATCH_MAX_STEPS)
        throw RwkvError(RWKV_ERR_INVALID, "ring_steps must be 1.." + std::to_string(RWKV_GEN_WATCH_MAX_STEPS) + ", got " + std::to_string(ring_steps));
    gen_init();
    if (!d_gen_watch) d_gen_watch = dalloc<GenWatchDev>(1);
    auto w = std::make_unique<rwkv_gen_watch>();
    w->ring_steps = ring_steps; w->B = max_batch;
    const size_t bytes = gen_watch_bytes(ring_steps, max_batch);
    void *p = nullptr, *dv = nullptr;
    HIP_CHECK(hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(p, 0, bytes);                                      // stamps 0 (no record), head 0, no cancel word set
    if (hipHostGetDevicePointer(&dv, p, 0) != hipSuccess) { (void)hipHostFree(p); throw RwkvError(RWKV_ERR_DEVICE, "no device alias for the watch's ring"); }
    w->ring = (unsigned char *)p;
    GenWatchDev d{};
    d.ring = (unsigned char *)dv; d.cancel = gen_watch_cancel_ptr((unsigned char *)dv, ring_steps, max_batch); d.seq = 0; d.ring_steps = ring_steps;
    hipError_t err = hipStreamSynchronize(s_main);
    if (err == hipSuccess) err = hipMemcpy(d_gen_watch, &d, sizeof d, hipMemcpyHostToDevice);
    if (err != hipSuccess) { (void)hipHostFree(p); HIP_CHECK(err); }
    gen_watch = w.release();
    *out = gen_watch;
}
void rwkv_engine::gen_watch_close(rwkv_gen_watch *w) {
    HIP_CHECK(hipSetDevice(device));
    if (!w || w != gen_watch) throw RwkvError(RWKV_ERR_INVALID, "not this engine's open watch");
    HIP_CHECK(hipStreamSynchronize(s_main));
    const GenWatchDev d{};                                         // ring null: a step that still reached gen_publish would write nothing
    HIP_CHECK(hipMemcpy(d_gen_watch, &d, sizeof d, hipMemcpyHostToDevice));
    (void)hipHostFree(w->ring);
    delete w;
    gen_watch = nullptr;
}

// ---- captures and items: the prefix cache's two fill points (run.rs:834-845, 995-1001) and its full hit (run.rs:809-810) ----
static_assert(RWKV_GEN_CAPTURE_PROMPT == GEN_CAPTURE_PROMPT && RWKV_GEN_CAPTURE_FINISH == GEN_CAPTURE_FINISH, "rwkv_abi.h and rwkv_kernels.h disagree");
rwkv_gen_item *rwkv_engine::gen_item_new() const {
    std::unique_ptr<rwkv_gen_item, void (*)(rwkv_gen_item *)> it(new rwkv_gen_item(), gen_item_destroy);
    it->st.device = device;
    it->version = info.version; it->L = info.num_layer; it->C = info.num_emb; it->V = info.num_vocab;
    it->nsx = sx_slot_stride; it->nw = wkv_slot_stride;
    HIP_CHECK(hipMalloc((void **)&it->state, (size_t)(2 * it->nsx + it->nw) * 4));
    HIP_CHECK(hipMalloc((void **)&it->row, (size_t)it->V * 4));
    it->st = block_state(it->state);
    return it.release();
}
// the slot's GenCap as the host knows it.  Between runs: the stream is idle.
void rwkv_engine::gen_cap_upload(int slot) {
    const GenSlotHost &s = gen_slots[(size_t)slot];
    GenCap c{};
    if (const rwkv_gen_item *it = s.cap_item[0]) { c.p_state = it->state; c.p_row = it->row; }
    if (const rwkv_gen_item *it = s.cap_item[1]) c.f_row = it->row;
    if (s.inj) c.inj_row = s.inj_row;
    HIP_CHECK(hipStreamSynchronize(s_main));
    HIP_CHECK(hipMemcpy(d_gen_cap + slot, &c, sizeof c, hipMemcpyHostToDevice));
}
void rwkv_engine::gen_set_capture(int slot, unsigned what) {
    HIP_CHECK(hipSetDevice(device));
    if (!gen_is_live(slot)) throw RwkvError(RWKV_ERR_INVALID, "a capture needs an armed, unfinished slot");
    if (what & ~(unsigned)(RWKV_GEN_CAPTURE_PROMPT | RWKV_GEN_CAPTURE_FINISH)) throw RwkvError(RWKV_ERR_INVALID, "unknown capture bit");
    if ((what & RWKV_GEN_CAPTURE_PROMPT) && gen_prompt_left(slot) == 0)
        throw RwkvError(RWKV_ERR_INVALID, "RWKV_GEN_CAPTURE_PROMPT: the slot has no prompt left, its end has passed");
    GenSlotHost &s = gen_slots[(size_t)slot];
    std::array<rwkv_gen_item *, 2> fresh{nullptr, nullptr};         // everything is allocated before anything changes
    try {
        for (int i = 0; i < 2; ++i) if ((what >> i & 1) && !s.cap_item[(size_t)i]) fresh[(size_t)i] = gen_item_new();
    } catch (...) {
        for (rwkv_gen_item *it : fresh) gen_item_destroy(it);
        throw;
    }
    HIP_CHECK(hipStreamSynchronize(s_main));
    for (int i = 0; i < 2; ++i) {
        rwkv_gen_item *&it = s.cap_item[(size_t)i];
        if (fresh[(size_t)i]) { it = fresh[(size_t)i]; s.cap_taken &= ~(1u << i); s.cap_done &= ~(1u << i); }
        else if (!(what >> i & 1)) { gen_item_destroy(it); it = nullptr; s.cap_taken &= ~(1u << i); s.cap_done &= ~(1u << i); }
    }
    s.capture = what;
    gen_cap_upload(slot);
}
rwkv_gen_item *rwkv_engine::gen_take_item(int slot, unsigned which) {
    HIP_CHECK(hipSetDevice(device));
    if (which != RWKV_GEN_CAPTURE_PROMPT && which != RWKV_GEN_CAPTURE_FINISH) throw RwkvError(RWKV_ERR_INVALID, "`which` must be exactly one RWKV_GEN_CAPTURE_* bit");
    if (gen_slots.empty() || !(gen_slots[(size_t)slot].capture & which)) throw RwkvError(RWKV_ERR_INVALID, "the slot was not asked to capture this item");
    GenSlotHost &s = gen_slots[(size_t)slot];
    if (s.cap_taken & which) throw RwkvError(RWKV_ERR_INVALID, "the item was already taken");
    const int i = which == RWKV_GEN_CAPTURE_PROMPT ? 0 : 1;
    rwkv_gen_item *it = s.cap_item[(size_t)i];
    if (i == 0) {
        if (!(s.cap_done & which)) throw RwkvError(RWKV_ERR_INVALID, "the slot's prompt is not exhausted yet");
    } else {
        const int fin = s.g.finish;
        if (!fin) throw RwkvError(RWKV_ERR_INVALID, "the slot is still running");
        if (fin == RWKV_GEN_CANCELLED && s.prompt_left()) throw RwkvError(RWKV_ERR_INVALID, "the slot was cancelled inside its prompt: it never drew");
        // the state rule's state: gen_freeze kept it, the end of the run put it back into the slot, and nothing has run the slot since
        copy_state(it->st, slot_state(slot));
        HIP_CHECK(hipStreamSynchronize(s_main));
    }
    s.cap_item[(size_t)i] = nullptr;
    s.cap_taken |= which;
    try { gen_cap_upload(slot); } catch (...) { s.cap_item[(size_t)i] = it; s.cap_taken &= ~which; throw; }   // no step may write what the caller owns
    return it;
}
// rwkv_gen_arm_prompt for a prompt that is wholly cached: the slot takes the item's state, and the item's row waits in a buffer of the
// slot's own for the first step (gen_mixed_step), so the item may be freed as soon as this returns.
void rwkv_engine::gen_arm_item(int slot, const rwkv_gen_item *it, const rwkv_gen_params &p) {
    HIP_CHECK(hipSetDevice(device));
    if (!gen_item_fits(it)) throw RwkvError(RWKV_ERR_INVALID, "the item is null or was made for another device, model version or dimensions");
    // the refusals of rwkv_gen_arm, all as RWKV_ERR_INVALID: an item is a resident-only object, there is no other path to name
    try { gen_arm(slot, p, nullptr, 0, true); }
    catch (const RwkvError &err) { if (err.code == RWKV_ERR_UNSUPPORTED) throw RwkvError(RWKV_ERR_INVALID, err.what()); throw; }
    GenSlotHost &s = gen_slots[(size_t)slot];
    try {
        if (!s.inj_row) s.inj_row = dalloc<float>((size_t)info.num_vocab);
        HIP_CHECK(hipMemcpyAsync(s.inj_row, it->row, (size_t)it->V * 4, hipMemcpyDeviceToDevice, s_main));
        copy_state(slot_state(slot), it->st);
        s.inj = true;
        gen_cap_upload(slot);
    } catch (...) {
        gen_disarm_slot(slot);
        throw;
    }
}

// the non-null pointers of GenArgs say what the step's features (FEAT_*) are: gen_sample picks its launches from them
GenArgs rwkv_engine::gen_args(int n_rows, uint64_t feats) const {
    GenArgs a{};
    if (feats & FEAT_CAPTURE) a.cap = d_gen_cap;
    if (feats & FEAT_TOPN) {
        a.topn_n = d_gen_topn_n; a.top_ids = d_gen_top_ids; a.top_logp = d_gen_top_logp; a.tok_logp = d_gen_tok_logp;
        a.side_ms = d_gen_side_ms; a.side_rows = d_gen_side_rows;
    }
    if (feats & FEAT_STOPS) a.stops = d_gen_stop;
    if (feats & FEAT_DFA) { a.dfa = d_gen_dfa; a.tok_end = d_tok_end; }
    if (feats & FEAT_PDA) a.pda = d_gen_pda;
    if (feats & (FEAT_STOPS | FEAT_DFA | FEAT_PDA)) { a.tok_off = d_tok_off; a.tok_bytes = d_tok_bytes; a.n_tok = n_tok; }
    a.slots = d_gen; a.row_slot = dm.slot; a.logits = logits; a.penalty = d_gen_pen; a.bias = d_gen_bias;
    a.rows = d_gen_rows; a.samp_tok = d_gen_tok; a.samp_prob = d_gen_prob; a.feedback = d_tok_feedback;
    a.out_tok = d_gen_out; a.out_prob = (float *)(d_gen_out + (size_t)GEN_RING_STEPS * max_batch);
    a.run_step = d_gen_runstep; a.max_batch = max_batch; a.V = info.num_vocab; a.n_rows = n_rows;
    a.sxa = sxa; a.sxf = sxf; a.wkv = wkv; a.sx_slot_stride = sx_slot_stride; a.wkv_slot_stride = wkv_slot_stride;
    a.shadow = d_gen_shadow;
    if (feats & FEAT_WATCH) a.watch = d_gen_watch;
    return a;
}

// the sampler stage of a generation step over the a.n_rows rows of the logits block: the state machine around nucleus_kernel
void rwkv_engine::gen_sample(const GenArgs &a, unsigned needs) {
    if (a.cap) launch(FAM_COPY, [&] { launch_gen_capture(a, s_main); });   // the raw rows, like the top-n kernel's: in front of gen_pre
    if (a.topn_n) launch(FAM_SAMPLE, [&] { launch_gen_topn(a, s_main); });   // the raw rows: gen_pre edits the block in place
    launch(FAM_SAMPLE, [&] { launch_gen_pre(a, s_main); });
    if (a.dfa) launch(FAM_SAMPLE, [&] { launch_gen_mask(a, s_main); });   // `transform` (run.rs:676-679) of the constrained rows
    if (a.pda) launch(FAM_SAMPLE, [&] { launch_gen_pda_mask(a, s_main); });   // ... and of the rows under a stack constraint
    launch(FAM_SAMPLE, [&] { launch_nucleus(logits, a.n_rows, info.num_vocab, d_gen_rows, needs & NEEDS_NT, needs & NEEDS_MIRO, needs & NEEDS_WIDE, d_gen_tok, d_gen_prob, s_main); });
    launch(FAM_SAMPLE, [&] { launch_gen_post(a, s_main); });
    if (a.watch) launch(FAM_SAMPLE, [&] { launch_gen_publish(a, s_main); });   // behind gen_post (a slot's own reason stands), before gen_freeze (a cancel freezes here)
    launch(FAM_COPY, [&] { launch_gen_freeze(a, s_main); });
}

// one decode step of the rows of `pl` that feeds itself: forward pass on the feedback tokens, then the sampler stage
void rwkv_engine::gen_step(const StepPlan &pl, unsigned needs, uint64_t feats) {
    run_layers(pl.T, pl.n_seq, pl.n_out, d_tok_feedback, pl.dense);
    gen_sample(gen_args(pl.T, feats), needs);
}

// `n` decode-only steps of the slots `rows` (ascending): one captured graph per set of rows, fed from and handed back to d_gen_held
void rwkv_engine::gen_decode_steps(const std::vector<int> &rows, int n) {
    if ((int)rows.size() > chunk) throw RwkvError(RWKV_ERR_INVALID, "more armed slots than token_chunk_size");
    const unsigned needs = gen_needs(rows);
    const uint64_t feats = gen_feats(rows);
    // the step's plan: one token per row, every row emitted (the token ids come from the feedback buffer, not from the plan)
    StepPlan pl;
    plan_step(one_token_each(rows, nullptr).data(), pl);
    upload_plan(pl);
    step_max_rows = 1;
    launch_gen_handover(d_tok_feedback, d_gen_held, dm.slot, pl.T, false, s_main);
    const std::vector<uint64_t> key = gen_step_key(max_batch, rows, needs, feats);
    int s0 = 0;
    hipGraphExec_t *exec = gen_graphs.find(key);
    if (!exec) {
        // as in run_plan: a set of rows runs its first step directly, the steps after it go through the captured graph
        if (!gen_graphs.should_capture(key)) { gen_step(pl, needs, feats); s0 = 1; }
        if (s0 < n) exec = &gen_graphs.insert(key, capture(s_main, [&] { gen_step(pl, needs, feats); }));
    }
    for (int s = s0; s < n; ++s) HIP_CHECK(hipGraphLaunch(*exec, s_main));
    launch_gen_handover(d_tok_feedback, d_gen_held, dm.slot, pl.T, true, s_main);
}

// One MIXED step (rwkv_gen_arm_prompt): every slot of `dec` contributes its one feedback row, every slot of `pro` a share of what is
// left of the chunk (plan_step's water-filling: a pending count of 1 is always served first, so decode rows are never starved).  The
// logits block holds the decode rows and the last row of every prompt that ends here; the <true> kernels sample exactly those.  Runs
// uncaptured through the plan path, like the first step of a new row set: its shape is a one-off.
// A slot of `inj` (rwkv_gen_arm_item, its first step) consumes nothing: it has no step row, only a logits row behind the forward pass's,
// into which gen_inject copies its item's row; it takes one row of the chunk all the same.  With nothing but such slots the step runs
// no forward pass at all.
void rwkv_engine::gen_mixed_step(const std::vector<int> &dec, const std::vector<int> &pro, const std::vector<int> &inj, std::vector<int> &remain) {
    const int B = max_batch;
    // dec.size() < chunk: gen_run checked, before its first step, that all live slots together fit one chunk
    std::vector<rwkv_slot_input> in = one_token_each(dec, nullptr);
    for (int b : pro) in[(size_t)b] = rwkv_slot_input{gen_slots[(size_t)b].prompt.data() + gen_slots[(size_t)b].ppos, gen_prompt_left(b), RWKV_OPTION_LAST, 0};
    StepPlan pl;
    plan_step(in.data(), pl, (int)inj.size());
    for (int i = 0; i < pl.n_seq; ++i) if (!gen_prompt_left(pl.seq_slot[i])) pl.token[(size_t)pl.seq_begin[i]] = -1;   // a decode row; gen_tokens_kernel: held[slot]
    std::vector<int> drawn;                                        // the slots that sample here: every decode row, every prompt that ends, every item's row
    for (int b = 0; b < B; ++b) if (pl.slot_out_rows[(size_t)b]) drawn.push_back(b);
    drawn.insert(drawn.end(), inj.begin(), inj.end());
    uint64_t feats = gen_feats(drawn);
    for (int b : pro)                                              // the prompts that end here and are to be kept: complete once this step has run
        if (pl.slot_out_rows[(size_t)b] && (gen_slots[(size_t)b].capture & RWKV_GEN_CAPTURE_PROMPT)) { gen_slots[(size_t)b].cap_done |= RWKV_GEN_CAPTURE_PROMPT; feats |= FEAT_CAPTURE; }
    const int n_rows = pl.n_out + (int)inj.size();
    upload_plan(pl, inj);
    uploaded_id = 0;                                               // the uploaded token row is not the plan's: nobody may skip an upload on it
    launch(FAM_ROW, [&] { launch_gen_tokens(dm.token, dm.slot, d_gen_held, d_gen_runstep, pl.T, s_main); });
    step_max_rows = pl.max_rows();
    if (pl.T > 0) run_layers(pl.T, pl.n_seq, pl.n_out, dm.token, pl.dense);
    if (n_rows > 0) {
        GenArgs a = gen_args(n_rows, inj.empty() ? feats : feats | FEAT_CAPTURE);   // gen_inject reads a.cap as well
        a.out_rows = dm.out_rows;
        a.held = d_gen_held;
        if (!inj.empty()) launch(FAM_COPY, [&] { launch_gen_inject(a, pl.n_out, s_main); });
        if (!(feats & FEAT_CAPTURE)) a.cap = nullptr;              // gen_inject alone needed it
        gen_sample(a, gen_needs(drawn));
    } else if (gen_watch) {                                        // a step without a row still publishes its (all padding) record
        const GenArgs a = gen_args(0, FEAT_WATCH);
        launch(FAM_SAMPLE, [&] { launch_gen_publish(a, s_main); });
    }
    for (int b : dec) remain[(size_t)b] -= 1;
    for (int b : pro) {
        gen_slots[(size_t)b].ppos += (size_t)pl.slot_consumed[(size_t)b];
        if (pl.slot_out_rows[(size_t)b]) remain[(size_t)b] -= 1;      // the prompt ended: its last row was the slot's first draw
    }
    for (int b : inj) { gen_slots[(size_t)b].inj = false; remain[(size_t)b] -= 1; }
}

// n_top > 0 (rwkv_gen_run_topn): the three top-n outputs are filled as well, n_top places per step and slot.
void rwkv_engine::gen_run(int n_steps, uint32_t *out_tokens, float *out_probs, int32_t *n_emitted, int32_t *finish, int n_top, float *out_tok_logp,
                          uint32_t *out_top_ids, float *out_top_logp) {
    HIP_CHECK(hipSetDevice(device));
    (void)hipGetLastError();                                       // the poll behind the enqueue must only see this call's errors
    const int B = max_batch;
    const float nan = std::nanf("");
    if (n_top) {                                                   // refused before the first step, and before anything is written
        for (int b = 0; b < B; ++b)
            if (gen_is_live(b) && gen_slots[(size_t)b].topn > n_top)
                throw RwkvError(RWKV_ERR_INVALID, "slot " + std::to_string(b) + " lists " + std::to_string(gen_slots[(size_t)b].topn) + " places, n_top is " + std::to_string(n_top));
        std::fill(out_tok_logp, out_tok_logp + (size_t)n_steps * B, nan);
        std::fill(out_top_ids, out_top_ids + (size_t)n_steps * B * n_top, RWKV_TOPN_NONE);
        std::fill(out_top_logp, out_top_logp + (size_t)n_steps * B * n_top, nan);
    }
    std::fill(out_tokens, out_tokens + (size_t)n_steps * B, 0xFFFFFFFFu);
    if (out_probs) std::fill(out_probs, out_probs + (size_t)n_steps * B, nan);
    if (n_emitted) std::fill(n_emitted, n_emitted + B, 0);
    if (finish) std::fill(finish, finish + B, (int32_t)RWKV_GEN_RUNNING);
    const size_t ring = (size_t)GEN_RING_STEPS * B;
    for (int done = 0; done < n_steps && !gen_slots.empty();) {
        // One enqueue: up to a ring of steps with no wait in between.  The host knows which slots are in their prompt and when each
        // prompt ends (the plan says so); what it cannot know is who finished on the device, so a slot rides until the enqueue ends or
        // until it can emit nothing more (`remain`: max_tokens less what it has emitted for certain).
        const int nb = std::min(n_steps - done, (int)GEN_RING_STEPS);
        std::vector<int> live, remain((size_t)B, 0), cancelled;
        for (int b = 0; b < B; ++b) {
            GenSlotHost &s = gen_slots[(size_t)b];
            if (gen_watch && !s.armed && s.g.finish) {                 // a record shows 0 for a slot that is not armed: drop the word
                s.g.finish = RWKV_GEN_RUNNING;                         // its last request left behind (nothing else reads it)
                HIP_CHECK(hipMemsetAsync(&d_gen[b].finish, 0, sizeof(int), s_main));
            }
            if (!s.armed || s.g.finish) continue;
            live.push_back(b);
            remain[(size_t)b] = s.g.max_tokens - s.g.emitted;
        }
        if (live.empty()) break;
        // refused before anything is enqueued (a throw from the middle of an enqueue would lose the steps already run): every live slot
        // may become a decode row while a prompt is still pending, and a prompt needs a row of its own next to them
        if ((int)live.size() > chunk) throw RwkvError(RWKV_ERR_INVALID, "more armed slots than token_chunk_size");
        HIP_CHECK(hipMemsetAsync(d_gen_runstep, 0xFF, 4, s_main));                          // -1: the first kernel of a step counts up
        HIP_CHECK(hipMemsetAsync(d_gen_out, 0xFF, (size_t)nb * B * 4, s_main));             // 0xFFFFFFFF: nothing emitted
        HIP_CHECK(hipMemsetAsync(d_gen_out + ring, 0xFF, (size_t)nb * B * 4, s_main));      // ... and the same bits are a NaN
        const bool lists = gen_feats(live) & FEAT_TOPN;            // the top-n planes of the ring: RWKV_TOPN_NONE / NaN until a slot lists
        if (lists) {
            HIP_CHECK(hipMemsetAsync(d_gen_top_ids, 0xFF, (size_t)nb * B * TOPN_MAX * 4, s_main));
            HIP_CHECK(hipMemsetAsync(d_gen_top_logp, 0xFF, (size_t)nb * B * TOPN_MAX * 4, s_main));
            HIP_CHECK(hipMemsetAsync(d_gen_tok_logp, 0xFF, (size_t)nb * B * 4, s_main));
        }
        int k = 0;
        while (k < nb) {
            // A cancel word on a slot still INSIDE ITS PROMPT is the host's to see: the slot has no row a kernel could end.  It leaves
            // `live` here — it is planned no more, and the shadow restore below must not touch it: it was never frozen.
            for (size_t i = 0; gen_watch && i < live.size();) {
                const int b = live[i];
                if (gen_prompt_left(b) && gen_cancel_set(b)) { cancelled.push_back(b); live.erase(live.begin() + (long)i); }
                else ++i;
            }
            std::vector<int> dec, pro, inj;                        // ascending slot order
            for (int b : live) {
                if (gen_prompt_left(b)) pro.push_back(b);
                else if (gen_slots[(size_t)b].inj) inj.push_back(b);         // armed from an item: its first draw needs no forward row
                else if (remain[(size_t)b] > 0) dec.push_back(b);
            }
            if (!pro.empty() || !inj.empty()) {
                gen_mixed_step(dec, pro, inj, remain);
                k += 1;
                continue;
            }
            if (dec.empty()) break;
            int n = 0;
            for (int b : dec) n = std::max(n, remain[(size_t)b]);  // nobody runs longer than this
            n = std::min(n, nb - k);
            gen_decode_steps(dec, n);
            for (int b : dec) remain[(size_t)b] = std::max(0, remain[(size_t)b] - n);
            k += n;
        }
        HIP_CHECK(hipPeekAtLastError());                               // a failed launch is this call's error, not stale tokens with RWKV_OK
        if (k > 0) {
            HIP_CHECK(hipMemcpyAsync(h_gen_out, d_gen_out, (size_t)k * B * 4, hipMemcpyDeviceToHost, s_main));
            HIP_CHECK(hipMemcpyAsync(h_gen_out + ring, d_gen_out + ring, (size_t)k * B * 4, hipMemcpyDeviceToHost, s_main));
            if (lists && n_top) {
                HIP_CHECK(hipMemcpyAsync(h_gen_top_ids, d_gen_top_ids, (size_t)k * B * TOPN_MAX * 4, hipMemcpyDeviceToHost, s_main));
                HIP_CHECK(hipMemcpyAsync(h_gen_top_logp, d_gen_top_logp, (size_t)k * B * TOPN_MAX * 4, hipMemcpyDeviceToHost, s_main));
                HIP_CHECK(hipMemcpyAsync(h_gen_tok_logp, d_gen_tok_logp, (size_t)k * B * 4, hipMemcpyDeviceToHost, s_main));
            }
        }
        std::vector<GenSlot> back((size_t)B);
        HIP_CHECK(hipMemcpyAsync(back.data(), d_gen, (size_t)B * sizeof(GenSlot), hipMemcpyDeviceToHost, s_main));
        HIP_CHECK(hipStreamSynchronize(s_main));
        for (int b : cancelled) {                                  // the stream is idle (as where gen_set_topn writes its word); not in `live`: no restore
            const int fin = RWKV_GEN_CANCELLED;
            gen_slots[(size_t)b].g.finish = fin;
            HIP_CHECK(hipMemcpy(&d_gen[b].finish, &fin, sizeof(int), hipMemcpyHostToDevice));
        }
        if (k == 0) break;
        std::memcpy(out_tokens + (size_t)done * B, h_gen_out, (size_t)k * B * 4);
        if (out_probs) std::memcpy(out_probs + (size_t)done * B, h_gen_out + ring, (size_t)k * B * 4);
        // a step in which a slot emitted: its own n places, (RWKV_TOPN_NONE, -inf) up to the caller's stride; the rest keeps (NONE, NaN)
        for (int s = 0; n_top && s < k; ++s)
            for (int b : live) {
                const size_t cell = (size_t)s * B + (size_t)b, to = ((size_t)(done + s) * B + (size_t)b) * (size_t)n_top;
                if (h_gen_out[cell] == 0xFFFFFFFFu) continue;
                const int n = gen_slots[(size_t)b].topn;
                if (n) {
                    out_tok_logp[(size_t)(done + s) * B + (size_t)b] = h_gen_tok_logp[cell];
                    std::memcpy(out_top_ids + to, h_gen_top_ids + cell * TOPN_MAX, (size_t)n * 4);
                    std::memcpy(out_top_logp + to, h_gen_top_logp + cell * TOPN_MAX, (size_t)n * 4);
                }
                std::fill(out_top_logp + to + n, out_top_logp + to + n_top, -INFINITY);
            }
        bool restored = false;
        for (int b : live) {
            GenSlotHost &s = gen_slots[(size_t)b];
            const int got = back[(size_t)b].emitted - s.g.emitted;
            s.g = back[(size_t)b];
            if (n_emitted) n_emitted[b] += got;
            if (s.g.finish) {
                // the slot rode the steps behind the one it finished in: its state goes back to what it was there (the state rule)
                copy_state(slot_state(b), block_state(s.shadow));
                restored = true;
            }
        }
        if (restored) HIP_CHECK(hipStreamSynchronize(s_main));
        done += k;
    }
    if (finish) for (int b = 0; b < B; ++b) if (gen_is_armed(b)) finish[b] = gen_slots[(size_t)b].g.finish;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char *rwkv_last_error(void) { return g_err.c_str(); }
void rwkv_set_last_error(const char *msg) { g_err = msg ? msg : ""; }   // internal: the tokenizer TU reports through the same slot
int32_t rwkv_abi_version(void) { return RWKV_ABI_VERSION; }

int32_t rwkv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

rwkv_status rwkv_device_name(int32_t index, char *buf, size_t buf_len) {
    return guard([&] {
        if (!buf || !buf_len) throw RwkvError(RWKV_ERR_INVALID, "null buffer");
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        if (index < 0 || index >= n) throw RwkvError(RWKV_ERR_DEVICE, "adapter index out of range (ContextError::RequestAdapterFailed)");
        hipDeviceProp_t p;
        HIP_CHECK(hipGetDeviceProperties(&p, index));
        std::snprintf(buf, buf_len, "%s (%s, HIP)", p.name, p.gcnArchName);
    });
}

rwkv_status rwkv_model_info_from_st(const uint8_t *st_bytes, size_t st_len, rwkv_model_info *out) {
    return guard([&] {
        if (!out) throw RwkvError(RWKV_ERR_INVALID, "null out");
        if (prefab_sniff(st_bytes, st_len)) {                   // lib.rs:585-588: safetensors or prefab, by content
            // the whole entry table is walked (headers only: no payload byte is touched), so a truncated or corrupt image is
            // refused here, where a caller asks "what is this file", rather than halfway through a load
            const Prefab p = Prefab::parse(st_bytes, st_len);
            *out = p.hdr.info;
            return;
        }
        SafeTensors st = SafeTensors::parse(st_bytes, st_len);
        *out = detect_info(st);
    });
}

rwkv_status rwkv_engine_save_prefab(rwkv_engine *e, const char *path) {
    return guard([&] {
        if (!e || !path) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        e->save_prefab(path);
    });
}

rwkv_status rwkv_engine_create(const rwkv_load_desc *desc, rwkv_engine **out) {
    return guard([&] {
        if (!desc || !out || !desc->st_bytes) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        *out = nullptr;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
            throw RwkvError(RWKV_ERR_DEVICE, "no HIP device: librwkv_hip has no CPU fallback");
        if (desc->adapter < RWKV_ADAPTER_ECONOMICAL) throw RwkvError(RWKV_ERR_INVALID, "adapter must be RWKV_ADAPTER_AUTO, RWKV_ADAPTER_ECONOMICAL or a device index");
        int dev = desc->adapter >= 0 ? desc->adapter : 0;   // Auto / Economical: every MI355X is identical -> device 0
        if (dev >= n) throw RwkvError(RWKV_ERR_DEVICE, "adapter index out of range (ContextError::RequestAdapterFailed)");
        HIP_CHECK(hipSetDevice(dev));
        hipDeviceProp_t p;
        HIP_CHECK(hipGetDeviceProperties(&p, dev));
        if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
            throw RwkvError(RWKV_ERR_DEVICE, std::string("device is ") + p.gcnArchName + ", this library is built for gfx950 only");
        std::unique_ptr<rwkv_engine> e(new rwkv_engine());
        e->device = dev;
        e->load(*desc);
        *out = e.release();
    });
}

void rwkv_engine_destroy(rwkv_engine *e) { delete e; }

rwkv_status rwkv_engine_info(const rwkv_engine *e, rwkv_model_info *out) {
    return guard([&] {
        if (!e || !out) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        *out = e->info;
    });
}
int32_t rwkv_engine_device(const rwkv_engine *e) { return e ? e->device : -1; }
int32_t rwkv_engine_max_batch(const rwkv_engine *e) { return e ? e->max_batch : 0; }
int32_t rwkv_engine_token_chunk_size(const rwkv_engine *e) { return e ? e->chunk : 0; }
uint64_t rwkv_engine_weight_bytes(const rwkv_engine *e) { return e ? e->weight_bytes : 0; }

// Blocks handed out by rwkv_host_alloc, base -> bytes: the asynchronous read-back checks that the rows it is asked to write END inside the
// block they start in (a pinned block that is too small, or a large offset into it, must come back as RWKV_ERR_INVALID, not as a DMA
// over whatever follows the block in host memory).
static std::mutex g_host_mu;
static std::map<uintptr_t, size_t> g_host_blocks;
rwkv_status rwkv_host_alloc(size_t bytes, void **out) {
    return guard([&] {
        if (!out || bytes == 0) throw RwkvError(RWKV_ERR_INVALID, "bad arguments");
        void *p = nullptr;
        HIP_CHECK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        { std::lock_guard<std::mutex> g(g_host_mu); g_host_blocks[(uintptr_t)p] = bytes; }
        *out = p;
    });
}
void rwkv_host_free(void *p) {
    if (!p) return;
    { std::lock_guard<std::mutex> g(g_host_mu); g_host_blocks.erase((uintptr_t)p); }
    (void)hipHostFree(p);
}
// bytes from `p` to the end of the pinned block that holds it: from the registry above, else (memory the caller pinned itself) from the
// HIP runtime's address-range query; 0 = unknown
static size_t pinned_bytes_left(const void *p) {
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        auto it = g_host_blocks.upper_bound((uintptr_t)p);
        if (it != g_host_blocks.begin()) {
            --it;
            if ((uintptr_t)p < it->first + it->second) return it->first + it->second - (uintptr_t)p;
        }
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess && base && (uintptr_t)p >= (uintptr_t)base && (uintptr_t)p < (uintptr_t)base + size)
        return (uintptr_t)base + size - (uintptr_t)p;
    (void)hipGetLastError();
    return 0;
}

rwkv_status rwkv_infer(rwkv_engine *e, const rwkv_slot_input *in, rwkv_slot_output *out) {
    return guard([&] {
        if (!e || !in || !out) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        use_knobs(e->kn);
        e->infer(in, out);
    });
}

rwkv_status rwkv_infer_sample(rwkv_engine *e, const rwkv_slot_input *in, const rwkv_sample_params *sp, uint32_t *out_tokens,
                              float *out_probs, uint8_t *emitted, size_t *n_consumed) {
    return guard([&] {
        if (!e || !in || !sp || !out_tokens || !emitted) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        use_knobs(e->kn);
        e->infer_sample(in, sp, out_tokens, out_probs, emitted, n_consumed);
    });
}

rwkv_status rwkv_infer_score(rwkv_engine *e, const rwkv_slot_input *in, const uint32_t *const *targets, float *const *out_logp,
                             size_t *n_consumed) {
    return guard([&] {
        if (!e || !in || !targets || !n_consumed) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        use_knobs(e->kn);
        e->infer_score(in, targets, out_logp, n_consumed);
    });
}

rwkv_status rwkv_infer_topn(rwkv_engine *e, const rwkv_slot_input *in, int32_t n, uint32_t *const *out_ids, float *const *out_logp,
                            const uint32_t *const *targets, float *const *out_tok_logp, size_t *n_rows, size_t *n_consumed) {
    return guard([&] {
        if (!e || !in || !out_ids || !out_logp || !n_rows || !n_consumed) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        if (n < 1 || n > RWKV_TOPN_MAX) throw RwkvError(RWKV_ERR_INVALID, "n must be 1.." + std::to_string(RWKV_TOPN_MAX) + ", got " + std::to_string(n));
        use_knobs(e->kn);
        e->infer_topn(in, n, out_ids, out_logp, targets, out_tok_logp, n_rows, n_consumed);
    });
}

rwkv_status rwkv_plan_chunk(int32_t max_batch, int32_t token_chunk_size, const size_t *n_tokens, int32_t *consumed) {
    return guard([&] {
        if (max_batch <= 0 || token_chunk_size <= 0 || !n_tokens || !consumed) throw RwkvError(RWKV_ERR_INVALID, "bad arguments");
        std::vector<size_t> pending(n_tokens, n_tokens + max_batch);
        std::vector<int> take;
        water_fill(token_chunk_size, pending, take);
        for (int b = 0; b < max_batch; ++b) consumed[b] = take[b];
    });
}

const char *rwkv_profile_family_name(int32_t f) { return f >= 0 && f < RWKV_PROFILE_FAMILIES ? kFamilyNames[f] : ""; }

rwkv_status rwkv_profile_infer(rwkv_engine *e, const rwkv_slot_input *in, rwkv_slot_output *out, float *ms, int32_t *launches) {
    return guard([&] {
        if (!e || !in || !out || !ms) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        use_knobs(e->kn);
        std::fill(e->prof_ms, e->prof_ms + RWKV_PROFILE_FAMILIES, 0.f);
        std::fill(e->prof_n, e->prof_n + RWKV_PROFILE_FAMILIES, 0);
        e->profiling = true;
        e->prof_fam.clear();
        try {
            e->infer(in, out);
            e->prof_collect();
        } catch (...) {
            e->profiling = false;
            throw;
        }
        e->profiling = false;
        for (int i = 0; i < RWKV_PROFILE_FAMILIES; ++i) {
            ms[i] = e->prof_ms[i];
            if (launches) launches[i] = e->prof_n[i];
        }
    });
}

// ---- state ---------------------------------------------------------------------------------------
size_t rwkv_state_len(const rwkv_engine *e) { return e ? e->state_len() : 0; }
void rwkv_state_shape(const rwkv_engine *e, size_t shape[4]) {
    if (!e || !shape) return;
    shape[0] = (size_t)e->info.num_emb; shape[1] = 66; shape[2] = (size_t)e->info.num_layer; shape[3] = 1;
    if (e->info.version == 4) { shape[1] = 5 * (size_t)e->info.num_layer; shape[2] = 1; }   // web-rwkv's V4 state is [C, 5L, 1]
}
rwkv_status rwkv_state_init(const rwkv_engine *e, float *dst) {
    return guard([&] {
        if (!e || !dst) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        e->fill_init_state(dst);                            // v5/v6/v7: all-zero; v4: -1e30 in the pp rows
    });
}
static StatePackArgs pack_args(rwkv_engine *e, const rwkv_dstate &st, int to_slab, int layer_only) {
    StatePackArgs a{};
    a.slab = e->slab_dev; a.sxa = st.sxa; a.sxf = st.sxf; a.wkv = st.wkv;
    a.L = e->info.num_layer; a.C = e->info.num_emb; a.H = e->info.num_head;
    a.transposed = e->info.version != 7; a.to_slab = to_slab; a.layer_only = layer_only;
    a.v4 = e->info.version == 4;
    return a;
}
static void check_slot(const rwkv_engine *e, int slot) {
    if (!e) throw RwkvError(RWKV_ERR_INVALID, "null engine");
    if (slot < 0 || slot >= e->max_batch) throw RwkvError(RWKV_ERR_INVALID, "slot out of range");
}
rwkv_status rwkv_state_load(rwkv_engine *e, int32_t slot, const float *src) {
    return guard([&] {
        check_slot(e, slot);
        if (!src) throw RwkvError(RWKV_ERR_INVALID, "null src");
        HIP_CHECK(hipSetDevice(e->device));
        e->gen_disarm_slot(slot);
        const size_t n = rwkv_state_len(e);
        std::memcpy(e->slab_host, src, n * 4);
        HIP_CHECK(hipMemcpyAsync(e->slab_dev, e->slab_host, n * 4, hipMemcpyHostToDevice, e->s_main));
        launch_state_pack(pack_args(e, e->slot_state(slot), 0, -1), e->s_main);
        HIP_CHECK(hipStreamSynchronize(e->s_main));
    });
}
rwkv_status rwkv_state_back(rwkv_engine *e, int32_t slot, float *dst) {
    return guard([&] {
        check_slot(e, slot);
        if (!dst) throw RwkvError(RWKV_ERR_INVALID, "null dst");
        HIP_CHECK(hipSetDevice(e->device));
        const size_t n = rwkv_state_len(e);
        launch_state_pack(pack_args(e, e->slot_state(slot), 1, -1), e->s_main);
        HIP_CHECK(hipMemcpyAsync(e->slab_host, e->slab_dev, n * 4, hipMemcpyDeviceToHost, e->s_main));
        HIP_CHECK(hipStreamSynchronize(e->s_main));
        std::memcpy(dst, e->slab_host, n * 4);
    });
}
rwkv_status rwkv_state_back_layer(rwkv_engine *e, int32_t slot, int32_t layer, float *dst) {
    return guard([&] {
        check_slot(e, slot);
        if (!dst || layer < 0 || layer >= e->info.num_layer) throw RwkvError(RWKV_ERR_INVALID, "bad layer/dst");
        HIP_CHECK(hipSetDevice(e->device));
        const size_t n = (size_t)e->wkv_layer_floats();       // the layer's WKV rows: [64][C], V4 [3][C]
        launch_state_pack(pack_args(e, e->slot_state(slot), 1, layer), e->s_main);
        HIP_CHECK(hipMemcpyAsync(e->slab_host, e->slab_dev, n * 4, hipMemcpyDeviceToHost, e->s_main));
        HIP_CHECK(hipStreamSynchronize(e->s_main));
        std::memcpy(dst, e->slab_host, n * 4);
    });
}
rwkv_status rwkv_state_back_layer_async(rwkv_engine *e, int32_t slot, int32_t layer, float *dst) {
    return guard([&] {
        check_slot(e, slot);
        if (!dst || layer < 0 || layer >= e->info.num_layer) throw RwkvError(RWKV_ERR_INVALID, "bad layer/dst");
        HIP_CHECK(hipSetDevice(e->device));
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, dst) != hipSuccess || at.type != hipMemoryTypeHost) {
            (void)hipGetLastError();
            throw RwkvError(RWKV_ERR_INVALID, "rwkv_state_back_layer_async: dst must be pinned host memory (rwkv_host_alloc)");
        }
        const size_t n = (size_t)e->wkv_layer_floats();       // the layer's WKV rows: [64][C], V4 [3][C]
        {
            const size_t left = pinned_bytes_left(dst);
            if (left && left < n * 4) throw RwkvError(RWKV_ERR_INVALID, "rwkv_state_back_layer_async: the rows would end " + std::to_string(n * 4 - left) + " bytes past the pinned block that holds dst");
        }
        if (!e->s_copy) {
            HIP_CHECK(hipStreamCreateWithFlags(&e->s_copy, hipStreamNonBlocking));
            HIP_CHECK(hipEventCreateWithFlags(&e->ev_copy_a, hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&e->ev_copy_b, hipEventDisableTiming));
            HIP_CHECK(hipMalloc((void **)&e->emb_stage, (size_t)e->max_batch * n * 4));
        }
        // the pack reads the slot as the compute stream left it ...
        HIP_CHECK(hipEventRecord(e->ev_copy_a, e->s_main));
        HIP_CHECK(hipStreamWaitEvent(e->s_copy, e->ev_copy_a, 0));
        StatePackArgs a = pack_args(e, e->slot_state(slot), 1, layer);
        a.slab = e->emb_stage + (size_t)slot * n;                // per-slot staging: the copy stream is in order, so a slot's staging
        launch_state_pack(a, e->s_copy);                         // area is free again before its next pack runs
        // ... and whatever the compute stream does to the slot next waits for the pack (microseconds), not for the PCIe copy
        HIP_CHECK(hipEventRecord(e->ev_copy_b, e->s_copy));
        HIP_CHECK(hipStreamWaitEvent(e->s_main, e->ev_copy_b, 0));
        HIP_CHECK(hipMemcpyAsync(dst, a.slab, n * 4, hipMemcpyDeviceToHost, e->s_copy));
    });
}
rwkv_status rwkv_state_sync(rwkv_engine *e) {
    return guard([&] {
        if (!e) throw RwkvError(RWKV_ERR_INVALID, "null engine");
        HIP_CHECK(hipSetDevice(e->device));
        if (e->s_copy) HIP_CHECK(hipStreamSynchronize(e->s_copy));
    });
}
rwkv_status rwkv_state_read(rwkv_engine *e, int32_t slot, rwkv_dstate **snap) {
    return guard([&] {
        check_slot(e, slot);
        if (!snap) throw RwkvError(RWKV_ERR_INVALID, "null snap");
        HIP_CHECK(hipSetDevice(e->device));
        std::unique_ptr<rwkv_dstate> s(new rwkv_dstate());
        s->device = e->device;
        const size_t nsx = (size_t)e->sx_slot_stride * 4, nw = (size_t)e->wkv_slot_stride * 4;
        HIP_CHECK(hipMalloc((void **)&s->sxa, nsx));
        HIP_CHECK(hipMalloc((void **)&s->sxf, nsx));
        HIP_CHECK(hipMalloc((void **)&s->wkv, nw));
        e->copy_state(*s, e->slot_state(slot));
        HIP_CHECK(hipStreamSynchronize(e->s_main));
        *snap = s.release();
    });
}
rwkv_status rwkv_state_write(rwkv_engine *e, int32_t slot, const rwkv_dstate *s) {
    return guard([&] {
        check_slot(e, slot);
        if (!s) throw RwkvError(RWKV_ERR_INVALID, "null snap");
        HIP_CHECK(hipSetDevice(e->device));
        e->gen_disarm_slot(slot);
        e->copy_state(e->slot_state(slot), *s);
        HIP_CHECK(hipStreamSynchronize(e->s_main));
    });
}
void rwkv_dstate_free(rwkv_dstate *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipFree(s->sxa); (void)hipFree(s->sxf); (void)hipFree(s->wkv);
    delete s;
}

rwkv_status rwkv_read_init_state(const rwkv_engine *e, const uint8_t *st_bytes, size_t st_len, float *dst) {
    return guard([&] {
        if (!e || !dst) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        if (e->info.version == 4) throw RwkvError(RWKV_ERR_UNSUPPORTED, "v4 does not support init state yet");   // lib.rs:384
        SafeTensors st = SafeTensors::parse(st_bytes, st_len);
        const int L = e->info.num_layer, C = e->info.num_emb, H = e->info.num_head, N = 64;
        if (!st.find("blocks.0.att.time_state")) throw RwkvError(RWKV_ERR_NO_STATE, "no `time_state` tensors in file");
        std::memset(dst, 0, rwkv_state_len(e) * 4);
        for (int l = 0; l < L; ++l) {
            const StTensor &t = st.get("blocks." + std::to_string(l) + ".att.time_state");
            if (t.dtype != "F16" || t.numel() != (int64_t)H * N * N) throw RwkvError(RWKV_ERR_FORMAT, "bad time_state tensor");
            const _Float16 *ts = (const _Float16 *)t.data;     // stored [H][j][i] (converter transposed the last two dims)
            float *rows = dst + ((size_t)l * 66 + 1) * C;
            for (int h = 0; h < H; ++h)
                for (int j = 0; j < N; ++j)
                    for (int i = 0; i < N; ++i) rows[(size_t)i * C + h * N + j] = (float)ts[((size_t)h * N + j) * N + i];
        }
    });
}

// ---- softmax (second caller thread, own stream) ---------------------------------------------------
static std::mutex g_soft_mu;                                   // one softmax task per engine by contract; guard the staging rwkv_softmax and rwkv_score_rows share
rwkv_status rwkv_softmax(rwkv_engine *e, const float *const *in, float *const *out, size_t n_rows) {
    return guard([&] {
        if (!e || (n_rows && (!in || !out))) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        if (!n_rows) return;
        HIP_CHECK(hipSetDevice(e->device));
        const size_t V = (size_t)e->info.num_vocab;
        std::lock_guard<std::mutex> lk(g_soft_mu);
        // staging for max_batch rows is allocated at load (never from this thread: the allocator belongs to the infer
        // thread); larger requests are processed in groups
        for (size_t r0 = 0; r0 < n_rows; r0 += e->soft_rows_cap) {
            const size_t n = std::min(e->soft_rows_cap, n_rows - r0);
            for (size_t r = 0; r < n; ++r) {
                if (!in[r0 + r] || !out[r0 + r]) throw RwkvError(RWKV_ERR_INVALID, "null row");
                std::memcpy(e->soft_host + r * V, in[r0 + r], V * 4);
            }
            HIP_CHECK(hipMemcpyAsync(e->soft_in, e->soft_host, n * V * 4, hipMemcpyHostToDevice, e->s_soft));
            launch_softmax(e->soft_in, e->soft_out, (int)n, (int)V, e->s_soft);
            HIP_CHECK(hipMemcpyAsync(e->soft_host, e->soft_out, n * V * 4, hipMemcpyDeviceToHost, e->s_soft));
            HIP_CHECK(hipStreamSynchronize(e->s_soft));
            for (size_t r = 0; r < n; ++r) std::memcpy(out[r0 + r], e->soft_host + r * V, V * 4);
        }
    });
}

// ln softmax(row)[target] of host rows (the `head` term of Choose, run.rs:971-972): rwkv_softmax's staging, stream and thread rule; one float per
// row comes back instead of the row
rwkv_status rwkv_score_rows(rwkv_engine *e, const float *const *in, const uint32_t *targets, float *out_logp, size_t n_rows) {
    return guard([&] {
        if (!e || (n_rows && (!in || !targets || !out_logp))) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        if (!n_rows) return;
        const size_t V = (size_t)e->info.num_vocab;
        for (size_t r = 0; r < n_rows; ++r) {                  // before anything is written or launched
            if (!in[r]) throw RwkvError(RWKV_ERR_INVALID, "null row");
            if (targets[r] >= V && targets[r] != RWKV_SCORE_SKIP) throw RwkvError(RWKV_ERR_INVALID, "target " + std::to_string(targets[r]) + " is not a token of this vocabulary");
        }
        HIP_CHECK(hipSetDevice(e->device));
        std::lock_guard<std::mutex> lk(g_soft_mu);
        for (size_t r0 = 0; r0 < n_rows; r0 += e->soft_rows_cap) {
            const size_t n = std::min(e->soft_rows_cap, n_rows - r0);
            for (size_t r = 0; r < n; ++r) std::memcpy(e->soft_host + r * V, in[r0 + r], V * 4);
            std::memcpy(e->h_soft_tgt, targets + r0, n * 4);
            HIP_CHECK(hipMemcpyAsync(e->soft_in, e->soft_host, n * V * 4, hipMemcpyHostToDevice, e->s_soft));
            HIP_CHECK(hipMemcpyAsync(e->d_soft_tgt, e->h_soft_tgt, n * 4, hipMemcpyHostToDevice, e->s_soft));
            launch_score_rows(e->soft_in, e->d_soft_tgt, e->d_soft_score, (int)n, (int)V, e->s_soft);
            HIP_CHECK(hipMemcpyAsync(e->h_soft_score, e->d_soft_score, n * 4, hipMemcpyDeviceToHost, e->s_soft));
            HIP_CHECK(hipPeekAtLastError());
            HIP_CHECK(hipStreamSynchronize(e->s_soft));
            std::memcpy(out_logp + r0, e->h_soft_score, n * 4);
        }
    });
}

// the n most likely tokens of host rows with their ln-probabilities: rwkv_score_rows's staging, stream and thread rule; n ids and n floats per row
// come back instead of the row
rwkv_status rwkv_topn_rows(rwkv_engine *e, const float *const *in, int32_t n, uint32_t *out_ids, float *out_logp, size_t n_rows) {
    return guard([&] {
        if (!e || (n_rows && (!in || !out_ids || !out_logp))) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        if (n < 1 || n > RWKV_TOPN_MAX) throw RwkvError(RWKV_ERR_INVALID, "n must be 1.." + std::to_string(RWKV_TOPN_MAX) + ", got " + std::to_string(n));
        if (!n_rows) return;
        const size_t V = (size_t)e->info.num_vocab;
        for (size_t r = 0; r < n_rows; ++r)                    // before anything is written or launched
            if (!in[r]) throw RwkvError(RWKV_ERR_INVALID, "null row");
        HIP_CHECK(hipSetDevice(e->device));
        std::lock_guard<std::mutex> lk(g_soft_mu);
        for (size_t r0 = 0; r0 < n_rows; r0 += e->soft_rows_cap) {
            const size_t rows = std::min(e->soft_rows_cap, n_rows - r0), cells = rows * (size_t)n;
            for (size_t r = 0; r < rows; ++r) std::memcpy(e->soft_host + r * V, in[r0 + r], V * 4);
            HIP_CHECK(hipMemcpyAsync(e->soft_in, e->soft_host, rows * V * 4, hipMemcpyHostToDevice, e->s_soft));
            launch_topn_rows(e->soft_in, n, e->d_soft_topn_ids, e->d_soft_topn_logp, (int)rows, (int)V, e->s_soft);
            HIP_CHECK(hipMemcpyAsync(e->h_soft_topn_ids, e->d_soft_topn_ids, cells * 4, hipMemcpyDeviceToHost, e->s_soft));
            HIP_CHECK(hipMemcpyAsync(e->h_soft_topn_logp, e->d_soft_topn_logp, cells * 4, hipMemcpyDeviceToHost, e->s_soft));
            HIP_CHECK(hipPeekAtLastError());
            HIP_CHECK(hipStreamSynchronize(e->s_soft));
            std::memcpy(out_ids + r0 * n, e->h_soft_topn_ids, cells * 4);
            std::memcpy(out_logp + r0 * n, e->h_soft_topn_logp, cells * 4);
        }
    });
}

// ---- device-resident greedy decode ----------------------------------------------------------------
rwkv_status rwkv_decode_greedy(rwkv_engine *e, int32_t n_slots, const uint32_t *first_tokens, int32_t n_steps,
                               uint32_t *out_tokens, float *elapsed_ms) {
    return guard([&] {
        if (!e || !first_tokens || !out_tokens || n_slots <= 0 || n_slots > e->max_batch || n_slots > e->chunk || n_steps <= 0)
            throw RwkvError(RWKV_ERR_INVALID, "bad arguments");
        HIP_CHECK(hipSetDevice(e->device));
        use_knobs(e->kn);
        for (int b = 0; b < n_slots; ++b) e->gen_disarm_slot(b);
        StepPlan pl;
        std::vector<int> slots((size_t)n_slots);
        std::iota(slots.begin(), slots.end(), 0);
        e->plan_step(e->one_token_each(slots, first_tokens).data(), pl);
        e->upload_plan(pl);
        const size_t need = (size_t)n_steps * n_slots;
        if (need > e->hist_cap) {                                  // grow: the old buffer goes back (dalloc only frees at destroy)
            if (e->d_hist) {
                e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), (void *)e->d_hist), e->allocs.end());
                (void)hipFree(e->d_hist);
            }
            e->d_hist = e->dalloc<int>(need);
            e->hist_cap = need;
        }
        HIP_CHECK(hipMemcpyAsync(e->d_tok_feedback, first_tokens, n_slots * 4, hipMemcpyHostToDevice, e->s_main));
        HIP_CHECK(hipStreamSynchronize(e->s_main));
        // one graph = one decode step + arg-max feeding the next step's token ids on the device; kept per slot count (the plan of
        // "slots 0..n-1, one token each" is always the same and every buffer it names lives as long as the engine), so a
        // serving loop that calls this repeatedly pays capture + instantiation (~0.7 ms for 260 nodes) once
        hipGraphExec_t *exec = e->greedy_graphs->find(n_slots);
        if (!exec)
            exec = &e->greedy_graphs->insert(n_slots, capture(e->s_main, [&] {
                e->run_layers(pl.T, pl.n_seq, pl.n_out, e->d_tok_feedback, pl.dense);
                launch_argmax(e->logits, n_slots, e->info.num_vocab, e->d_tok_feedback, e->d_amax_v, e->d_amax_i, e->s_main);
            }));
        HIP_CHECK(hipEventRecord(e->ev0, e->s_main));
        for (int s = 0; s < n_steps; ++s) {
            HIP_CHECK(hipGraphLaunch(*exec, e->s_main));
            HIP_CHECK(hipMemcpyAsync(e->d_hist + (size_t)s * n_slots, e->d_tok_feedback, n_slots * 4, hipMemcpyDeviceToDevice, e->s_main));
        }
        HIP_CHECK(hipEventRecord(e->ev1, e->s_main));
        HIP_CHECK(hipEventSynchronize(e->ev1));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
        if (elapsed_ms) *elapsed_ms = ms;
        HIP_CHECK(hipMemcpy(out_tokens, e->d_hist, need * 4, hipMemcpyDeviceToHost));
    });
}

// ---- device-resident sampled generation ------------------------------------------------------------
rwkv_status rwkv_gen_arm(rwkv_engine *e, int32_t slot, const rwkv_gen_params *p) {
    return guard([&] {
        check_slot(e, slot);
        if (!p) throw RwkvError(RWKV_ERR_INVALID, "null params");
        use_knobs(e->kn);
        e->gen_arm(slot, *p, nullptr, 0);
    });
}
rwkv_status rwkv_gen_arm_prompt(rwkv_engine *e, int32_t slot, const uint32_t *tokens, size_t n_tokens, const rwkv_gen_params *p) {
    return guard([&] {
        check_slot(e, slot);
        if (!p) throw RwkvError(RWKV_ERR_INVALID, "null params");
        if (!tokens || n_tokens == 0) throw RwkvError(RWKV_ERR_INVALID, "a prompt needs at least one token");
        use_knobs(e->kn);
        e->gen_arm(slot, *p, tokens, n_tokens);
    });
}
rwkv_status rwkv_gen_prompt_left(const rwkv_engine *e, int32_t slot, size_t *left) {
    return guard([&] {
        check_slot(e, slot);
        if (!left) throw RwkvError(RWKV_ERR_INVALID, "null left");
        *left = e->gen_prompt_left(slot);
    });
}
rwkv_status rwkv_gen_disarm(rwkv_engine *e, int32_t slot) {
    return guard([&] {
        check_slot(e, slot);
        e->gen_disarm_slot(slot);
    });
}
rwkv_status rwkv_gen_run(rwkv_engine *e, int32_t n_steps, uint32_t *out_tokens, float *out_probs, int32_t *n_emitted, int32_t *finish) {
    return guard([&] {
        if (!e || !out_tokens || n_steps <= 0) throw RwkvError(RWKV_ERR_INVALID, "bad arguments");
        use_knobs(e->kn);
        e->gen_run(n_steps, out_tokens, out_probs, n_emitted, finish);
    });
}
// ---- captures and items ----
rwkv_status rwkv_gen_set_capture(rwkv_engine *e, int32_t slot, uint32_t what) {
    return guard([&] {
        check_slot(e, slot);
        e->gen_set_capture(slot, what);
    });
}
rwkv_status rwkv_gen_take_item(rwkv_engine *e, int32_t slot, uint32_t which, rwkv_gen_item **out) {
    return guard([&] {
        check_slot(e, slot);
        if (!out) throw RwkvError(RWKV_ERR_INVALID, "null out");
        *out = e->gen_take_item(slot, which);
    });
}
void rwkv_gen_item_free(rwkv_gen_item *it) { gen_item_destroy(it); }
const void *rwkv_gen_item_state(const rwkv_gen_item *it) { return it ? &it->st : nullptr; }
rwkv_status rwkv_gen_item_back(rwkv_engine *e, const rwkv_gen_item *it, float *state_dst, float *row_dst) {
    return guard([&] {
        if (!e) throw RwkvError(RWKV_ERR_INVALID, "null engine");
        if (!e->gen_item_fits(it)) throw RwkvError(RWKV_ERR_INVALID, "the item is null or was made for another device, model version or dimensions");
        HIP_CHECK(hipSetDevice(e->device));
        if (state_dst) {
            const size_t n = rwkv_state_len(e);
            launch_state_pack(pack_args(e, it->st, 1, -1), e->s_main);   // to_slab: the item is only read
            HIP_CHECK(hipMemcpyAsync(e->slab_host, e->slab_dev, n * 4, hipMemcpyDeviceToHost, e->s_main));
            HIP_CHECK(hipStreamSynchronize(e->s_main));
            std::memcpy(state_dst, e->slab_host, n * 4);
        }
        if (row_dst) HIP_CHECK(hipMemcpy(row_dst, it->row, (size_t)it->V * 4, hipMemcpyDeviceToHost));
    });
}
rwkv_status rwkv_gen_item_from_host(rwkv_engine *e, const float *state, const float *row, rwkv_gen_item **out) {
    return guard([&] {
        if (!e || !state || !row || !out) throw RwkvError(RWKV_ERR_INVALID, "null argument");
        HIP_CHECK(hipSetDevice(e->device));
        std::unique_ptr<rwkv_gen_item, void (*)(rwkv_gen_item *)> it(e->gen_item_new(), gen_item_destroy);
        const size_t n = rwkv_state_len(e);
        std::memcpy(e->slab_host, state, n * 4);
        HIP_CHECK(hipMemcpyAsync(e->slab_dev, e->slab_host, n * 4, hipMemcpyHostToDevice, e->s_main));
        launch_state_pack(pack_args(e, it->st, 0, -1), e->s_main);
        HIP_CHECK(hipStreamSynchronize(e->s_main));
        HIP_CHECK(hipMemcpy(it->row, row, (size_t)it->V * 4, hipMemcpyHostToDevice));
        *out = it.release();
    });
}
rwkv_status rwkv_gen_arm_item(rwkv_engine *e, int32_t slot, const rwkv_gen_item *it, const rwkv_gen_params *p) {
    return guard([&] {
        check_slot(e, slot);
        if (!p) throw RwkvError(RWKV_ERR_INVALID, "null params");
        use_knobs(e->kn);
        e->gen_arm_item(slot, it, *p);
    });
}
// ---- the watch: open / close on the infer thread between runs; head / read / cancel from ANY thread, on the watch's host block alone ----
rwkv_status rwkv_gen_watch_open(rwkv_engine *e, int32_t ring_steps, rwkv_gen_watch **out) {
    return guard([&] {
        if (!e || !out) throw RwkvError(RWKV_ERR_INVALID, "null engine / out");
        *out = nullptr;
        e->gen_watch_open(ring_steps, out);
    });
}
rwkv_status rwkv_gen_watch_close(rwkv_engine *e, rwkv_gen_watch *w) {
    return guard([&] {
        if (!e || !w) throw RwkvError(RWKV_ERR_INVALID, "null engine / watch");
        e->gen_watch_close(w);
    });
}
rwkv_status rwkv_gen_watch_head(const rwkv_gen_watch *w, uint64_t *seq) {
    return guard([&] {
        if (!w || !seq) throw RwkvError(RWKV_ERR_INVALID, "null watch / seq");
        *seq = gen_watch_head(w->ring, w->ring_steps, w->B);
    });
}
rwkv_status rwkv_gen_watch_read(rwkv_gen_watch *w, uint64_t *cursor, int32_t max_steps, uint32_t *tokens, float *probs, int32_t *finish,
                                int32_t *n_steps, uint64_t *lost) {
    return guard([&] {
        if (!w || !cursor || !tokens || !n_steps || !lost || max_steps < 0) throw RwkvError(RWKV_ERR_INVALID, "bad arguments");
        unsigned long long c = *cursor, l = 0;
        *n_steps = gen_watch_read(w->ring, w->ring_steps, w->B, &c, max_steps, tokens, (unsigned *)probs, finish, &l);
        *cursor = c; *lost = l;
    });
}
rwkv_status rwkv_gen_watch_cancel(rwkv_gen_watch *w, int32_t slot) {
    return guard([&] {
        if (!w) throw RwkvError(RWKV_ERR_INVALID, "null watch");
        if (slot < 0 || slot >= w->B) throw RwkvError(RWKV_ERR_INVALID, "slot out of range");
        __atomic_store_n(w->cancel() + slot, 1u, __ATOMIC_RELEASE);
    });
}
rwkv_status rwkv_gen_set_topn(rwkv_engine *e, int32_t slot, int32_t n) {
    return guard([&] {
        check_slot(e, slot);
        e->gen_set_topn(slot, n);
    });
}
rwkv_status rwkv_gen_run_topn(rwkv_engine *e, int32_t n_steps, uint32_t *out_tokens, float *out_probs, int32_t *n_emitted, int32_t *finish,
                              int32_t n_top, float *out_tok_logp, uint32_t *out_top_ids, float *out_top_logp) {
    return guard([&] {
        if (!e || !out_tokens || n_steps <= 0 || !out_tok_logp || !out_top_ids || !out_top_logp) throw RwkvError(RWKV_ERR_INVALID, "bad arguments");
        if (n_top < 1 || n_top > RWKV_TOPN_MAX) throw RwkvError(RWKV_ERR_INVALID, "n_top must be 1.." + std::to_string(RWKV_TOPN_MAX) + ", got " + std::to_string(n_top));
        use_knobs(e->kn);
        e->gen_run(n_steps, out_tokens, out_probs, n_emitted, finish, n_top, out_tok_logp, out_top_ids, out_top_logp);
    });
}
rwkv_status rwkv_gen_set_token_bytes(rwkv_engine *e, const uint8_t *bytes, const int32_t *lens, size_t n_tokens) {
    return guard([&] {
        if (!e) throw RwkvError(RWKV_ERR_INVALID, "null engine");
        e->gen_set_token_bytes(bytes, lens, n_tokens);
    });
}
rwkv_status rwkv_gen_set_stops(rwkv_engine *e, int32_t slot, const rwkv_gen_stops *s) {
    return guard([&] {
        check_slot(e, slot);
        if (!s) throw RwkvError(RWKV_ERR_INVALID, "null stops");
        e->gen_set_stops(slot, *s);
    });
}
rwkv_status rwkv_gen_stop_tail(rwkv_engine *e, int32_t slot, uint8_t *out, size_t cap, size_t *len) {
    return guard([&] {
        check_slot(e, slot);
        if (!len || (cap && !out)) throw RwkvError(RWKV_ERR_INVALID, "null out / len");
        *len = e->gen_stop_tail(slot, out, cap);
    });
}
rwkv_status rwkv_gen_set_constraint(rwkv_engine *e, int32_t slot, const rwkv_dfa *dfa, int32_t state, int32_t halt_mode) {
    return guard([&] {
        check_slot(e, slot);
        e->gen_set_constraint(slot, dfa, state, halt_mode);
    });
}
rwkv_status rwkv_gen_constraint_state(rwkv_engine *e, int32_t slot, int32_t *state) {
    return guard([&] {
        check_slot(e, slot);
        if (!state) throw RwkvError(RWKV_ERR_INVALID, "null state");
        *state = e->gen_constraint_state(slot);
    });
}
rwkv_status rwkv_gen_set_pda(rwkv_engine *e, int32_t slot, const rwkv_pda *pda, int32_t state, const uint16_t *stack, int32_t depth, int32_t halt_mode) {
    return guard([&] {
        check_slot(e, slot);
        e->gen_set_pda(slot, pda, state, stack, depth, halt_mode);
    });
}
rwkv_status rwkv_gen_pda_config(rwkv_engine *e, int32_t slot, int32_t *state, uint16_t *stack, size_t cap, int32_t *depth) {
    return guard([&] {
        check_slot(e, slot);
        if (!state || !depth || (cap && !stack)) throw RwkvError(RWKV_ERR_INVALID, "null state / depth / stack");
        e->gen_pda_config(slot, state, stack, cap, depth);
    });
}
rwkv_status rwkv_gen_uniform(uint64_t seed, uint32_t stream, uint32_t first_step, size_t n, float *out) {
    return guard([&] {
        if (n && !out) throw RwkvError(RWKV_ERR_INVALID, "null out");
        for (size_t i = 0; i < n; ++i) out[i] = gen_uniform_draw(seed, stream, first_step + (uint32_t)i);
    });
}

// ---- kernel microbench (measurement hook): one [rows x K] problem, `nmat` distinct weight copies rotated so
// that the 256 MiB Infinity Cache cannot serve re-reads; returns average microseconds per launch.
rwkv_status rwkv_bench_gemm(int32_t rows, int32_t K, int32_t fmt, int32_t T, int32_t hilo, int32_t spb, int32_t nmat,
                            int32_t iters, float *us_per_launch, float *lds_kib) {
    return guard([&] {
        if (rows % 16 || K % 256 || T < 1 || nmat < 1 || iters < 1 || iters > 2000 || fmt < W_F16 || fmt > W_SF4) throw RwkvError(RWKV_ERR_INVALID, "bad args");
        use_knobs(Knobs::from_env());                            // no engine here: the microbenchmark reads the environment per call
        hipStream_t st;
        HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        const size_t wbytes = fmt == W_F16 ? (size_t)rows * K * 2 : fmt == W_INT8 ? (size_t)rows * K : (size_t)rows * K / 2;   // NF4, SF4
        const size_t sbytes = fmt == W_F16 ? 16 : fmt == W_INT8 ? (size_t)rows * (K / 128) * 4 : (size_t)rows * (K / 64) * 2;
        std::vector<void *> bufs;
        auto dal = [&](size_t n) { void *p = nullptr; HIP_CHECK(hipMalloc(&p, n)); bufs.push_back(p); return p; };
        std::vector<DMat> mats(nmat);
        // Random operands (round 6): zero or constant fills let the chip clock higher than real data does (the micro-architecture guide measures
        // +15...21 % on a GEMM), so a zero-filled microbenchmark flatters every number it prints.  Weights: random bytes (fp16: random halfs of
        // magnitude < 2; quantised: random codes, scale words near 0.01); X: uniform halfs in [-1, 1).
        uint64_t rs = 0x9E3779B97F4A7C15ull;
        auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; };
        std::vector<uint16_t> hbuf(std::max(wbytes, sbytes) / 2 + 8);
        auto fill_halfs = [&](void *dst, size_t bytes, int kind) {      // 0: raw random bytes, 1: fp16 in (-2, 2), 2: fp16 scale ~0.01, 3: fp16 in [-1, 1)
            const size_t n = (bytes + 1) / 2;
            if (hbuf.size() < n) hbuf.resize(n);
            for (size_t j = 0; j < n; ++j) {
                const uint64_t r = rnd();
                hbuf[j] = kind == 0 ? (uint16_t)r : kind == 1 ? (uint16_t)((r & 0x8000) | (0x3000 + (r >> 20) % 0x1000))
                        : kind == 2 ? (uint16_t)(0x2100 + (r >> 20) % 0x100) : (uint16_t)((r & 0x8000) | (0x2C00 + (r >> 20) % 0x1000));
            }
            HIP_CHECK(hipMemcpy(dst, hbuf.data(), bytes, hipMemcpyHostToDevice));
        };
        for (int i = 0; i < nmat; ++i) {
            mats[i].data = dal(wbytes); mats[i].scales = dal(sbytes);
            if (i == 0) { fill_halfs((void *)mats[i].data, wbytes, fmt == W_F16 ? 1 : 0); fill_halfs((void *)mats[i].scales, sbytes, 2); }
            else {                                                       // the other copies: the same bytes rotated (device-to-device, cheap)
                const size_t rot = ((size_t)i * 4099 * 16) % wbytes & ~(size_t)15;
                HIP_CHECK(hipMemcpy((char *)mats[i].data, (const char *)mats[0].data + rot, wbytes - rot, hipMemcpyDeviceToDevice));
                if (rot) HIP_CHECK(hipMemcpy((char *)mats[i].data + (wbytes - rot), mats[0].data, rot, hipMemcpyDeviceToDevice));
                HIP_CHECK(hipMemcpy((void *)mats[i].scales, mats[0].scales, sbytes, hipMemcpyDeviceToDevice));
            }
            mats[i].fmt = fmt; mats[i].rows = rows; mats[i].K = K;
        }
        Opd x; x.ld = K;
        const size_t xcap = (size_t)((T + 15) / 16 * 16) * x.ld * 2;
        x.hi = (_Float16 *)dal(xcap); x.lo = (_Float16 *)dal(xcap);
        fill_halfs(x.hi, xcap, 3);
        HIP_CHECK(hipMemcpy(x.lo, x.hi, xcap, hipMemcpyDeviceToDevice));
        float *out = (float *)dal((size_t)T * rows * 4);
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
        std::vector<float *> parts;                                   // partial-sum target when K needs a block split
        float *pbuf = (float *)dal((size_t)8 * T * rows * 4);
        // RWKV_BENCH_DUAL=1 (dev): TWO dependent chains over the same matrices on two streams of one graph — what two half-batches
        // of a decode step would do (each chain's launch k streams matrix k; the chains are independent of each other)
        const bool dual = std::getenv("RWKV_BENCH_DUAL") && std::atoi(std::getenv("RWKV_BENCH_DUAL")) != 0;
        hipStream_t st2 = nullptr;
        Opd x2 = x;
        float *out2 = out, *pbuf2 = pbuf;
        if (dual) {
            HIP_CHECK(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
            x2.hi = (_Float16 *)dal(xcap); x2.lo = (_Float16 *)dal(xcap);
            HIP_CHECK(hipMemset(x2.hi, 0, xcap)); HIP_CHECK(hipMemset(x2.lo, 0, xcap));
            out2 = (float *)dal((size_t)T * rows * 4);
            pbuf2 = (float *)dal((size_t)8 * T * rows * 4);
        }
        const char *ks_env = std::getenv("RWKV_BENCH_KSPLIT");                 // (dev) K copies of a tile launch
        const int bench_ksplit = ks_env ? std::max(1, std::min(8, std::atoi(ks_env))) : 0;
        hipStream_t run_st = st;
        auto run = [&](int n) {
            const bool second = run_st != st;
            for (int i = 0; i < n; ++i) {
                ProbSpec ps;
                ps.W = &mats[i % nmat]; ps.x = second ? x2 : x; ps.out = K > 5120 ? (second ? pbuf2 : pbuf) : (second ? out2 : out); ps.ldo = rows;
                ps.partial = K > 5120;
                const ProbShape shp = shape_of(ps);
                GemmLaunch Lh;
                int shape = -1;
                if (T >= GEMM_TILE_MIN_T) {                      // prefill path; `spb` selects the tile shape (0..12), -1 = auto
                    shape = spb;
                    if (shape < 0 || shape >= GEMM_TILE_SHAPES) {
                        shape = GEMM_TILE3;
                        for (int sh = 0; sh < GEMM_TILE_SHAPES; ++sh) if (gemm_tile_blocks(sh, rows, T) >= 1024) { shape = sh; break; }
                    }
                    if (!gemm_tile_shape_supported(shape, hilo != 0, K)) throw RwkvError(RWKV_ERR_INVALID, "bench_gemm: the pipelined shapes need K % 128 == 0; shapes 10 / 11 take plain operands, shape 12 hi + lo");
                    if (bench_ksplit) ps.out = second ? pbuf2 : pbuf;            // K copies of the tile grid writing partial slabs (linear launches)
                    tile_geometry(Lh, &shp, 1, T, shape, std::max(1, bench_ksplit));
                    if (knobs().tile_xcd >= 0) Lh.xcd_map = knobs().tile_xcd;    // 2: token-tile-major bands
                } else if (!plan_decode(Lh, &shp, 1, T, hilo != 0, spb)) throw RwkvError(RWKV_ERR_UNSUPPORTED, "cannot split inner dimension");
                fill_prob(Lh.p[0], ps, (long)T * rows);
                if (lds_kib) *lds_kib = (float)Lh.total_blocks;
                if (shape >= 0) launch_gemm_tile(Lh, shape, hilo != 0, run_st);
                else launch_gemm(Lh, hilo != 0, run_st);
            }
        };
        run(nmat);
        HIP_CHECK(hipStreamSynchronize(st));
        hipEvent_t ev_fork = nullptr, ev_join = nullptr;
        if (dual) { HIP_CHECK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming)); HIP_CHECK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming)); }
        const hipGraphExec_t ge = capture(st, [&] {
            if (dual) {
                HIP_CHECK(hipEventRecord(ev_fork, st));
                HIP_CHECK(hipStreamWaitEvent(st2, ev_fork, 0));
                run_st = st2; run(iters); run_st = st;
                HIP_CHECK(hipEventRecord(ev_join, st2));
            }
            run(iters);
            if (dual) HIP_CHECK(hipStreamWaitEvent(st, ev_join, 0));
        });
        HIP_CHECK(hipGraphLaunch(ge, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipEventRecord(e0, st));
        HIP_CHECK(hipGraphLaunch(ge, st));
        HIP_CHECK(hipEventRecord(e1, st));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipGraphExecDestroy(ge);
        if (us_per_launch) *us_per_launch = ms * 1e3f / iters;
        for (void *p : bufs) (void)hipFree(p);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(st);
        if (dual) { (void)hipEventDestroy(ev_fork); (void)hipEventDestroy(ev_join); (void)hipStreamDestroy(st2); }
    });
}

}  // extern "C"

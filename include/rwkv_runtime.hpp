// rwkv_runtime.hpp — header-only C++17 mirror of the `web_rwkv` items ai00-core uses, on top of rwkv_abi.h.
// Same names and argument meaning as the reference's Rust call sites (crates/ai00-core/src):
//   Loader::info                    lib.rs:587            ModelBuilder(...).quant().lora().build()   lib.rs:484-516
//   Runtime::infer(RnnInput&)       run.rs:1143           RnnInput / RnnInputBatch / RnnOption        run.rs:1128-1132
//   State::{init,load,back,read,write}  run.rs:477,1099-1106     softmax(runtime, rows)               run.rs:1179
//   State::{embed,embed_async,sync}  the `/embeddings` read-back (docs/doc-api/openai.md:376-437): one layer's WKV rows of a slot
//   Tokenizer::{encode,decode}      run.rs:157,856
// Errors surface as rwkv::Error (std::runtime_error) carrying the rwkv_status — the analogue of `anyhow ?`.
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rwkv_abi.h"

namespace rwkv {

struct Error : std::runtime_error {
    rwkv_status code;
    Error(rwkv_status c) : std::runtime_error(std::string("rwkv: ") + rwkv_last_error()), code(c) {}
};
inline void check(rwkv_status s) { if (s != RWKV_OK) throw Error(s); }

enum class RnnOption : int32_t { Last = RWKV_OPTION_LAST, Full = RWKV_OPTION_FULL, None = RWKV_OPTION_NONE };
enum class Quant : int32_t { None = RWKV_QUANT_NONE, Int8 = RWKV_QUANT_INT8, NF4 = RWKV_QUANT_NF4, SF4 = RWKV_QUANT_SF4 };
// reload.rs:89-94; Fp16Raw is this library's extension (ABI 7): f16 operands on EVERY launch — the fastest mode, outside 1e-3 at 32 layers
enum class Precision : int32_t { Fp16 = RWKV_PRECISION_FP16, Fp32 = RWKV_PRECISION_FP32, Fp16Raw = RWKV_PRECISION_FP16_RAW };
using ModelInfo = rwkv_model_info;

struct Loader {
    static ModelInfo info(const uint8_t *st, size_t len) { ModelInfo i{}; check(rwkv_model_info_from_st(st, len, &i)); return i; }
};

struct RnnInputBatch {                      // RnnInputBatch::new(tokens, option)
    std::vector<uint32_t> tokens;
    RnnOption option = RnnOption::Last;
};
struct RnnInput {                           // RnnInput::new(batches, token_chunk_size)
    std::vector<RnnInputBatch> batches;
    size_t num_token() const { size_t n = 0; for (auto &b : batches) n += b.tokens.size(); return n; }
};
using RnnOutputBatch = std::vector<float>;  // n_rows * num_vocab floats (empty: nothing emitted)

// A byte-level DFA (rwkv_dfa): the REGULAR format constraint resident generation masks on the device (Runtime::gen_set_constraint) and the
// same `Formatter` (sampler/bnf.rs:34-48) for the per-token path (DfaFormatter, include/rwkv_sampler.hpp).  Not kbnf.  Host only.
class Dfa {
   public:
    static Dfa compile(const std::string &pattern) {
        rwkv_dfa *d = nullptr;
        check(rwkv_dfa_compile((const uint8_t *)pattern.data(), pattern.size(), &d));
        return Dfa(d);
    }
    static Dfa from_table(const std::vector<uint16_t> &trans, const std::vector<uint8_t> &accepting, int32_t start = 1) {
        if (trans.size() != accepting.size() * 256) throw std::invalid_argument("Dfa::from_table: 256 transitions per state");
        rwkv_dfa *d = nullptr;
        check(rwkv_dfa_from_table(trans.data(), accepting.data(), (int32_t)accepting.size(), start, &d));
        return Dfa(d);
    }
    int32_t num_states() const { return rwkv_dfa_num_states(d_.get()); }
    int32_t start() const { return rwkv_dfa_start(d_.get()); }
    int32_t walk(int32_t state, const uint8_t *bytes, size_t n) const {
        int32_t next = 0;
        check(rwkv_dfa_walk(d_.get(), state, bytes, n, &next));
        return next;
    }
    bool accepting(int32_t state) const {
        std::vector<uint8_t> acc((size_t)num_states());
        check(rwkv_dfa_table(d_.get(), nullptr, acc.data()));
        return state >= 0 && (size_t)state < acc.size() && acc[(size_t)state] != 0;
    }
    const rwkv_dfa *raw() const { return d_.get(); }

   private:
    explicit Dfa(rwkv_dfa *d) : d_(d, rwkv_dfa_free) {}
    std::shared_ptr<rwkv_dfa> d_;
};

// A byte automaton with a return-state stack (rwkv_pda): the NESTED format constraint resident generation masks on the device
// (Runtime::gen_set_pda) — Pda::json is RFC 8259, "answer in JSON" — and the same `Formatter` for the per-token path (allow).  A
// configuration is (state, stack).  Not kbnf: general context-free grammars keep the per-token path.  Host only.
class Pda {
   public:
    struct Config {
        int32_t state = 0;
        std::vector<uint16_t> stack;                 // bottom first
    };
    static Pda json(uint32_t flags = 0, int32_t max_depth = RWKV_PDA_MAX_DEPTH) {
        rwkv_pda *p = nullptr;
        check(rwkv_pda_json(flags, max_depth, &p));
        return Pda(p);
    }
    static Pda from_table(const std::vector<uint16_t> &next, const std::vector<uint16_t> &act, const std::vector<uint8_t> &accepting, int32_t start = 1,
                          int32_t max_depth = RWKV_PDA_MAX_DEPTH) {
        if (next.size() != accepting.size() * 256 || act.size() != next.size()) throw std::invalid_argument("Pda::from_table: two planes of 256 entries per state");
        rwkv_pda *p = nullptr;
        check(rwkv_pda_from_table(next.data(), act.data(), accepting.data(), (int32_t)accepting.size(), start, max_depth, &p));
        return Pda(p);
    }
    int32_t num_states() const { return rwkv_pda_num_states(p_.get()); }
    int32_t start() const { return rwkv_pda_start(p_.get()); }
    int32_t max_depth() const { return rwkv_pda_max_depth(p_.get()); }
    Config walk(const Config &from, const uint8_t *bytes, size_t n) const {
        Config to;
        to.stack.resize(RWKV_PDA_MAX_DEPTH);
        int32_t depth = 0;
        check(rwkv_pda_walk(p_.get(), from.state, from.stack.data(), (int32_t)from.stack.size(), bytes, n, &to.state, to.stack.data(), &depth));
        to.stack.resize((size_t)std::max(depth, 0));
        return to;
    }
    // the num_vocab-byte mask rwkv_sample_params.allow takes; `bytes` / `lens` as for Runtime::gen_set_token_bytes
    std::vector<uint8_t> allow(const Config &at, const uint8_t *bytes, const int32_t *lens, size_t n_tokens, size_t num_vocab) const {
        std::vector<uint8_t> out(num_vocab);
        check(rwkv_pda_allow(p_.get(), at.state, at.stack.data(), (int32_t)at.stack.size(), bytes, lens, n_tokens, out.data(), num_vocab));
        return out;
    }
    const rwkv_pda *raw() const { return p_.get(); }

   private:
    explicit Pda(rwkv_pda *p) : p_(p, rwkv_pda_free) {}
    std::shared_ptr<rwkv_pda> p_;
};

class Runtime;
class TensorGpu {                            // device-resident state snapshot (`state.read`)
   public:
    explicit TensorGpu(rwkv_dstate *h) : h_(h, rwkv_dstate_free) {}
    const rwkv_dstate *get() const { return h_.get(); }
   private:
    std::shared_ptr<rwkv_dstate> h_;         // clone == share, like the Rust `backed.clone()` (run.rs:962)
};

// float32 block in pinned host memory (rwkv_host_alloc): where asynchronous read-backs (State::embed_async) land
class PinnedBuffer {
   public:
    explicit PinnedBuffer(size_t n) : n_(n) {
        void *p = nullptr;
        check(rwkv_host_alloc((n ? n : 1) * sizeof(float), &p));
        p_.reset((float *)p, rwkv_host_free);
    }
    float *data() const { return p_.get(); }
    size_t size() const { return n_; }
   private:
    std::shared_ptr<float> p_;
    size_t n_;
};

class State {
   public:
    explicit State(rwkv_engine *e) : e_(e) {}
    std::vector<size_t> shape() const { std::vector<size_t> s(4); rwkv_state_shape(e_, s.data()); return s; }
    std::vector<float> init() const { std::vector<float> v(rwkv_state_len(e_)); check(rwkv_state_init(e_, v.data())); return v; }
    void load(const std::vector<float> &t, int batch) {
        if (t.size() != rwkv_state_len(e_)) throw std::invalid_argument("state tensor has the wrong size");
        check(rwkv_state_load(e_, batch, t.data()));
    }
    std::vector<float> back(int batch) { std::vector<float> v(rwkv_state_len(e_)); check(rwkv_state_back(e_, batch, v.data())); return v; }
    TensorGpu read(int batch) { rwkv_dstate *h = nullptr; check(rwkv_state_read(e_, batch, &h)); return TensorGpu(h); }
    void write(const TensorGpu &t, int batch) { check(rwkv_state_write(e_, batch, t.get())); }
    // one layer's WKV rows of a slot, [head_size][num_emb] floats (rwkv_state_shape = [C, N + 2, L, 1]: the N rows between the two
    // token-shift rows) — what `/embeddings` returns for the chosen layer.  V4 (state [C, 5L, 1, 1]): the layer's aa / bb / pp rows, [3][num_emb]
    size_t layer_len() const {
        rwkv_model_info i{};
        check(rwkv_engine_info(e_, &i));
        auto s = shape();
        return s[0] * (i.version == RWKV_V4 ? 3 : s[1] - 2);
    }
    void embed(int layer, int batch, float *dst) { check(rwkv_state_back_layer(e_, batch, layer, dst)); }
    // not waited for: `dst` is pinned memory (PinnedBuffer), valid after sync(); the slot may take its next request at once
    void embed_async(int layer, int batch, float *dst) { check(rwkv_state_back_layer_async(e_, batch, layer, dst)); }
    void sync() { check(rwkv_state_sync(e_)); }
   private:
    rwkv_engine *e_;
};

class Runtime {
   public:
    explicit Runtime(rwkv_engine *e) : e_(e, rwkv_engine_destroy), state(e) {
        check(rwkv_engine_info(e, &info));
        max_batch = rwkv_engine_max_batch(e);
        token_chunk_size = rwkv_engine_token_chunk_size(e);      // what the engine was built with: sizes the buffers of Full requests
    }
    // runtime.infer(input) -> output; `input` is consumed in place (tokens drained by n_consumed)
    std::vector<RnnOutputBatch> infer(RnnInput &input) {
        if ((int)input.batches.size() != max_batch) throw std::invalid_argument("RnnInput must have max_batch entries");
        std::vector<rwkv_slot_input> in(max_batch);
        std::vector<rwkv_slot_output> out(max_batch);
        std::vector<RnnOutputBatch> bufs(max_batch);
        for (int b = 0; b < max_batch; ++b) {
            auto &ib = input.batches[b];
            // one call emits at most token_chunk_size rows for a slot however long its pending token list is (an 8k-token Full
            // request must not allocate 8k x V floats per call); slots without tokens and state-only slots need no buffer
            const size_t rows = ib.tokens.empty() || ib.option == RnnOption::None ? 0
                               : ib.option == RnnOption::Full ? std::min(ib.tokens.size(), (size_t)token_chunk_size) : 1;
            bufs[b].resize(rows * (size_t)info.num_vocab);
            in[b] = rwkv_slot_input{ib.tokens.data(), ib.tokens.size(), (int32_t)ib.option, 0};
            out[b] = rwkv_slot_output{rows ? bufs[b].data() : nullptr, rows, 0, 0};
        }
        check(rwkv_infer(e_.get(), in.data(), out.data()));
        for (int b = 0; b < max_batch; ++b) {
            auto &t = input.batches[b].tokens;
            t.erase(t.begin(), t.begin() + (long)out[b].n_consumed);
            bufs[b].resize(out[b].n_rows * (size_t)info.num_vocab);
        }
        return bufs;
    }
    // rwkv_infer_sample: the on-device sampling front-end.  Slots whose pending tokens this call exhausts get a
    // sampled token instead of a logits row; `sp[b]` comes from a host-side sampler (include/rwkv_sampler.hpp).  `input` is
    // consumed in place like infer().
    struct Sampled { bool emitted = false; uint32_t token = 0; float prob = 0.f; };
    std::vector<Sampled> infer_sample(RnnInput &input, const std::vector<rwkv_sample_params> &sp) {
        if ((int)input.batches.size() != max_batch || (int)sp.size() != max_batch) throw std::invalid_argument("infer_sample: need max_batch entries");
        std::vector<rwkv_slot_input> in((size_t)max_batch);
        for (int b = 0; b < max_batch; ++b) {
            auto &ib = input.batches[(size_t)b];
            in[(size_t)b] = rwkv_slot_input{ib.tokens.data(), ib.tokens.size(), (int32_t)RnnOption::Last, 0};
        }
        std::vector<uint32_t> tok((size_t)max_batch);
        std::vector<float> prob((size_t)max_batch);
        std::vector<uint8_t> emitted((size_t)max_batch);
        std::vector<size_t> consumed((size_t)max_batch);
        check(rwkv_infer_sample(e_.get(), in.data(), sp.data(), tok.data(), prob.data(), emitted.data(), consumed.data()));
        std::vector<Sampled> out((size_t)max_batch);
        for (int b = 0; b < max_batch; ++b) {
            auto &t = input.batches[(size_t)b].tokens;
            t.erase(t.begin(), t.begin() + (long)consumed[(size_t)b]);
            out[(size_t)b] = Sampled{emitted[(size_t)b] != 0, tok[(size_t)b], prob[(size_t)b]};
        }
        return out;
    }
    // rwkv_infer_score: one step like infer(), for slots that are scored instead of read (perplexity run.rs:699-755, Choose run.rs:936-982).
    // Slot b is scored when `targets[b]` holds one target per pending token (targets[b][i] — a token id or RWKV_SCORE_SKIP — is scored on
    // the row that consuming tokens[b][i] produces); a slot with no targets must have no tokens or RnnOption::None.  `input` and `targets`
    // are consumed in place; returns per slot the ln-probabilities of the rows this call consumed (NaN where skipped).  No row crosses PCIe.
    std::vector<std::vector<float>> infer_score(RnnInput &input, std::vector<std::vector<uint32_t>> &targets) {
        if ((int)input.batches.size() != max_batch || (int)targets.size() != max_batch) throw std::invalid_argument("infer_score: need max_batch entries");
        std::vector<rwkv_slot_input> in((size_t)max_batch);
        std::vector<const uint32_t *> tp((size_t)max_batch, nullptr);
        std::vector<float *> op((size_t)max_batch, nullptr);
        std::vector<std::vector<float>> out((size_t)max_batch);
        std::vector<size_t> consumed((size_t)max_batch);
        for (size_t b = 0; b < (size_t)max_batch; ++b) {
            auto &ib = input.batches[b];
            in[b] = rwkv_slot_input{ib.tokens.data(), ib.tokens.size(), (int32_t)ib.option, 0};
            if (targets[b].empty()) continue;
            if (targets[b].size() != ib.tokens.size()) throw std::invalid_argument("infer_score: a scored slot needs one target per pending token");
            out[b].resize(std::min(ib.tokens.size(), (size_t)token_chunk_size));
            tp[b] = targets[b].data();
            op[b] = out[b].data();
        }
        check(rwkv_infer_score(e_.get(), in.data(), tp.data(), op.data(), consumed.data()));
        for (size_t b = 0; b < (size_t)max_batch; ++b) {
            auto &t = input.batches[b].tokens;
            t.erase(t.begin(), t.begin() + (long)consumed[b]);
            if (!tp[b]) continue;
            targets[b].erase(targets[b].begin(), targets[b].begin() + (long)consumed[b]);
            out[b].resize(consumed[b]);
        }
        return out;
    }
    // rwkv_score_rows: ln softmax(rows[i])[targets[i]] of host rows on the device (RWKV_SCORE_SKIP -> NaN) — Choose's `head` term (run.rs:971-972).
    // The softmax task's stream and thread, like softmax() below.
    std::vector<float> score_rows(const std::vector<std::vector<float>> &rows, const std::vector<uint32_t> &targets) {
        if (rows.size() != targets.size()) throw std::invalid_argument("score_rows: one target per row");
        for (const auto &r : rows) if (r.size() != (size_t)info.num_vocab) throw std::invalid_argument("score_rows: every row must hold num_vocab values");
        std::vector<const float *> pi(rows.size());
        for (size_t i = 0; i < rows.size(); ++i) pi[i] = rows[i].data();
        std::vector<float> out(rows.size());
        check(rwkv_score_rows(e_.get(), pi.data(), targets.data(), out.data(), rows.size()));
        return out;
    }
    // Top-n lists (rwkv_topn_rows / rwkv_infer_topn): `rows` lists of `n` places; ids[r * n + i] / logp[r * n + i] are the i-th most likely
    // token of row r and its ln-probability (logits descending, ties to the lower id; RWKV_TOPN_NONE / -inf where the row has fewer than n
    // entries above -inf, RWKV_TOPN_NONE / NaN on a row holding +inf or NaN); tok_logp[r] is the realised token's ln-probability where the
    // slot had targets.  Every logp is score_rows()'s value for that row and id, bit for bit.
    struct TopLists { int n = 0; size_t rows = 0; std::vector<uint32_t> ids; std::vector<float> logp, tok_logp; };
    // The softmax task's stream and thread, like score_rows().
    TopLists topn_rows(const std::vector<std::vector<float>> &rows, int n) {
        for (const auto &r : rows) if (r.size() != (size_t)info.num_vocab) throw std::invalid_argument("topn_rows: every row must hold num_vocab values");
        std::vector<const float *> pi(rows.size());
        for (size_t i = 0; i < rows.size(); ++i) pi[i] = rows[i].data();
        const size_t cells = n > 0 ? rows.size() * (size_t)n : 0;
        TopLists out{n, rows.size(), std::vector<uint32_t>(cells, RWKV_TOPN_NONE), std::vector<float>(cells), {}};
        check(rwkv_topn_rows(e_.get(), pi.data(), n, out.ids.data(), out.logp.data(), rows.size()));
        return out;
    }
    // One step like infer(), with lists instead of rows: every slot that has tokens and an option other than RnnOption::None lists and keeps
    // its option (Last: one list when the call exhausts its tokens, Full: one per consumed token).  `targets` is empty, or max_batch entries
    // of which targets[b] is empty or holds one target per pending token of a Full slot (a token id or RWKV_SCORE_SKIP): the realised token
    // is scored on its row exactly as infer_score() does.  `input` and `targets` are consumed in place.  No row crosses PCIe.
    std::vector<TopLists> infer_topn(RnnInput &input, int n, std::vector<std::vector<uint32_t>> &targets) {
        if ((int)input.batches.size() != max_batch || (!targets.empty() && (int)targets.size() != max_batch)) throw std::invalid_argument("infer_topn: need max_batch entries");
        if (n < 1 || n > RWKV_TOPN_MAX) throw std::invalid_argument("infer_topn: n must be 1..RWKV_TOPN_MAX");
        std::vector<rwkv_slot_input> in((size_t)max_batch);
        std::vector<uint32_t *> ip((size_t)max_batch, nullptr);
        std::vector<float *> lp((size_t)max_batch, nullptr), op((size_t)max_batch, nullptr);
        std::vector<const uint32_t *> tp((size_t)max_batch, nullptr);
        std::vector<TopLists> out((size_t)max_batch);
        std::vector<size_t> n_rows((size_t)max_batch), consumed((size_t)max_batch);
        for (size_t b = 0; b < (size_t)max_batch; ++b) {
            auto &ib = input.batches[b];
            in[b] = rwkv_slot_input{ib.tokens.data(), ib.tokens.size(), (int32_t)ib.option, 0};
            out[b].n = n;
            const size_t rows = ib.tokens.empty() || ib.option == RnnOption::None ? 0
                               : ib.option == RnnOption::Full ? std::min(ib.tokens.size(), (size_t)token_chunk_size) : 1;
            if (!rows) continue;
            out[b].ids.assign(rows * (size_t)n, RWKV_TOPN_NONE);
            out[b].logp.resize(rows * (size_t)n);
            ip[b] = out[b].ids.data();
            lp[b] = out[b].logp.data();
            if (targets.empty() || targets[b].empty()) continue;
            if (targets[b].size() != ib.tokens.size()) throw std::invalid_argument("infer_topn: a scored slot needs one target per pending token");
            out[b].tok_logp.resize(rows);
            tp[b] = targets[b].data();
            op[b] = out[b].tok_logp.data();
        }
        check(rwkv_infer_topn(e_.get(), in.data(), n, ip.data(), lp.data(), targets.empty() ? nullptr : tp.data(), targets.empty() ? nullptr : op.data(),
                              n_rows.data(), consumed.data()));
        for (size_t b = 0; b < (size_t)max_batch; ++b) {
            auto &t = input.batches[b].tokens;
            t.erase(t.begin(), t.begin() + (long)consumed[b]);
            out[b].rows = n_rows[b];
            out[b].ids.resize(n_rows[b] * (size_t)n);
            out[b].logp.resize(n_rows[b] * (size_t)n);
            if (!tp[b]) continue;
            targets[b].erase(targets[b].begin(), targets[b].begin() + (long)consumed[b]);
            out[b].tok_logp.resize(n_rows[b]);
        }
        return out;
    }
    // Device-resident sampled generation (rwkv_gen_arm / _run / _disarm): arm a slot with `sampler.gen_params_for(...)`
    // (include/rwkv_sampler.hpp), then every gen_run generates up to n_steps tokens per armed slot without a host turn-around.
    void gen_arm(int slot, const rwkv_gen_params &p) { check(rwkv_gen_arm(e_.get(), slot, &p)); }
    // Admission (rwkv_gen_arm_prompt): `p` from `sampler.gen_params_for_prompt(...)`, i.e. after init(prompt) and before any update;
    // the prompt's tail rides in the resident steps and its first token is drawn on the device.
    void gen_arm_prompt(int slot, const std::vector<uint32_t> &tokens, const rwkv_gen_params &p) {
        check(rwkv_gen_arm_prompt(e_.get(), slot, tokens.data(), tokens.size(), &p));
    }
    size_t gen_prompt_left(int slot) const {
        size_t left = 0;
        check(rwkv_gen_prompt_left(e_.get(), slot, &left));
        return left;
    }
    void gen_disarm(int slot) { check(rwkv_gen_disarm(e_.get(), slot)); }
    // Stop strings on the device (rwkv_gen_set_token_bytes / _set_stops / _stop_tail; run.rs:855-869, 899-932, 990-1011).  `table[i]` is what
    // `tokenizer.decode(&[i])` yields; `known[i] == 0` marks an id that is not in the vocabulary (decode error: empty word and stop).
    void gen_set_token_bytes(const std::vector<std::string> &table, const std::vector<uint8_t> &known = {}) {
        std::vector<int32_t> lens(table.size());
        std::string bytes;
        for (size_t i = 0; i < table.size(); ++i) {
            const bool ok = known.empty() || known[i];
            lens[i] = ok ? (int32_t)table[i].size() : -1;
            if (ok) bytes += table[i];
        }
        check(rwkv_gen_set_token_bytes(e_.get(), (const uint8_t *)bytes.data(), lens.data(), lens.size()));
    }
    // the strings of an armed, unfinished slot; `tail` is StopMatcher::tail() of the caller's own matcher (include/rwkv_scheduler.hpp)
    void gen_set_stops(int slot, const std::vector<std::string> &stops, const std::vector<uint8_t> &tail = {}) {
        std::vector<const uint8_t *> strs(stops.size());
        std::vector<size_t> lens(stops.size());
        for (size_t i = 0; i < stops.size(); ++i) { strs[i] = (const uint8_t *)stops[i].data(); lens[i] = stops[i].size(); }
        const rwkv_gen_stops s{strs.data(), lens.data(), stops.size(), tail.data(), tail.size()};
        check(rwkv_gen_set_stops(e_.get(), slot, &s));
    }
    std::vector<uint8_t> gen_stop_tail(int slot) {
        std::vector<uint8_t> out(RWKV_GEN_STOP_BUF);
        size_t len = 0;
        check(rwkv_gen_stop_tail(e_.get(), slot, out.data(), out.size(), &len));
        out.resize(std::min(len, out.size()));
        return out;
    }
    // The format constraint of an armed, unfinished slot (rwkv_gen_set_constraint; `Formatter`, run.rs:676-680, 892-897, 990), next to its
    // stop strings: masked, advanced and halted on the device.  `state`: dfa.start() after gen_arm_prompt; after gen_arm the state behind
    // first_token (DfaFormatter::state after its update).  Needs the token table (gen_set_token_bytes).
    void gen_set_constraint(int slot, const Dfa &dfa, int32_t state, int32_t halt_mode = RWKV_DFA_HALT_FINAL) {
        check(rwkv_gen_set_constraint(e_.get(), slot, dfa.raw(), state, halt_mode));
    }
    void gen_clear_constraint(int slot) { check(rwkv_gen_set_constraint(e_.get(), slot, nullptr, 0, 0)); }
    // the state behind every token the slot has emitted: what a caller that goes on per token hands its DfaFormatter
    int32_t gen_constraint_state(int slot) {
        int32_t state = 0;
        check(rwkv_gen_constraint_state(e_.get(), slot, &state));
        return state;
    }
    // The stack constraint of an armed, unfinished slot (rwkv_gen_set_pda): masked, committed and halted on the device.  `at`: {pda.start(), {}}
    // after gen_arm_prompt; the caller's own configuration after gen_arm or a hand-over.  A slot holds a Dfa or a Pda, not both.
    void gen_set_pda(int slot, const Pda &pda, const Pda::Config &at, int32_t halt_mode = RWKV_PDA_HALT_FINAL) {
        check(rwkv_gen_set_pda(e_.get(), slot, pda.raw(), at.state, at.stack.data(), (int32_t)at.stack.size(), halt_mode));
    }
    void gen_clear_pda(int slot) { check(rwkv_gen_set_pda(e_.get(), slot, nullptr, 0, nullptr, 0, 0)); }
    // the configuration behind every token the slot has emitted: what a caller that goes on per token starts its own formatter from
    Pda::Config gen_pda_config(int slot) {
        Pda::Config c;
        c.stack.resize(RWKV_PDA_MAX_DEPTH);
        int32_t depth = 0;
        check(rwkv_gen_pda_config(e_.get(), slot, &c.state, c.stack.data(), c.stack.size(), &depth));
        c.stack.resize((size_t)std::max(depth, 0));
        return c;
    }
    struct Generated {
        std::vector<uint32_t> tokens;                // [n_steps][max_batch], 0xFFFFFFFF where a slot emitted nothing
        std::vector<float> probs;                    // same shape, NaN there
        std::vector<int32_t> n_emitted, finish;      // [max_batch]: tokens of this call, RWKV_GEN_* (RWKV_GEN_HANDBACK: replay StopMatcher, go on per token)
        // gen_run(n_steps, top > 0) only: the emitted token's raw ln-probability [n_steps][max_batch] (NaN where nothing was emitted or the slot
        // lists nothing) and the lists [n_steps][max_batch][n_top] (RWKV_TOPN_NONE / -inf behind a slot's own n, RWKV_TOPN_NONE / NaN where nothing was emitted)
        int n_top = 0;
        std::vector<float> tok_logp, top_logp;
        std::vector<uint32_t> top_ids;
    };
    // An armed, unfinished slot lists its n (0 .. RWKV_TOPN_MAX; 0 = off) most likely tokens of the RAW model row with every token it emits
    // from now on (rwkv_gen_set_topn); re-arming the slot resets it.
    void gen_set_topn(int slot, int n) { check(rwkv_gen_set_topn(e_.get(), slot, n)); }
    // `top` > 0 (rwkv_gen_run_topn; `top` >= every armed slot's n): tok_logp / top_ids / top_logp of the result are filled as well.
    Generated gen_run(int n_steps, int top = 0) {
        if (n_steps <= 0) throw std::invalid_argument("gen_run: n_steps must be > 0");
        Generated g;
        g.tokens.resize((size_t)n_steps * (size_t)max_batch);
        g.probs.resize(g.tokens.size());
        g.n_emitted.resize((size_t)max_batch);
        g.finish.resize((size_t)max_batch);
        if (top <= 0) {
            check(rwkv_gen_run(e_.get(), n_steps, g.tokens.data(), g.probs.data(), g.n_emitted.data(), g.finish.data()));
            return g;
        }
        g.n_top = top;
        g.tok_logp.resize(g.tokens.size());
        g.top_ids.resize(g.tokens.size() * (size_t)top);
        g.top_logp.resize(g.top_ids.size());
        check(rwkv_gen_run_topn(e_.get(), n_steps, g.tokens.data(), g.probs.data(), g.n_emitted.data(), g.finish.data(), top, g.tok_logp.data(),
                                g.top_ids.data(), g.top_logp.data()));
        return g;
    }
    // A watch on the engine's resident generation (rwkv_gen_watch_*): while one thread sits in gen_run, ANOTHER reads every step's record
    // as it ends (read, head) and cancels slots (cancel) — no HIP call, no lock, the device never waits.  RAII: the destructor closes the
    // watch, on the thread that runs the engine and between runs; it keeps the engine alive.  One reader per Cursor.
    class GenWatch {
       public:
        struct Records {
            int n = 0;                                   // records returned
            uint64_t lost = 0;                           // records skipped in this call: the reader fell more than ring_steps behind
            std::vector<uint32_t> tokens;                // [n][max_batch]: the rows of gen_run's outputs, 0xFFFFFFFF where a slot emitted nothing
            std::vector<float> probs;                    // same shape, NaN there
            std::vector<int32_t> finish;                 // same shape: RWKV_GEN_* after the step
        };
        GenWatch(std::shared_ptr<rwkv_engine> e, int max_batch, int ring_steps) : e_(std::move(e)), max_batch_(max_batch) {
            check(rwkv_gen_watch_open(e_.get(), ring_steps, &w_));
        }
        GenWatch(const GenWatch &) = delete;
        GenWatch &operator=(const GenWatch &) = delete;
        ~GenWatch() { if (w_) (void)rwkv_gen_watch_close(e_.get(), w_); }
        uint64_t head() const { uint64_t s = 0; check(rwkv_gen_watch_head(w_, &s)); return s; }
        Records read(uint64_t &cursor, int max_steps) {
            Records r;
            const size_t cells = (size_t)std::max(max_steps, 0) * (size_t)max_batch_;
            r.tokens.resize(cells); r.probs.resize(cells); r.finish.resize(cells);
            int32_t n = 0;
            check(rwkv_gen_watch_read(w_, &cursor, std::max(max_steps, 0), r.tokens.data(), r.probs.data(), r.finish.data(), &n, &r.lost));
            r.n = n;
            r.tokens.resize((size_t)n * (size_t)max_batch_); r.probs.resize(r.tokens.size()); r.finish.resize(r.tokens.size());
            return r;
        }
        void cancel(int slot) { check(rwkv_gen_watch_cancel(w_, slot)); }
        rwkv_gen_watch *raw() const { return w_; }
       private:
        std::shared_ptr<rwkv_engine> e_;
        rwkv_gen_watch *w_ = nullptr;
        int max_batch_ = 0;
    };
    std::unique_ptr<GenWatch> gen_watch_open(int ring_steps) { return std::make_unique<GenWatch>(e_, max_batch, ring_steps); }
    // A cached (state, raw logits row) pair on the device (rwkv_gen_item; CachedItem, run.rs:201-223): what a slot captures at its prompt's
    // end or when it finishes, and what gen_arm_item starts a slot from.  Immutable; clone == share, like TensorGpu; the last copy frees it.
    // It outlives the Runtime that made it; back() wants a Runtime of the same device, model version and dimensions.
    class GenItem {
       public:
        struct Host { std::vector<float> state, row; };   // `state` as State::back lays it out, `row` num_vocab floats
        explicit GenItem(rwkv_gen_item *h) : h_(h, rwkv_gen_item_free) {}
        static GenItem from_host(const Runtime &rt, const std::vector<float> &state, const std::vector<float> &row) {
            if (state.size() != rwkv_state_len(rt.raw()) || row.size() != (size_t)rt.info.num_vocab) throw Error(RWKV_ERR_INVALID);
            rwkv_gen_item *h = nullptr;
            check(rwkv_gen_item_from_host(rt.raw(), state.data(), row.data(), &h));
            return GenItem(h);
        }
        Host back(const Runtime &rt) const {
            Host o{std::vector<float>(rwkv_state_len(rt.raw())), std::vector<float>((size_t)rt.info.num_vocab)};
            check(rwkv_gen_item_back(rt.raw(), h_.get(), o.state.data(), o.row.data()));
            return o;
        }
        // the item's state into a slot (rwkv_state_write of rwkv_gen_item_state): a PARTIAL prefix hit, continued with gen_arm_prompt
        void write_state(const Runtime &rt, int batch) const {
            check(rwkv_state_write(rt.raw(), batch, static_cast<const rwkv_dstate *>(rwkv_gen_item_state(h_.get()))));
        }
        const rwkv_gen_item *get() const { return h_.get(); }
       private:
        std::shared_ptr<rwkv_gen_item> h_;
    };
    // what an armed, unfinished slot keeps for the prefix cache, between runs: RWKV_GEN_CAPTURE_PROMPT | RWKV_GEN_CAPTURE_FINISH, 0 clears
    void gen_set_capture(int slot, uint32_t what) { check(rwkv_gen_set_capture(e_.get(), slot, what)); }
    // `which` is exactly one bit: PROMPT once the run that exhausted the prompt has returned, FINISH once the slot has finished; each once
    GenItem gen_take_item(int slot, uint32_t which) {
        rwkv_gen_item *h = nullptr;
        check(rwkv_gen_take_item(e_.get(), slot, which, &h));
        return GenItem(h);
    }
    // gen_arm_prompt for a prompt that is wholly cached (run.rs:809-810): `p` as for gen_arm_prompt; the first token is drawn on the device
    // from the item's row in the slot's first step, which consumes nothing
    void gen_arm_item(int slot, const GenItem &item, const rwkv_gen_params &p) { check(rwkv_gen_arm_item(e_.get(), slot, item.get(), &p)); }
    rwkv_engine *raw() const { return e_.get(); }
    ModelInfo info{};
    int max_batch = 0;
    int token_chunk_size = 128;                  // tokens one infer call consumes at most (bounds the rows of a Full request)
   private:
    std::shared_ptr<rwkv_engine> e_;
   public:
    State state;
};

class ModelBuilder {
   public:
    ModelBuilder(const uint8_t *st, size_t len, int adapter = RWKV_ADAPTER_AUTO) { d_.st_bytes = st; d_.st_len = len; d_.adapter = adapter; }
    ModelBuilder &quant(int layers, Quant q) { d_.quant_layers = layers; d_.quant_type = (int32_t)q; return *this; }
    ModelBuilder &lora(const uint8_t *st, size_t len, float alpha) { lora_.push_back({st, len, alpha}); return *this; }
    Runtime build(int max_batch = 8, int token_chunk_size = 128, Precision p = Precision::Fp16) {
        d_.max_batch = max_batch; d_.token_chunk_size = token_chunk_size; d_.precision = (int32_t)p;
        d_.lora = lora_.empty() ? nullptr : lora_.data(); d_.n_lora = lora_.size();
        rwkv_engine *e = nullptr;
        check(rwkv_engine_create(&d_, &e));
        return Runtime(e);
    }
   private:
    rwkv_load_desc d_{};
    std::vector<rwkv_lora_desc> lora_;
};

inline std::vector<std::vector<float>> softmax(Runtime &rt, const std::vector<std::vector<float>> &rows) {
    for (const auto &r : rows)                    // rwkv_softmax reads num_vocab floats per row: a short row would be read out of bounds
        if (r.size() != (size_t)rt.info.num_vocab) throw std::invalid_argument("softmax: every row must hold num_vocab values");
    std::vector<std::vector<float>> out(rows.size());
    std::vector<const float *> pi(rows.size());
    std::vector<float *> po(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) { out[i].resize(rows[i].size()); pi[i] = rows[i].data(); po[i] = out[i].data(); }
    check(rwkv_softmax(rt.raw(), pi.data(), po.data(), rows.size()));
    return out;
}

class Tokenizer {
   public:
    explicit Tokenizer(const std::string &vocab_json) {
        rwkv_tokenizer *t = nullptr;
        check(rwkv_tokenizer_create(vocab_json.data(), vocab_json.size(), &t));
        t_.reset(t, rwkv_tokenizer_destroy);
    }
    std::vector<uint32_t> encode(const std::string &text) const {
        int64_t n = rwkv_tokenizer_encode(t_.get(), (const uint8_t *)text.data(), text.size(), nullptr, 0);
        if (n < 0) throw Error((rwkv_status)n);
        std::vector<uint32_t> v((size_t)n);
        rwkv_tokenizer_encode(t_.get(), (const uint8_t *)text.data(), text.size(), v.data(), v.size());
        return v;
    }
    std::string decode(const std::vector<uint32_t> &toks) const {
        int64_t n = rwkv_tokenizer_decode(t_.get(), toks.data(), toks.size(), nullptr, 0);
        if (n < 0) throw Error((rwkv_status)n);
        std::string s((size_t)n, '\0');
        rwkv_tokenizer_decode(t_.get(), toks.data(), toks.size(), (uint8_t *)s.data(), s.size());
        return s;
    }
   private:
    std::shared_ptr<rwkv_tokenizer> t_;
};

}  // namespace rwkv

// rwkv_sampler.hpp — host-side STATE of ai00-core's samplers (crates/ai00-core/src/sampler/*.rs) for the on-device sampling
// front-end (rwkv_infer_sample).  The device does what `Sampler::sample` does to a probability row (sort,
// top-k, top-p / tau / max_surprise, temperature, inverse CDF); what survives on the host is what the reference keeps between
// tokens:
//   NucleusSampler   nucleus.rs:13-122    penalty map: init (:49-59), transform (:61-67), the update at the end of sample (:104-119)
//   TypicalSampler   typical.rs:11-140    the same penalty state machine (:47-58, :62-68, :122-133); tau / top_k / temperature
//   MirostatSampler  mirostat.rs:11-90    max_surprise, updated from the token surprise the device returns (:85-87)
// `params_for()` fills the rwkv_sample_params of one slot: `-penalty` (transform) and `bias` (run.rs:681-683) merged into one
// sparse adjustment list, plus the uniform draw `fastrand::f32()` would make.  All arithmetic is f32, as in the reference.
// `gen_params_for()` hands the same state to the DEVICE instead (rwkv_gen_arm, ABI 8): after `init()` over the prompt it fills a
// rwkv_gen_params with the sampler's settings, the penalty map as it stands (positive values: the device negates them like `transform`)
// and the bias, so that the slot is armed with the map the host would have had.
// `gen_params_for_prompt()` is the same hand-over for rwkv_gen_arm_prompt (ABI 9): call it right after `init()`, BEFORE the first
// `update()` — the device draws the first token itself and runs that update there.
// Header-only; needs rwkv_abi.h only for the structs.
#pragma once
#include <cmath>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "rwkv_abi.h"

namespace rwkv {

struct SamplerAdjust {                 // keeps the arrays rwkv_sample_params points into alive until the call returns
    std::vector<uint32_t> tokens;
    std::vector<float> values;
};

struct GenArrays {                     // keeps the arrays rwkv_gen_params points into alive until rwkv_gen_arm returns (it copies them)
    std::vector<uint32_t> penalty_tokens, bias_tokens, stop_tokens;
    std::vector<float> penalty_values, bias_values;
};

// The reference's `Formatter` trait (sampler/bnf.rs:34-48) over a byte-level DFA (rwkv_dfa_*), for the per-token path: `transform`
// yields the mask rwkv_sample_params.allow takes (run.rs:676-679), `update` advances and says whether the request halts (run.rs:892-897,
// 990).  The same automaton runs on the device under rwkv_gen_set_constraint; `state` is what the two paths hand each other
// (rwkv_gen_constraint_state in one direction, the `state` argument of rwkv_gen_set_constraint in the other).  REGULAR constraints only:
// the reference's kbnf is another implementation of the trait.  The token table is the one rwkv_gen_set_token_bytes takes.
class DfaFormatter {
   public:
    DfaFormatter(const rwkv_dfa *dfa, std::vector<uint8_t> token_bytes, std::vector<int32_t> token_lens, size_t num_vocab,
                 int32_t halt_mode = RWKV_DFA_HALT_FINAL)
        : state(rwkv_dfa_start(dfa)), dfa_(dfa), bytes_(std::move(token_bytes)), lens_(std::move(token_lens)), allow_(num_vocab), halt_(halt_mode) {
        const size_t n = (size_t)rwkv_dfa_num_states(dfa);
        trans_.resize(n * 256);
        accepting_.resize(n);
        rwkv_dfa_table(dfa, trans_.data(), accepting_.data());
        off_.resize(lens_.size() + 1, 0);
        for (size_t i = 0; i < lens_.size(); ++i) off_[i + 1] = off_[i] + (lens_[i] > 0 ? (size_t)lens_[i] : 0);
    }
    int32_t state;                     // the state behind every token handled so far
    // the mask of the current state; valid until the next call
    const uint8_t *transform() {
        rwkv_dfa_allow(dfa_, state, bytes_.data(), lens_.data(), lens_.size(), allow_.data(), allow_.size());
        return allow_.data();
    }
    // a token that is not allowed (id 0, an empty or unknown token, bytes that kill the walk) leaves the state and does not halt (bnf.rs:44)
    bool update(uint32_t token) {
        if (token == 0 || token >= lens_.size() || lens_[token] <= 0) return false;
        int32_t end = 0;
        if (rwkv_dfa_walk(dfa_, state, bytes_.data() + off_[token], (size_t)lens_[token], &end) != RWKV_OK || end == 0) return false;
        state = end;
        if (!accepting_[(size_t)end]) return false;
        if (halt_ == RWKV_DFA_HALT_ACCEPT) return true;
        for (int c = 0; c < 256; ++c) if (trans_[(size_t)end * 256 + (size_t)c]) return false;
        return true;
    }

   private:
    const rwkv_dfa *dfa_;
    std::vector<uint8_t> bytes_;
    std::vector<int32_t> lens_;
    std::vector<size_t> off_;
    std::vector<uint16_t> trans_;
    std::vector<uint8_t> accepting_, allow_;
    int32_t halt_;
};

class NucleusSampler {
   public:
    float top_p = 0.5f;                // NucleusParams defaults, nucleus.rs:13-26
    int32_t top_k = 128;
    float temperature = 1.0f, presence_penalty = 0.3f, frequency_penalty = 0.3f, penalty_decay = 0.99654026f;
    std::map<uint32_t, float> penalties;             // NucleusState (a HashMap there; ordered here so adjustment lists are deterministic)
    std::map<uint32_t, float> bias;                  // GenerateRequest::bias (run.rs:681-683)

    virtual ~NucleusSampler() = default;
    // nucleus.rs:49-59: walk the prompt backwards, the most recent token first
    void init(const std::vector<uint32_t> &model_tokens) {
        float index = 0.f;
        for (auto it = model_tokens.rbegin(); it != model_tokens.rend(); ++it, index += 1.f) {
            auto f = penalties.find(*it);
            float penalty = f == penalties.end() ? presence_penalty : f->second;
            penalty += frequency_penalty * std::pow(penalty_decay, index);
            penalties[*it] = penalty;
        }
    }
    // what `transform` (nucleus.rs:61-67) and the bias loop (run.rs:681-683) add to the logits, duplicates merged
    SamplerAdjust adjustments() const {
        std::map<uint32_t, float> adj;
        for (auto &kv : penalties) adj[kv.first] = -kv.second;
        for (auto &kv : bias) adj[kv.first] += kv.second;
        SamplerAdjust a;
        for (auto &kv : adj) { a.tokens.push_back(kv.first); a.values.push_back(kv.second); }
        return a;
    }
    // the tail of `sample` (nucleus.rs:104-119) with the token the device picked
    void update(uint32_t token) {
        for (auto &kv : penalties) kv.second *= penalty_decay;
        auto f = penalties.find(token);
        penalties[token] = f == penalties.end() ? presence_penalty : f->second + frequency_penalty;
    }
    virtual rwkv_sample_params params_for(float uniform, const SamplerAdjust &adj, const uint8_t *allow = nullptr) const {
        return rwkv_sample_params{top_p, top_k, temperature, uniform, adj.tokens.empty() ? nullptr : adj.tokens.data(),
                                  adj.values.empty() ? nullptr : adj.values.data(), adj.tokens.size(), RWKV_SAMPLER_NUCLEUS, 0.f, allow};
    }
    // the slot's generation context for rwkv_gen_arm: this sampler's settings and its penalty map / bias as they stand now
    virtual rwkv_gen_params gen_params_for(uint32_t first_token, int32_t max_tokens, uint64_t seed, uint32_t stream, GenArrays &keep,
                                           const std::vector<uint32_t> &stop_tokens = {}) const {
        keep = GenArrays{};
        for (auto &kv : penalties) { keep.penalty_tokens.push_back(kv.first); keep.penalty_values.push_back(kv.second); }
        for (auto &kv : bias) { keep.bias_tokens.push_back(kv.first); keep.bias_values.push_back(kv.second); }
        keep.stop_tokens = stop_tokens;
        rwkv_gen_params p{};
        p.first_token = first_token; p.max_tokens = max_tokens; p.kind = RWKV_SAMPLER_NUCLEUS;
        p.top_p = top_p; p.top_k = top_k; p.temperature = temperature;
        p.reserved = top_k > 256 ? RWKV_GEN_WIDE_TOP_K : 0u;        // any top_k, as nucleus.rs:78 / typical.rs:93 take it: the wide kernel's rows
        p.presence_penalty = presence_penalty; p.frequency_penalty = frequency_penalty; p.penalty_decay = penalty_decay;
        p.penalty_tokens = keep.penalty_tokens.empty() ? nullptr : keep.penalty_tokens.data();
        p.penalty_values = keep.penalty_values.empty() ? nullptr : keep.penalty_values.data();
        p.n_penalty = keep.penalty_tokens.size();
        p.bias_tokens = keep.bias_tokens.empty() ? nullptr : keep.bias_tokens.data();
        p.bias_values = keep.bias_values.empty() ? nullptr : keep.bias_values.data();
        p.n_bias = keep.bias_tokens.size();
        p.stop_tokens = keep.stop_tokens.empty() ? nullptr : keep.stop_tokens.data();
        p.n_stop = keep.stop_tokens.size();
        p.seed = seed; p.stream = stream;
        return p;
    }
    // for rwkv_gen_arm_prompt: the map as `init` left it, no first token (the device draws it)
    rwkv_gen_params gen_params_for_prompt(int32_t max_tokens, uint64_t seed, uint32_t stream, GenArrays &keep,
                                          const std::vector<uint32_t> &stop_tokens = {}) const {
        return gen_params_for(0, max_tokens, seed, stream, keep, stop_tokens);
    }
};

class TypicalSampler : public NucleusSampler {       // typical.rs: TypicalParams defaults tau 0.5, top_k 128, temperature 1.0
   public:
    float tau = 0.5f;
    rwkv_sample_params params_for(float uniform, const SamplerAdjust &adj, const uint8_t *allow = nullptr) const override {
        rwkv_sample_params p = NucleusSampler::params_for(uniform, adj, allow);
        p.top_p = 0.f;
        p.kind = RWKV_SAMPLER_TYPICAL;
        p.tau = tau;
        return p;
    }
    rwkv_gen_params gen_params_for(uint32_t first_token, int32_t max_tokens, uint64_t seed, uint32_t stream, GenArrays &keep,
                                   const std::vector<uint32_t> &stop_tokens = {}) const override {
        rwkv_gen_params p = NucleusSampler::gen_params_for(first_token, max_tokens, seed, stream, keep, stop_tokens);
        p.top_p = 0.f;
        p.kind = RWKV_SAMPLER_TYPICAL;
        p.tau = tau;
        return p;
    }
};

class MirostatSampler {                              // mirostat.rs:11-36: tau (target surprise) 3.0, rate 0.1, max_surprise starts at 2 tau
   public:
    explicit MirostatSampler(float tau = 3.0f, float rate_ = 0.1f) : target(tau), rate(rate_), max_surprise(2.0f * tau) {}
    float target, rate, max_surprise;
    void init(const std::vector<uint32_t> &) {}      // mirostat.rs:38
    SamplerAdjust adjustments() const { return {}; } // transform is a no-op (mirostat.rs:40)
    // mirostat.rs:85-87 with the token surprise rwkv_infer_sample returns in out_probs
    void update(float token_surprise) {
        const float error = token_surprise - target;
        max_surprise = std::fmin(max_surprise - rate * error, 4.0f * target);
    }
    rwkv_sample_params params_for(float uniform, const SamplerAdjust &, const uint8_t *allow = nullptr) const {
        return rwkv_sample_params{0.f, 1, 1.0f, uniform, nullptr, nullptr, 0, RWKV_SAMPLER_MIROSTAT, max_surprise, allow};
    }
    // the device carries max_surprise on from its current value (mirostat.rs:85-87 run there)
    rwkv_gen_params gen_params_for(uint32_t first_token, int32_t max_tokens, uint64_t seed, uint32_t stream, GenArrays &keep,
                                   const std::vector<uint32_t> &stop_tokens = {}) const {
        keep = GenArrays{};
        keep.stop_tokens = stop_tokens;
        rwkv_gen_params p{};
        p.first_token = first_token; p.max_tokens = max_tokens; p.kind = RWKV_SAMPLER_MIROSTAT;
        p.top_k = 1; p.temperature = 1.0f; p.tau = max_surprise; p.miro_target = target; p.miro_rate = rate;
        p.stop_tokens = keep.stop_tokens.empty() ? nullptr : keep.stop_tokens.data();
        p.n_stop = keep.stop_tokens.size();
        p.seed = seed; p.stream = stream;
        return p;
    }
    rwkv_gen_params gen_params_for_prompt(int32_t max_tokens, uint64_t seed, uint32_t stream, GenArrays &keep,
                                          const std::vector<uint32_t> &stop_tokens = {}) const {
        return gen_params_for(0, max_tokens, seed, stream, keep, stop_tokens);
    }
};

}  // namespace rwkv

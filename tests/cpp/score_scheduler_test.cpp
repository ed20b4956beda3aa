// CPU test of Scheduler::perplexity_scored / choose_scored (include/rwkv_scheduler.hpp) against perplexity / choose on a fake engine that
// scores its own Full rows in float64 (no GPU, no HIP): same ranking, values within 1e-5, the slot's state restored.
#include <cmath>
#include <cstdio>
#include <numeric>

#include "../../include/rwkv_scheduler.hpp"

#include "fake_engine.hpp"

namespace {
double log_softmax(const float *row, size_t V, uint32_t t) {
    double m = row[0];
    for (size_t v = 1; v < V; ++v) m = std::max(m, (double)row[v]);
    double s = 0.0;
    for (size_t v = 0; v < V; ++v) s += std::exp((double)row[v] - m);
    return ((double)row[t] - m) - std::log(s);
}
// FakeEngine plus the two scoring calls of rwkv::Runtime, computed from the fake's own Full rows
struct ScoringFake : FakeEngine {
    using FakeEngine::FakeEngine;
    int score_calls = 0, head_calls = 0;
    std::vector<std::vector<float>> infer_score(rwkv::RnnInput &in, std::vector<std::vector<uint32_t>> &targets) {
        ++score_calls;
        std::vector<size_t> before((size_t)max_batch);
        for (int b = 0; b < max_batch; ++b) {
            auto &ib = in.batches[(size_t)b];
            before[(size_t)b] = ib.tokens.size();
            if (!targets[(size_t)b].empty()) {
                if (targets[(size_t)b].size() != ib.tokens.size()) throw std::invalid_argument("one target per pending token");
                ib.option = rwkv::RnnOption::Full;
            } else if (!ib.tokens.empty() && ib.option != rwkv::RnnOption::None) throw std::invalid_argument("unscored slot must be state-only");
        }
        const std::vector<rwkv::RnnOutputBatch> rows = infer(in);
        std::vector<std::vector<float>> out((size_t)max_batch);
        for (int b = 0; b < max_batch; ++b) {
            auto &tg = targets[(size_t)b];
            if (tg.empty()) continue;
            const size_t n = before[(size_t)b] - in.batches[(size_t)b].tokens.size();
            for (size_t i = 0; i < n; ++i)
                out[(size_t)b].push_back(tg[i] == RWKV_SCORE_SKIP ? std::nanf("") : (float)log_softmax(rows[(size_t)b].data() + i * 8, 8, tg[i]));
            tg.erase(tg.begin(), tg.begin() + (long)n);
        }
        return out;
    }
    std::vector<float> score_rows(const std::vector<std::vector<float>> &rows, const std::vector<uint32_t> &tg) {
        ++head_calls;
        std::vector<float> out;
        for (size_t i = 0; i < rows.size(); ++i) out.push_back((float)log_softmax(rows[i].data(), rows[i].size(), tg[i]));
        return out;
    }
};
std::vector<size_t> ranking(const std::vector<float> &v) {
    std::vector<size_t> idx(v.size());
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return v[a] < v[b]; });
    return idx;
}
}  // namespace

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    using namespace rwkv;
    ScoringFake e(3, 2);                                             // 2 tokens per slot per call: several steps per evaluation
    Scheduler<ScoringFake> s(e);
    const Tokens prompt = {5, 1, 2, 6, 3};
    int b = -1, doc = -1;
    CHECK(s.queue(prompt, b) == SlotResult::Success);
    while (s.pending()) s.step();
    const std::vector<float> after_prompt = e.state.back(b);
    // a state-only request is mid-prefill while the choices are scored: it rides the scoring steps
    CHECK(s.queue({7, 7, 7, 7, 7, 7, 7}, doc, RnnOption::None) == SlotResult::Success && doc != b);
    const std::vector<Tokens> choices = {{1, 2, 3}, {}, {4}, {6, 6, 0, 1, 2}, {3, 3}};
    (void)s.choose_scored(b, choices, false);
    CHECK(s.request(doc).suffix.empty() && s.request(doc).prefix.size() == 7);   // the document rode along
    CHECK(e.state.back(b) == after_prompt);
    for (bool calibrate : {false, true}) {
        const std::vector<float> want = s.choose(b, choices, calibrate);
        CHECK(e.state.back(b) == after_prompt);
        const int heads = e.head_calls;
        const std::vector<float> got = s.choose_scored(b, choices, calibrate);
        CHECK(e.head_calls == heads + 1);                            // no `probs`: the head terms come from one score_rows call on the last row
        CHECK(e.state.back(b) == after_prompt);                      // the slot is back where the prompt left it
        CHECK(got.size() == want.size() && std::isinf(got[1]) && got[1] > 0);
        for (size_t i : {0u, 2u, 3u, 4u}) CHECK(std::fabs(got[i] - want[i]) <= 1e-5f);
        CHECK(ranking(got) == ranking(want));
        // probabilities handed in by the caller (what `sample()` returned): score_rows is not consulted
        std::vector<float> probs(8);
        for (uint32_t v = 0; v < 8; ++v) probs[v] = (float)std::exp(log_softmax(s.request(b).output.data(), 8, v));
        const std::vector<float> got2 = s.choose_scored(b, choices, calibrate, probs);
        CHECK(e.head_calls == heads + 1);
        for (size_t i : {0u, 2u, 3u, 4u}) CHECK(std::fabs(got2[i] - want[i]) <= 1e-5f);
        CHECK(e.state.back(b) == after_prompt);
    }
    CHECK(e.score_calls > 0);
    CHECK(s.request(doc).suffix.empty() && s.request(doc).prefix.size() == 7);   // the document rode along
    // perplexity_scored on its own, with and without head, against perplexity from the same state
    const float head = 0.25f;
    const float p1 = s.perplexity(b, {2, 2, 5}, &head);
    e.state.load(after_prompt, b);
    const float q1 = s.perplexity_scored(b, {2, 2, 5}, &head);
    e.state.load(after_prompt, b);
    const float p2 = s.perplexity(b, {2, 2, 5}, nullptr);
    e.state.load(after_prompt, b);
    const float q2 = s.perplexity_scored(b, {2, 2, 5}, nullptr);
    CHECK(std::fabs(p1 - q1) <= 1e-5f && std::fabs(p2 - q2) <= 1e-5f && std::fabs(p1 - p2) > 1e-3f);
    // a request that wants rows does not ride a scoring step, and is served by the next step()
    int other = -1;
    e.state.load(after_prompt, b);
    CHECK(s.queue({9, 9, 9}, other) == SlotResult::Success);
    (void)s.perplexity_scored(b, {1}, nullptr);
    CHECK(s.request(other).suffix.size() == 3);
    while (s.pending()) s.step();
    CHECK(s.request(other).suffix.empty() && !s.request(other).output.empty());
    // misuse: choices before the prompt has been read in
    s.push(b, 4);
    bool threw = false;
    try { s.choose_scored(b, choices, false); } catch (const std::logic_error &) { threw = true; }
    CHECK(threw);
    std::printf("score_scheduler_test: ok\n");
    return 0;
}

// CPU test of Scheduler::arm_with_stops(..., top_logprobs) (include/rwkv_scheduler.hpp) on a fake engine (no GPU, no HIP): the option reaches
// gen_set_topn of the armed slot, behind the arm (arming resets the slot's count), and 0 leaves the engine as it was.
#include <cstdio>
#include <string>

#include "../../include/rwkv_scheduler.hpp"

#include "fake_engine.hpp"

namespace {
// FakeEngine plus the three resident-generation calls the helper makes, recorded in order
struct ResidentFake : FakeEngine {
    using FakeEngine::FakeEngine;
    std::vector<std::string> calls;
    void gen_arm(int slot, const rwkv_gen_params &p) { calls.push_back("arm " + std::to_string(slot) + " " + std::to_string(p.first_token)); }
    void gen_set_stops(int slot, const std::vector<std::string> &stops, const std::vector<uint8_t> &tail) {
        calls.push_back("stops " + std::to_string(slot) + " " + std::to_string(stops.size()) + " " + std::to_string(tail.size()));
    }
    void gen_set_topn(int slot, int n) { calls.push_back("topn " + std::to_string(slot) + " " + std::to_string(n)); }
};
}  // namespace

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    using namespace rwkv;
    ResidentFake e(3, 4);
    Scheduler<ResidentFake> s(e);
    int b = -1;
    CHECK(s.queue({5, 1, 2}, b) == SlotResult::Success);
    while (s.pending()) s.step();
    rwkv_gen_params p{};
    p.first_token = 7;
    p.max_tokens = 4;
    const StopMatcher matcher({"ab"});
    s.arm_with_stops(b, p, {"ab"}, matcher, 5);
    const std::string at = std::to_string(b);
    CHECK((e.calls == std::vector<std::string>{"arm " + at + " 7", "stops " + at + " 1 0", "topn " + at + " 5"}));
    e.calls.clear();
    s.arm_with_stops(b, p, {"ab"}, matcher);                         // no lists asked for: the engine is not told anything about them
    CHECK((e.calls == std::vector<std::string>{"arm " + at + " 7", "stops " + at + " 1 0"}));
    e.calls.clear();
    for (int bad : {-1, RWKV_TOPN_MAX + 1}) {                        // refused before the slot is armed
        bool threw = false;
        try { s.arm_with_stops(b, p, {"ab"}, matcher, bad); } catch (const std::invalid_argument &) { threw = true; }
        CHECK(threw && e.calls.empty());
    }
    s.arm_with_stops(b, p, {}, matcher, RWKV_TOPN_MAX);
    CHECK(e.calls.back() == "topn " + at + " " + std::to_string(RWKV_TOPN_MAX));
    std::printf("topn_scheduler_test: ok\n");
    return 0;
}

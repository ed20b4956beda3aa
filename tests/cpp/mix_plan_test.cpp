// mix_plan_test.cpp — the commit carrier's plan without a GPU (tests/test_mix_cases_cpu.py, tests/mix_cases.py carrier_plans).
//   mix_plan_test        stdin: one line "T hilo C Dd" per carrier; stdout: the JSON object tests/cpp/mix_probe.hip prints as "carrier"
// Build: g++ -std=c++17 tests/cpp/mix_plan_test.cpp
#include "mix_probe_plan.h"

int main() {
    int T, hilo, C, Dd;
    while (std::scanf("%d %d %d %d", &T, &hilo, &C, &Dd) == 4) {
        rwkv::CarrierPlan r;
        rwkv::carrier_plan(T, hilo != 0, C, Dd, r);
        if (r.why) { std::fprintf(stderr, "mix_plan_test: %s\n", r.why); return 1; }
        rwkv::carrier_print(stdout, r);
        std::printf("\n");
    }
    return 0;
}

"""GPU (-m gpu): launch_topn_rows against a reference, launch by launch (DESIGN.md 3.8 "Top-n lists").

tests/cpp/topn_probe.hip — a stand-alone program linked against the kernel objects of the library build — calls launch_topn_rows once per case
of tests/topn_cases.py (proved on the CPU by tests/test_topn_cases_cpu.py) and copies every buffer back whole.  Asserted:

  * ownership, bit for bit: logits, spare rows and guard bands still hold what they held;
  * the ids are the reference's on EVERY row — dyadic, normal, all-equal, forty ties across lanes, waves and the last float4, zeros of both
    signs, alternating -inf, n > V, fewer than n live entries, a spike, a row that takes the exact search — nothing is skipped;
  * ln-probabilities within 2e-5 * max(1, |ref|) of float64 (dyadic rows: one ulp), -inf in the places without an entry, NaN on poisoned rows;
  * the side outputs: the copy of the rows bit for bit, m exact, ln S at the same bound, and every listed logp is (x - m) - ln S of them in
    every bit;
  * a row's list has the same bits whether the launch carries one row, five or all, with or without the side outputs.

One probe process per vocabulary size, each under its own time limit.  A process that ends by a signal, an abort, a HIP error or its time limit
is recorded: every later test of this module then fails at once and starts nothing on the GPU.  Nothing is retried.  The last test writes the
worst error / bound per group to profiles/r12_topn_probe_ratios.jsonl."""
import json
import os

import pytest

from tests import topn_cases as T
from tests.probe_run import require_alive, run_probe

pytestmark = pytest.mark.gpu
CASES = T.all_cases()
_STATE = {"dead": None, "lines": {}, "ratios": {}}
PROFILE = os.path.join(T.ROOT, "profiles", "r12_topn_probe_ratios.jsonl")


@pytest.fixture(scope="module")
def probe():
    return T.build_probe()


@pytest.mark.parametrize("group", T.GROUPS)
def test_lists_of_every_row(probe, tmp_path, group):
    cases = [c for c in CASES if c.group == group]
    datas = [T.make(c) for c in cases]
    plans, inp, out = run_probe(_STATE, probe, tmp_path, group, cases, lambda path: T.write_cases(path, cases, datas))
    results = T.read_results(out, cases, datas)
    os.remove(inp), os.remove(out)
    msgs, ratios = [], []
    for c, d, res, line in zip(cases, datas, results, plans):
        _STATE["lines"][c.name] = line
        msgs += T.check_case(c, d, res, line, ratios)
    msgs += T.cross_checks(cases, results, datas)
    worst = max(ratios, key=lambda x: x[2])
    print(f"worst error / bound in {group}: {worst[2]:.4f} ({worst[1]})")
    _STATE["ratios"][group] = {"group": group, "cases": len(cases), "rows": sum(c.p["n_rows"] for c in cases), "gpu_worst_error_over_bound": round(worst[2], 4),
                               "gpu_worst_case": worst[1]}
    assert not msgs, f"{len(msgs)} findings in {group}:\n" + "\n".join(m[:600] for m in msgs[:12])


def test_every_case_ran():
    require_alive(_STATE)
    missing = [c.name for c in CASES if c.name not in _STATE["lines"]]
    assert not missing, f"no line for {missing[:8]} (run the whole module)"
    with open(PROFILE, "w") as f:
        for g in T.GROUPS:
            f.write(json.dumps(_STATE["ratios"][g]) + "\n")

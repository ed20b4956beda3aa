"""GPU (-m gpu): the resident-generation kernels against a reference, launch by launch (DESIGN.md "Resident-generation probe").

tests/cpp/gen_probe.hip — a stand-alone program linked against the kernel objects of the library build — makes ONE launch of one gen_*
launcher per case of tests/gen_cases.py (proved on the CPU by tests/test_gen_cases_cpu.py) and copies every buffer back whole.  Asserted, bit
for bit: everything the launch writes is what the Python reference writes — SampleRow, the edited logits, penalty rows, GenSlot / GenStop /
GenDfa / GenPda words, tok_end, ring cells, the watch's record, captured and frozen state — and everything it does not own still holds what it
held: other slots' rows, other steps' ring cells, spare rows, guard bands.  gen_topn's ln-probabilities and ln S are held to the bound of
tests/topn_cases.py and, in kind topn_pair, to launch_topn_rows on the same rows in every bit.  The one exemption is the penalty row of a slot
that had finished before gen_post (dead data by the kernel's comment).

One probe process per group, each under its own time limit.  A process that ends by a signal, an abort, a HIP error, a refused case or its
time limit is recorded: every later test of this module then fails at once and starts nothing on the GPU.  Nothing is retried.  The last test
writes one line per group to profiles/r13_gen_probe_ratios.jsonl."""
import json
import os

import pytest

from tests import gen_cases as G
from tests.probe_run import require_alive, run_probe

pytestmark = pytest.mark.gpu
_STATE = {"dead": None, "lines": {}, "ratios": {}}
PROFILE = os.path.join(G.ROOT, "profiles", "r13_gen_probe_ratios.jsonl")


@pytest.fixture(scope="module")
def probe():
    return G.build_probe()


@pytest.mark.parametrize("group", G.GROUPS)
def test_every_buffer_of_every_launch(probe, tmp_path, group):
    cases = [c for c in G.all_cases() if c.group == group]
    datas = [G.make(c) for c in cases]
    plans, inp, out = run_probe(_STATE, probe, tmp_path, group, cases, lambda path: G.write_cases(path, cases, datas))
    results = G.read_results(out, cases, datas)
    os.remove(inp), os.remove(out)
    msgs, ratios = [], []
    for c, d, res, line in zip(cases, datas, results, plans):
        _STATE["lines"][c.name] = line
        msgs += G.check_case(c, d, res, line, ratios)
    worst = max(ratios, key=lambda x: x[2])
    print(f"worst top-n error / bound in {group}: {worst[2]:.4f} ({worst[1]})")
    rows = sum(c.p["n_rows"] for c in cases)
    _STATE["ratios"][group] = ({"group": group, "cases": len(cases), "rows": rows, "gpu_worst_error_over_bound": round(worst[2], 4), "gpu_worst_case": worst[1]}
                               if group == "topn" else {"group": group, "cases": len(cases), "rows": rows, "compared": "exact"})
    assert not msgs, f"{len(msgs)} findings in {group}:\n" + "\n".join(m[:600] for m in msgs[:12])


def test_every_case_ran():
    require_alive(_STATE)
    cases = G.all_cases()
    missing = [c.name for c in cases if c.name not in _STATE["lines"]]
    assert not missing, f"no line for {missing[:8]} (run the whole module)"
    wrong = [c.name for c in cases if _STATE["lines"][c.name] != G.plan_line(c)]
    assert not wrong, f"the probe's line differs from the table's for {wrong[:8]}"
    ran = [c for c in cases if c.name in _STATE["lines"]]
    assert G.coverage_gaps(ran) == []
    with open(PROFILE, "w") as f:
        for g in G.GROUPS:
            f.write(json.dumps(_STATE["ratios"][g]) + "\n")

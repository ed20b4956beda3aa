"""GPU (-m gpu): the sampling and vocabulary-row kernels against a reference, launch by launch (DESIGN.md "Sampling and vocabulary-row probe").

tests/cpp/sample_probe.hip — a stand-alone program linked against the kernel objects of the library build — calls launch_nucleus,
launch_softmax, launch_score_rows, launch_argmax, launch_logit_adjust and launch_logit_mask once per case of tests/sample_cases.py (proved
on the CPU by tests/test_sample_cases_cpu.py), a sampler case twice into separate outputs, and copies every buffer back whole.  Asserted:

  * ownership, bit for bit: logits, spare rows, guard bands, the SampleRow array, rows whose kind's `any_*` flag is off, untouched elements
    of the logit edits, the arg-max scratch beyond n_rows * 32 entries still hold what they held;
  * the two launches of a sampler case agree in every bit; a row the narrow kernels serve exactly has the same bits from the wide one;
  * the sampled token is the reference's on EVERY row: nothing is skipped, no margin caps a comparison (family A: dyadic rows, out_prob
    exact too; family B: flattened draws with asserted margins; family C: level rows over several windows, restated from calibrated bits);
  * out_prob / the Mirostat surprise of families B and C against float64 at the project's Fp32 bound 2e-5; softmax at its addition-chain
    bound; score_rows at 2e-5 * max(1, |ref|), the same bits whether a launch carries one row, five or all; arg-max, logit_adjust and
    logit_mask exact.

One probe process per group, each under its own time limit.  A process that ends by a signal, an abort, a HIP error or its time limit is
recorded: every later test of this module then fails at once and starts nothing on the GPU.  Nothing is retried.  The last test proves
coverage from the lines the probe printed and writes the worst error / bound per group to profiles/r11_sample_probe_ratios.jsonl."""
import json
import os

import pytest

from tests import sample_cases as S
from tests.probe_run import require_alive, run_probe

pytestmark = pytest.mark.gpu
CASES = S.all_cases()
_STATE = {"dead": None, "lines": {}, "ratios": {}, "datas": {}}
PROFILE = os.path.join(S.ROOT, "profiles", "r11_sample_probe_ratios.jsonl")


@pytest.fixture(scope="module")
def probe():
    return S.build_probe()


def run_group(probe, tmp_path, group):
    cases = [c for c in CASES if c.group == group]
    datas = [S.make(c) for c in cases]
    plans, inp, out = run_probe(_STATE, probe, tmp_path, group, cases, lambda path: S.write_cases(path, cases, datas))
    results = S.read_results(out, cases, datas)
    os.remove(inp), os.remove(out)
    msgs, ratios = [], []
    for c, d, res, line in zip(cases, datas, results, plans):
        _STATE["lines"][c.name] = line
        _STATE["datas"][c.name] = {k: d[k] for k in ("S", "rows") if k in d}
        msgs += S.check_case(c, d, res, line, ratios)
    msgs += S.cross_checks(cases, results, datas)
    if ratios:
        worst = max(ratios, key=lambda x: x[2])
        print(f"worst error / bound in {group}: {worst[2]:.4f} ({worst[1]})")
        _STATE["ratios"][group] = {"group": group, "cases": len(cases), "rows": sum(c.p["n_rows"] for c in cases), "gpu_worst_error_over_bound": round(worst[2], 4),
                                   "gpu_worst_case": worst[1]}
    else:
        _STATE["ratios"][group] = {"group": group, "cases": len(cases), "rows": sum(c.p["n_rows"] for c in cases), "gpu_worst_error_over_bound": 0.0, "gpu_worst_case": "exact"}
    assert not msgs, f"{len(msgs)} findings in {group}:\n" + "\n".join(m[:600] for m in msgs[:12])


def test_dyadic_rows_full_vocabulary(probe, tmp_path):
    run_group(probe, tmp_path, "dyadic_full")


def test_dyadic_rows_id_sets(probe, tmp_path):
    run_group(probe, tmp_path, "dyadic_sets")


def test_flattened_draws_rank_by_rank(probe, tmp_path):
    run_group(probe, tmp_path, "flattened")


def test_calibrated_level_rows(probe, tmp_path):
    run_group(probe, tmp_path, "calibrated")


def test_routing_and_ownership(probe, tmp_path):
    run_group(probe, tmp_path, "routing")


def test_softmax(probe, tmp_path):
    run_group(probe, tmp_path, "softmax")


def test_score_rows(probe, tmp_path):
    run_group(probe, tmp_path, "score_rows")


def test_argmax(probe, tmp_path):
    run_group(probe, tmp_path, "argmax")


def test_logit_adjust_and_mask(probe, tmp_path):
    run_group(probe, tmp_path, "logit_edit")


def test_the_table_reached_every_branch():
    require_alive(_STATE)
    missing = [c.name for c in CASES if c.name not in _STATE["lines"]]
    assert not missing, f"no line for {missing[:8]} (run the whole module)"
    assert [_STATE["lines"][c.name] for c in CASES] == [S.plan_line(c) for c in CASES]
    # coverage from what the probe repeated (its flags and shapes are the table's, just asserted) and the rows that went in
    assert S.coverage_gaps(CASES, [_STATE["datas"][c.name] for c in CASES]) == []
    with open(PROFILE, "w") as f:
        for g in S.GROUPS:
            f.write(json.dumps(_STATE["ratios"][g]) + "\n")

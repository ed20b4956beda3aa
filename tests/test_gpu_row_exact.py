"""GPU (-m gpu): the row, WKV and state kernels against a reference, launch by launch (DESIGN.md "Row and recurrence probe").

tests/cpp/row_probe.hip — a stand-alone program linked against the kernel objects of the library build — calls launch_wkv, launch_wkv4,
launch_ln_shift, launch_embed, launch_ln_out and launch_state_pack once per case of tests/row_cases.py (proved on the CPU by
tests/test_row_cases_cpu.py) and copies every buffer back whole.  Asserted, per case:

  * ownership, bit for bit: operand rows of no sequence, rows T .. ceil16(T) - 1, columns C .. ldh - 1, guard bands, state tiles and sx rows
    of slots outside the step and the gaps between slots, v_first when layer != 0 still hold what they held; no NaN of an unowned input row
    reaches an owned output; on V7 layer 0 the owned v_first rows are v's bits;
  * state_pack is a permutation: every element exact, both ways, the source side untouched;
  * ln_shift's x_out equals the fp32 sum x_in + P[0] + .. + P[np-1] in that order, bit for bit;
  * the WKV state of the exact-grid cases meets the float64 reference in EVERY BIT, in all three kernel forms: no tolerance;
  * everything else against float64 numpy at the project's Fp32 bound 2e-5 * max(1, |ref|); the worst error / bound per group is printed (`-s`).

One probe process per group, each under its own time limit.  A process that ends by a signal, an abort, a HIP error or its time limit is
recorded: every later test of this module then fails at once and starts nothing on the GPU.  Nothing is retried.  The last test proves from
the lines the probe printed that every kernel the table exists for was reached."""
import os

import numpy as np
import pytest

from tests import row_cases as R
from tests.probe_run import require_alive, run_probe

pytestmark = pytest.mark.gpu
CASES = R.all_cases()
_STATE = {"dead": None, "lines": {}, "ratios": [], "results": {}}


@pytest.fixture(scope="module")
def probe():
    return R.build_probe()


def run_group(probe, tmp_path, group):
    cases = [c for c in CASES if c.group == group]
    datas = [R.make(c) for c in cases]
    plans, inp, out = run_probe(_STATE, probe, tmp_path, group, cases, lambda path: R.write_cases(path, cases, datas))
    results = R.read_results(out, cases, datas)
    os.remove(inp), os.remove(out)
    msgs, before = [], len(_STATE["ratios"])
    for c, d, res, line in zip(cases, datas, results, plans):
        _STATE["lines"][c.name] = line
        msgs += R.check_case(c, d, res, line, _STATE["ratios"])
        if c.kind == R.K_WKV and (c.name.endswith("_unknown") or c.name + "_unknown" in {x.name for x in cases}):
            _STATE["results"][c.name] = {k: res[k] for k in ("state", "yhi", "ylo") if k in res}
    ratios = _STATE["ratios"][before:]
    if ratios:
        worst = max(ratios, key=lambda x: x[2])
        print(f"worst error / bound in {group}: {worst[2]:.4f} ({worst[1]})")
    assert not msgs, f"{len(msgs)} findings in {group}:\n" + "\n".join(msgs[:12])


def test_wkv_v5(probe, tmp_path):
    run_group(probe, tmp_path, "wkv5")


def test_wkv_v6(probe, tmp_path):
    run_group(probe, tmp_path, "wkv6")


def test_wkv_v7(probe, tmp_path):
    run_group(probe, tmp_path, "wkv7")


def test_wkv4(probe, tmp_path):
    run_group(probe, tmp_path, "wkv4")


def test_ln_shift_1024_threads(probe, tmp_path):
    run_group(probe, tmp_path, "ln_shift_1024")


def test_ln_shift_512_threads(probe, tmp_path):
    run_group(probe, tmp_path, "ln_shift_512")


def test_embed_and_ln_out(probe, tmp_path):
    run_group(probe, tmp_path, "embed_ln_out")


def test_state_pack(probe, tmp_path):
    run_group(probe, tmp_path, "state_pack")


def test_the_table_reached_every_kernel():
    require_alive(_STATE)
    missing = [c.name for c in CASES if c.name not in _STATE["lines"]]
    assert not missing, f"no line for {missing[:8]} (run the whole module)"
    lines = [_STATE["lines"][c.name] for c in CASES]
    assert lines == [R.plan_line(c) for c in CASES]
    assert R.coverage_gaps(lines) == []
    # reported, not asserted: do the CH = 8 and CH = 32 forms of wkv_chunk_kernel give the same bits on the same step?  (They share phase B's arithmetic; if
    # they differ, a slot's result depends on how many rows its neighbours have in the step.)
    for short, long_ in R.twins(CASES):
        a, b = _STATE["results"][short.name], _STATE["results"][long_.name]
        same = {k: bool(np.array_equal(a[k], b[k])) for k in a}
        print(f"CH = 8 against CH = 32 on {short.name}: " + ", ".join(f"{k} {'identical' if v else 'DIFFERENT'}" for k, v in same.items()))

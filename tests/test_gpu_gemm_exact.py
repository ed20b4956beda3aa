"""GPU (-m gpu): every GEMM kernel variant against an exact reference, launch by launch (DESIGN.md "GEMM probe").

tests/cpp/gemm_probe.hip — a stand-alone program linked against the kernel objects of the library build — runs the product's load-time
kernel on raw weights, plans with the engine's own planner, launches through launch_smallk / launch_gemm_tile / launch_gemm and copies every
buffer back whole.  The inputs (tests/gemm_cases.py; proved on the CPU by tests/test_gemm_cases_cpu.py) come from grids on which every product
and every partial sum is an fp32 value, so the order of summation — k-steps, waves, LDS reduction, K slabs, hi + lo — cannot matter and the
fp64 reference must be met in EVERY BIT: no tolerance.  Whatever a launch does not own (rows >= T, columns between and beyond the problems,
slabs >= ksplit, operand rows T .. ceil16(T) - 1, guard bands) must still hold the NaN pattern it was filled with, and the NaN rows that
pad X must reach no valid output.  Only the transcendental activations are compared with a tolerance, the project's Fp32 one
(2e-5 * max(1, |ref|)), on an exact accumulator; the worst ratio is printed (`-s`).

One probe process per test, each under its own time limit.  A process that ends by a signal, an abort or its time limit is recorded: every
later test of this module then fails at once and starts nothing on the GPU.  Nothing is retried.  The last test reads the plan lines the
probe printed and proves that the table reached the paths it exists for, and that the probe planned what the CPU-compiled planner plans."""
import os

import pytest

from tests import gemm_cases as G
from tests.probe_run import require_alive, run_probe

pytestmark = pytest.mark.gpu
CASES = G.all_cases()
_STATE = {"dead": None, "plans": {}, "ratios": []}


@pytest.fixture(scope="module")
def probe():
    return G.build_probe()


def run_group(probe, tmp_path, group):
    cases = [c for c in CASES if c.group == group]
    datas = [G.make(c) for c in cases]
    plans, inp, out = run_probe(_STATE, probe, tmp_path, group, cases, lambda path: G.write_cases(path, cases, datas))
    results = G.read_results(out, cases)
    os.remove(inp), os.remove(out)
    msgs = []
    for c, d, res, plan in zip(cases, datas, results, plans):
        _STATE["plans"][c.name] = plan
        msgs += G.check_case(c, d, res, plan, _STATE["ratios"])
    assert not msgs, f"{len(msgs)} findings in {group}:\n" + "\n".join(msgs[:12])
    return cases, plans


def test_decode_plain(probe, tmp_path):
    run_group(probe, tmp_path, "decode_plain")


def test_decode_hilo(probe, tmp_path):
    run_group(probe, tmp_path, "decode_hilo")


def test_decode_ksplit_tail_multiproblem(probe, tmp_path):
    run_group(probe, tmp_path, "decode_split")


def test_smallk(probe, tmp_path):
    run_group(probe, tmp_path, "smallk")


def test_tile_chunked_registers(probe, tmp_path):
    run_group(probe, tmp_path, "tile_kind0")


def test_tile_chunked_lds_dma(probe, tmp_path):
    run_group(probe, tmp_path, "tile_kind1")


def test_tile_pipelined(probe, tmp_path):
    run_group(probe, tmp_path, "tile_kind2")


def test_tile_pipelined_hilo(probe, tmp_path):
    run_group(probe, tmp_path, "tile_kind3")


def test_onehot_int8(probe, tmp_path):
    run_group(probe, tmp_path, "onehot_int8")


def test_onehot_nf4(probe, tmp_path):
    run_group(probe, tmp_path, "onehot_nf4")


def test_epilogues(probe, tmp_path):
    before = len(_STATE["ratios"])
    run_group(probe, tmp_path, "epilogues")
    ratios = _STATE["ratios"][before:]
    assert ratios
    for name, i, ratio in ratios:
        print(f"activation error / tolerance: {name} problem {i}: {ratio:.4f}")
    print(f"worst activation error / tolerance: {max(r for _, _, r in ratios):.4f}")


def test_the_table_took_the_paths_it_exists_for(tmp_path):
    require_alive(_STATE)
    missing = [c.name for c in CASES if c.name not in _STATE["plans"]]
    assert not missing, f"no plan line for {missing[:8]} (run the whole module)"
    plans = [_STATE["plans"][c.name] for c in CASES]
    gaps = G.coverage_gaps(CASES, plans)
    assert not gaps, gaps
    # the probe planned what the planner compiled with a plain host compiler plans (tests/test_gemm_cases_cpu.py proves coverage on those lines)
    cpu = G.plan_cpu(G.build_planner(tmp_path), CASES)
    strip = lambda p: {k: v for k, v in p.items() if k != "case"}
    differ = [(c.name, strip(g), strip(w)) for c, g, w in zip(CASES, plans, cpu) if not c.single and strip(g) != strip(w)]
    assert not differ, differ[:4]

"""GPU (-m gpu): the V6 mix kernels, the LayerNorm prologue and the token-shift commit block against a reference, launch by launch (DESIGN.md
"Mix, prologue and commit probe").

tests/cpp/mix_probe.hip — a stand-alone program linked against the kernel objects of the library build — calls launch_v6_mix once per case of
tests/mix_cases.py (proved on the CPU by tests/test_mix_cases_cpu.py), launch_gemm once per commit case and both, in that order, per pair case,
and copies every buffer back whole.  Asserted, per case:

  * the saturated lattice: every operand the launch writes, the fp32 slice partials slab by slab, the m tiles of the two-launch form, the published
    xx_out — bit for bit, no tolerance;
  * general values against float64 numpy at the project's Fp32 bound 2e-5 * max(1, |ref|) (the hi-only forms: plus the tie budget of the rounded
    entries); x_out equals the ordered fp32 sum bit for bit; the worst error / bound per group is printed (`-s`) and written to
    profiles/r10_mix_probe_ratios.jsonl;
  * ownership, bit for bit: operand rows T .. ceil16(T) - 1, columns C .. ld - 1, guard bands, slabs of mp beyond the slices, mg_* and mp whole when
    the form does not use them; the prologue launch leaves every sx row as it was; the commit writes the source row into the committed slot and
    nothing else, nothing at all with last = -1; the carrier's own outputs stay exact.

What the lines pin: `split` / `ksp` are the product's own v6_mix_split; form, NT, both grids and the apply launch's tile are the launcher's rule
RESTATED in the probe (launch_v6_mix returns nothing), so their equality with mix_cases.plan_line pins the Python transcription against that C++
restatement, not against what was launched.  What launch_v6_mix really launched is constrained by the outputs alone: a grid.x, a strip walk or an
apply tile other than the rule's leaves elements unwritten or written from the wrong tile, which the bit-exact family reports.

One probe process per group, each under its own time limit.  A process that ends by a signal, an abort, a HIP error or its time limit is
recorded: every later test of this module then fails at once and starts nothing on the GPU.  Nothing is retried.  The last test proves from
the lines the probe printed that every instantiation and branch the table exists for was reached."""
import json
import os

import pytest

from tests import mix_cases as M
from tests.probe_run import require_alive, run_probe

pytestmark = pytest.mark.gpu
CASES = M.all_cases()
_STATE = {"dead": None, "lines": {}, "ratios": []}
PROFILE = os.path.join(M.ROOT, "profiles", "r10_mix_probe_ratios.jsonl")


@pytest.fixture(scope="module")
def probe():
    return M.build_probe()


@pytest.fixture(scope="module")
def carriers(tmp_path_factory):
    return M.carrier_plans(M.build_planner(tmp_path_factory.mktemp("mix_plan")), CASES)


def record(group, worst):
    """One line per group in the profile file: tau and the worst error / bound the GPU gave."""
    rows = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as f:
            rows = {r["group"]: r for r in map(json.loads, filter(None, (l.strip() for l in f)))}
    rows[group] = {**rows.get(group, {}), "group": group, "tau": M.TAU[group], "tau_z": M.TAU_Z if group == "mix_lnp" else 0.0, "gpu_worst_error_over_bound": round(worst[2], 4),
                   "gpu_worst_case": worst[1]}
    with open(PROFILE, "w") as f:
        for g in M.GROUPS:
            if g in rows:
                f.write(json.dumps(rows[g]) + "\n")


def run_group(probe, tmp_path, group, carriers):
    cases = [c for c in CASES if c.group == group]
    datas = [M.make(c) for c in cases]
    plans, inp, out = run_probe(_STATE, probe, tmp_path, group, cases, lambda path: M.write_cases(path, cases, datas))
    results = M.read_results(out, cases, datas)
    os.remove(inp), os.remove(out)
    msgs, before = [], len(_STATE["ratios"])
    for c, d, res, line in zip(cases, datas, results, plans):
        _STATE["lines"][c.name] = line
        msgs += M.check_case(c, d, res, line, _STATE["ratios"], carriers.get(c.name))
    ratios = [x for x in _STATE["ratios"][before:] if not x[1].endswith("_lattice")]
    if ratios:
        worst = max(ratios, key=lambda x: x[2])
        print(f"worst error / bound in {group}: {worst[2]:.4f} ({worst[1]})")
        record(group, worst)
    assert not msgs, f"{len(msgs)} findings in {group}:\n" + "\n".join(m[:600] for m in msgs[:12])


def test_mix_decode(probe, tmp_path, carriers):
    run_group(probe, tmp_path, "mix_decode", carriers)


def test_mix_lnp(probe, tmp_path, carriers):
    run_group(probe, tmp_path, "mix_lnp", carriers)


def test_mix_wide(probe, tmp_path, carriers):
    run_group(probe, tmp_path, "mix_wide", carriers)


def test_mix_split(probe, tmp_path, carriers):
    run_group(probe, tmp_path, "mix_split", carriers)


def test_mix_ksliced(probe, tmp_path, carriers):
    run_group(probe, tmp_path, "mix_ksliced", carriers)


def test_commit(probe, tmp_path, carriers):
    run_group(probe, tmp_path, "commit", carriers)


def test_the_table_reached_every_instantiation(carriers):
    require_alive(_STATE)
    missing = [c.name for c in CASES if c.name not in _STATE["lines"]]
    assert not missing, f"no line for {missing[:8]} (run the whole module)"
    lines = [_STATE["lines"][c.name] for c in CASES]
    assert lines == [M.plan_line(c, carriers.get(c.name)) for c in CASES]
    assert M.coverage_gaps(lines) == []

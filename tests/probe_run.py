"""One probe process per group of cases, for the four tests/test_gpu_*_exact.py modules.  A process that ends by a signal, an abort, a HIP error,
a refused case or its time limit is recorded in the module's state: every later test of that module then fails at once and starts nothing on
the GPU.  Nothing is retried."""
import json
import subprocess

import pytest


def require_alive(state):
    if state["dead"]:
        pytest.fail(f"not run: an earlier probe process of this module did not end normally ({state['dead']})")


def run_probe(state, probe, tmp_path, group, cases, write):
    """`write(path)` writes the group's case file.  Returns the probe's JSON lines, one per case, and the paths of the case file and the result
    file: the caller reads the results, then removes both."""
    require_alive(state)
    inp, out = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    write(inp)
    limit = 30 + len(cases)                                            # seconds: a launch and its copies take milliseconds; the first one loads the code objects
    try:
        r = subprocess.run([probe, inp, out], capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        lines = (e.stdout or b"").decode(errors="replace").splitlines()
        state["dead"] = f"{group}: no end after {limit} s; {len(lines)} lines of {len(cases)} cases (at: {cases[min(len(lines), len(cases) - 1)].name}, {lines[-1:]})"
        pytest.fail(state["dead"])
    lines = r.stdout.splitlines()
    if r.returncode != 0:                                              # a signal, an abort, a refused case, or the first failed HIP call (the probe checks every one)
        at = cases[min(len(lines), len(cases) - 1)].name               # a case's line comes out only after its results: the next one was running
        state["dead"] = f"{group}: the probe ended with status {r.returncode} after {len(lines)} lines of {len(cases)} cases (at: {at}, {lines[-1:]}): {r.stderr[-600:]}"
        pytest.fail(state["dead"])
    plans = [json.loads(l) for l in lines]
    assert len(plans) == len(cases)
    return plans, inp, out

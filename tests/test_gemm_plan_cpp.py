"""CPU: the GEMM launch planner (ai00_server_amd/csrc/gemm_plan.h) replays launch logs recorded on the MI355X and must reproduce, for
every GEMM line, the five fields the engine logged: kind, variant, grid, threads, ksplit.  Compiled with g++, no GPU and no HIP involved.

A log line names the matrices of a launch; this file restates what the engine knows about them (shape and storage format by model width
and quantisation, which operand class a launch belongs to and so whether it reads hi + lo operands, its epilogue) — the planner under
test decides nothing of that."""
import glob
import json
import lzma
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = {   # (version, C, F); the head has 65536 rows everywhere
    "v5-24h": (5, 1536, 5376), "v6-1.6b": (6, 2048, 7168), "v6-3b": (6, 2560, 8960), "v6-7b": (6, 4096, 14336), "v7-2.9b": (7, 2560, 10240),
}
V = 65536
FMT = {"fp16": 0, "int8": 1, "nf4": 2}
# operand classes (rwkv_engine.cpp OpdClass) by the first matrix of a launch; Precision::Fp16 promotes the classes of promote_for_version
CLS_ATT, CLS_LORA2, CLS_WO, CLS_FFN1, CLS_FV, CLS_HEAD = range(6)
CLASS_OF = {"att.key.weight": CLS_ATT, "att.receptance.weight": CLS_ATT, "att.w2": CLS_LORA2, "att.output.weight": CLS_WO,
            "ffn.key.weight": CLS_FFN1, "ffn.value.weight": CLS_FV, "head.weight": CLS_HEAD}


def matrix(name, version, C, F, q):
    """(rows, K, fmt, partial, kcopies, smallk) of one problem: the shape the planner sees (gemm_plan.h ProbShape)."""
    if version == 6:
        Dd = 128 if C >= 4096 else 64
    lora7 = dict(zip("wavg", (96, 96, 64, 320) if C >= 2560 else (64, 64, 32, 128)))
    m = re.fullmatch(r"att\.([wavg])([12])", name)
    if m:                                                       # V7 LoRA pairs, fp16: first stage -> operand, second stage -> act(x + bias), fp32
        D = lora7[m.group(1)]
        return (D, C, 0, 0, 0, 0) if m.group(2) == "1" else (C, D, 0, 0, int(m.group(1) == "g"), 1)
    return {
        "att.receptance.weight": (C, C, q, 0, 1, 1), "att.key.weight": (C, C, q, 0, 1, 1), "att.value.weight": (C, C, q, 0, 1, 1),
        "att.gate.weight": (C, C, q, 0, 0, 1),                  # SiLU
        "att.time_decay_w1": (Dd if version == 6 else 0, C, 0, 0, 0, 1),   # tanh
        "att.output.weight": (C, C, q, 1, 1, 1),                # linear: partial slabs
        "ffn.key.weight": (F, C, q, 0, 0, 0),                   # relu^2 into the next launch's operand
        "ffn.receptance.weight": (C, C, q, 0, 0, 1),            # sigmoid
        "ffn.value.weight": (C, F, q, 1, 1, int(version == 7)),   # linear; V5 / V6 multiply by the receptance (POST_MUL)
        "head.weight": (V, C, 0, 0, 1, 1),
    }[name]


def case_of(d, width, quant, precision, switches):
    version, C, F = WIDTHS[width]
    names = d["mats"].split("+")
    cls = CLASS_OF[names[0]]
    mask = {"Fp32": 63, "Fp16Raw": 0, "Fp16": 7 if version == 7 else 1}[precision]
    hilo = (mask >> cls) & 1
    # V6 single-token steps: the time-mix launch follows the fused mix with the LayerNorm prologue and carries its token-shift commit
    # (rwkv_kernels.hip v6_mix_ln_supported: plain operands engine-wide, at most LNP_MAX_NP = 5 slabs to sum, C <= 4096)
    commit = int(version == 6 and cls == CLS_ATT and d["T"] == 1 and precision != "Fp32" and d["np_in"] <= 5 and C <= 4096)
    probs = [matrix(n, version, C, F, FMT[quant]) for n in names]
    assert sum(p[0] for p in probs) == d["rows"], d
    knobs = [int(switches.get("RWKV_NO_TILE", 0)), int(switches.get("RWKV_TILE_SHAPE", -1)), int(switches.get("RWKV_TILE_KSPLIT", 1)), -1]
    words = [d["T"], hilo, commit] + knobs + [len(probs)] + [x for p in probs for x in p]
    return " ".join(str(w) for w in words), f'{d["kind"]} {d["variant"]} {d["grid"]} {d["threads"]} {d["ksplit"]}'


def fixture_cases():
    with lzma.open(os.path.join(ROOT, "tests", "golden", "gemm_plans.json.xz")) as f:
        lines = json.load(f)
    for d in lines:
        width, quant, precision, *sw = d["engine"].split("/")
        yield d, case_of(d, width, quant, precision, dict(s.split("=") for s in sw))


def round6_cases():
    """profiles/r6_launch_log_*.jsonl: eleven runs recorded on hardware in round 6 (layers 0 and 1 and the head, layer numbers kept)."""
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r6_launch_log_*.jsonl")))
    assert len(paths) == 11
    for path in paths:
        m = re.search(r"_(v\d-[\d.]+b)_(int8|fp16|nf4)_[^_.]+(?:_(fp32|fp16raw))?\.jsonl$", path)
        width, quant = m.group(1), m.group(2)
        precision = {None: "Fp16", "fp32": "Fp32", "fp16raw": "Fp16Raw"}[m.group(3)]
        gemms = [d for d in map(json.loads, open(path)) if d["kind"] != "row"]
        fv = {d["T"]: d["ksplit"] for d in gemms if "blocks.0.ffn.value.weight" in d["mats"]}
        for d in gemms:
            d = dict(d, np_in=0 if d["mats"].startswith("blocks.0.") else fv.get(d["T"], 0), mats=re.sub(r"blocks\.\d+\.", "", d["mats"]))
            yield dict(d, engine=os.path.basename(path)), case_of(d, width, quant, precision, {})


def test_gemm_planner_replays_the_recorded_launches(tmp_path):
    exe = str(tmp_path / "gemm_plan_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "gemm_plan_test.cpp"), "-o", exe])
    cases = list(fixture_cases())
    n_fixture = len(cases)
    cases += list(round6_cases())
    # both sides of every threshold, every forced shape and both switches are in the fixture; every line is replayed
    engines = {d["engine"] for d, _ in cases[:n_fixture]}
    assert n_fixture >= 3000 and len(engines) == 32 and len(cases) - n_fixture >= 100
    assert {d["T"] for d, _ in cases[:n_fixture]} >= {1, 16, 17, 32, 33, 64, 65, 192, 193, 256, 320, 321, 512, 548, 768, 769, 1024, 1280, 1281, 2048}
    out = subprocess.run([exe], input="\n".join(c[0] for _, c in cases) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(cases)
    wrong = [(d["engine"], d["T"], d["mats"], want, g) for (d, (_, want)), g in zip(cases, got) if g != want]
    assert not wrong, f"{len(wrong)} of {len(cases)} launches planned differently (engine, T, matrices, logged, planned): {wrong[:10]}"

"""Build librwkv_hip.so in-tree with hipcc for gfx950 (no cmake needed; ~40 s cold).

    python -m ai00_server_amd.build [--force]
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librwkv_hip.so")
SOURCES = ["rwkv_kernels.hip", "rwkv_engine.cpp", "tokenizer.cpp", "rwkv_dfa.cpp"]
DEPS = SOURCES + ["rwkv_kernels.h", "gemm_plan.h", "graph_cache.h", "gen_stop.h", "gen_dfa.h", "rwkv_dfa.h", "safetensors.hpp", "rwkv_abi.map", os.path.join("..", "..", "include", "rwkv_abi.h"),
               os.path.join("..", "..", "include", "rwkv_runtime.hpp"), os.path.join("..", "..", "include", "rwkv_scheduler.hpp"),
               os.path.join("..", "..", "include", "rwkv_router.hpp"),
               os.path.join("..", "..", "harness", "decode_loop.cpp"), os.path.join("..", "..", "harness", "serve_loop.cpp"),
               os.path.join("..", "..", "harness", "router_loop.cpp")]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


STAMP = os.path.join(HERE, ".build_stamp")


def _sources_digest() -> str:
    import hashlib
    h = hashlib.sha256()
    for d in sorted(DEPS):
        with open(os.path.join(CSRC, d), "rb") as f:
            h.update(d.encode())
            h.update(f.read())
    return h.hexdigest()


def needs_build() -> bool:
    """Content-based (mtimes do not survive the copy to a GPU box): rebuild when a source differs from the stamp."""
    if not all(os.path.exists(p) for p in (LIB, HARNESS_BIN, SERVE_BIN, ROUTER_BIN, EMBED_BIN, STAMP)):
        return True
    return open(STAMP).read().strip() != _sources_digest()


KERNEL_PARTS = 6      # rwkv_kernels.hip is compiled once per part (-DRWKV_PART=k), in parallel


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and not needs_build():
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    hipcc = _hipcc()
    jobs = []
    for src in SOURCES:
        stem = os.path.splitext(src)[0]
        base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
        if src.endswith(".cpp"):
            base += ["-x", "hip"]
        if src == "rwkv_kernels.hip":
            for k in range(KERNEL_PARTS):
                obj = os.path.join(CSRC, f"{stem}.p{k}.o")
                jobs.append((base + [f"-DRWKV_PART={k}", "-c", os.path.join(CSRC, src), "-o", obj], obj))
        else:
            obj = os.path.join(CSRC, stem + ".o")
            jobs.append((base + ["-c", os.path.join(CSRC, src), "-o", obj], obj))

    def run(job):
        if verbose:
            print("[build]", " ".join(job[0]), flush=True)
        subprocess.check_call(job[0])
        return job[1]

    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as ex:
        objs = list(ex.map(run, jobs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, "rwkv_abi.map"), "-o", LIB] + objs
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    build_harness(verbose)
    with open(STAMP, "w") as f:
        f.write(_sources_digest())
    return LIB


HARNESS_SRC = os.path.join(HERE, "..", "harness", "decode_loop.cpp")
HARNESS_BIN = os.path.join(HERE, "..", "harness", "decode_loop")
SERVE_SRC = os.path.join(HERE, "..", "harness", "serve_loop.cpp")
SERVE_BIN = os.path.join(HERE, "..", "harness", "serve_loop")
ROUTER_SRC = os.path.join(HERE, "..", "harness", "router_loop.cpp")
ROUTER_BIN = os.path.join(HERE, "..", "harness", "router_loop")
EMBED_SRC = os.path.join(HERE, "..", "harness", "embed_job.cpp")
EMBED_BIN = os.path.join(HERE, "..", "harness", "embed_job")


def build_harness(verbose: bool = True) -> str:
    """C++ mirror of ai00-core's infer task + greedy loop (harness/decode_loop.cpp), linked against the .so."""
    for src, exe in ((HARNESS_SRC, HARNESS_BIN), (SERVE_SRC, SERVE_BIN), (ROUTER_SRC, ROUTER_BIN), (EMBED_SRC, EMBED_BIN)):
        cmd = ["g++", "-O2", "-std=c++17", "-pthread", src, "-o", exe, "-L" + HERE, "-lrwkv_hip", "-Wl,-rpath," + HERE]
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return HARNESS_BIN


PROBE_DIR = os.path.join(HERE, "..", "tests", "cpp")
PROBE_SRC = os.path.join(PROBE_DIR, "gemm_probe.hip")
PROBE_BIN = os.path.join(PROBE_DIR, "gemm_probe")
PROBE_STAMP = os.path.join(PROBE_DIR, ".gemm_probe_stamp")


def compile_gemm_probe(obj: str) -> str:
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-c", PROBE_SRC, "-o", obj])
    return obj


def build_gemm_probe(verbose: bool = True) -> str:
    """tests/cpp/gemm_probe.hip (the stand-alone GEMM probe of tests/test_gpu_gemm_exact.py) linked against the kernel objects of the
    library build: they are self-contained (Knobs, use_knobs and every launch_* live in them).  The probe is compiled to an object first
    (object files on the line of a .hip source would be read as HIP source).  Content-stamped like the library.  Built by the test that
    runs it, not by build(): the library build depends on nothing under tests/."""
    import hashlib
    build(verbose=verbose)
    h = hashlib.sha256(_sources_digest().encode())
    for src in (PROBE_SRC, os.path.join(PROBE_DIR, "gemm_probe_plan.h")):
        with open(src, "rb") as f:
            h.update(f.read())
    if os.path.exists(PROBE_BIN) and os.path.exists(PROBE_STAMP) and open(PROBE_STAMP).read().strip() == h.hexdigest():
        return PROBE_BIN
    parts = [os.path.join(CSRC, f"rwkv_kernels.p{k}.o") for k in range(KERNEL_PARTS)]
    if not all(os.path.exists(p) for p in parts):
        build(force=True, verbose=verbose)
    obj = compile_gemm_probe(os.path.join(PROBE_DIR, "gemm_probe.o"))
    cmd = [_hipcc(), "--offload-arch=gfx950", obj] + parts + ["-o", PROBE_BIN]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(PROBE_STAMP, "w") as f:
        f.write(h.hexdigest())
    return PROBE_BIN


ROW_PROBE_SRC = os.path.join(PROBE_DIR, "row_probe.hip")
ROW_PROBE_BIN = os.path.join(PROBE_DIR, "row_probe")
ROW_PROBE_STAMP = os.path.join(PROBE_DIR, ".row_probe_stamp")


def compile_row_probe(obj: str) -> str:
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-c", ROW_PROBE_SRC, "-o", obj])
    return obj


def build_row_probe(verbose: bool = True) -> str:
    """tests/cpp/row_probe.hip (the stand-alone row / WKV / state probe of tests/test_gpu_row_exact.py), linked and content-stamped like
    the GEMM probe above.  Built by the test that runs it, not by build()."""
    import hashlib
    build(verbose=verbose)
    h = hashlib.sha256(_sources_digest().encode())
    with open(ROW_PROBE_SRC, "rb") as f:
        h.update(f.read())
    if os.path.exists(ROW_PROBE_BIN) and os.path.exists(ROW_PROBE_STAMP) and open(ROW_PROBE_STAMP).read().strip() == h.hexdigest():
        return ROW_PROBE_BIN
    parts = [os.path.join(CSRC, f"rwkv_kernels.p{k}.o") for k in range(KERNEL_PARTS)]
    if not all(os.path.exists(p) for p in parts):
        build(force=True, verbose=verbose)
    obj = compile_row_probe(os.path.join(PROBE_DIR, "row_probe.o"))
    cmd = [_hipcc(), "--offload-arch=gfx950", obj] + parts + ["-o", ROW_PROBE_BIN]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(ROW_PROBE_STAMP, "w") as f:
        f.write(h.hexdigest())
    return ROW_PROBE_BIN


MIX_PROBE_SRC = os.path.join(PROBE_DIR, "mix_probe.hip")
MIX_PROBE_BIN = os.path.join(PROBE_DIR, "mix_probe")
MIX_PROBE_STAMP = os.path.join(PROBE_DIR, ".mix_probe_stamp")


def compile_mix_probe(obj: str) -> str:
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-c", MIX_PROBE_SRC, "-o", obj])
    return obj


def build_mix_probe(verbose: bool = True) -> str:
    """tests/cpp/mix_probe.hip (the stand-alone V6 mix / LayerNorm prologue / shift commit probe of tests/test_gpu_mix_exact.py), linked and
    content-stamped like the two probes above.  Built by the test that runs it, not by build()."""
    import hashlib
    build(verbose=verbose)
    h = hashlib.sha256(_sources_digest().encode())
    for src in (MIX_PROBE_SRC, os.path.join(PROBE_DIR, "mix_probe_plan.h")):
        with open(src, "rb") as f:
            h.update(f.read())
    if os.path.exists(MIX_PROBE_BIN) and os.path.exists(MIX_PROBE_STAMP) and open(MIX_PROBE_STAMP).read().strip() == h.hexdigest():
        return MIX_PROBE_BIN
    parts = [os.path.join(CSRC, f"rwkv_kernels.p{k}.o") for k in range(KERNEL_PARTS)]
    if not all(os.path.exists(p) for p in parts):
        build(force=True, verbose=verbose)
    obj = compile_mix_probe(os.path.join(PROBE_DIR, "mix_probe.o"))
    cmd = [_hipcc(), "--offload-arch=gfx950", obj] + parts + ["-o", MIX_PROBE_BIN]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(MIX_PROBE_STAMP, "w") as f:
        f.write(h.hexdigest())
    return MIX_PROBE_BIN


SAMPLE_PROBE_SRC = os.path.join(PROBE_DIR, "sample_probe.hip")
SAMPLE_PROBE_BIN = os.path.join(PROBE_DIR, "sample_probe")
SAMPLE_PROBE_STAMP = os.path.join(PROBE_DIR, ".sample_probe_stamp")


def compile_sample_probe(obj: str) -> str:
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-c", SAMPLE_PROBE_SRC, "-o", obj])
    return obj


def build_sample_probe(verbose: bool = True) -> str:
    """tests/cpp/sample_probe.hip (the stand-alone sampling / vocabulary-row probe of tests/test_gpu_sample_exact.py), linked and
    content-stamped like the three probes above.  Built by the test that runs it, not by build()."""
    import hashlib
    build(verbose=verbose)
    h = hashlib.sha256(_sources_digest().encode())
    with open(SAMPLE_PROBE_SRC, "rb") as f:
        h.update(f.read())
    if os.path.exists(SAMPLE_PROBE_BIN) and os.path.exists(SAMPLE_PROBE_STAMP) and open(SAMPLE_PROBE_STAMP).read().strip() == h.hexdigest():
        return SAMPLE_PROBE_BIN
    parts = [os.path.join(CSRC, f"rwkv_kernels.p{k}.o") for k in range(KERNEL_PARTS)]
    if not all(os.path.exists(p) for p in parts):
        build(force=True, verbose=verbose)
    obj = compile_sample_probe(os.path.join(PROBE_DIR, "sample_probe.o"))
    cmd = [_hipcc(), "--offload-arch=gfx950", obj] + parts + ["-o", SAMPLE_PROBE_BIN]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(SAMPLE_PROBE_STAMP, "w") as f:
        f.write(h.hexdigest())
    return SAMPLE_PROBE_BIN


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)

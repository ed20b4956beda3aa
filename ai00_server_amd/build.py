"""Build librwkv_hip.so in-tree with hipcc for gfx950 (no cmake needed; ~40 s cold).

    python -m ai00_server_amd.build [--force]
"""
from __future__ import annotations

import functools
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librwkv_hip.so")
SOURCES = ["rwkv_kernels.hip", "rwkv_engine.cpp", "tokenizer.cpp", "rwkv_dfa.cpp", "rwkv_pda.cpp"]
DEPS = SOURCES + ["rwkv_kernels.h", "gemm_plan.h", "graph_cache.h", "gen_host.h", "gen_stop.h", "gen_dfa.h", "rwkv_dfa.h", "gen_pda.h", "gen_watch.h", "rwkv_pda.h", "safetensors.hpp", "rwkv_abi.map", os.path.join("..", "..", "include", "rwkv_abi.h"),
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
PROBE_SHARED = ("probe_common.h", "probe_case.h")
# tests/cpp/<name>.hip, the stand-alone kernel probe of tests/test_gpu_<family>_exact.py (sf4_probe: tests/test_gpu_sf4.py) -> the headers beside it that enter its stamp
PROBES = {"gemm_probe": ("gemm_probe_plan.h",), "row_probe": (), "mix_probe": ("mix_probe_plan.h",), "sample_probe": (), "topn_probe": (),
          "gen_probe": (), "sf4_probe": ("gemm_probe_plan.h",)}


def kernel_objects() -> list:
    """The objects the library build leaves behind for rwkv_kernels.hip: self-contained (Knobs, use_knobs and every launch_* live in them)."""
    return [os.path.join(CSRC, f"rwkv_kernels.p{k}.o") for k in range(KERNEL_PARTS)]


def compile_probe(name: str, obj: str) -> str:
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-c", os.path.join(PROBE_DIR, name + ".hip"), "-o", obj])
    return obj


def build_probe(name: str, verbose: bool = True) -> str:
    """A probe of PROBES linked against the kernel objects of the library build.  The probe is compiled to an object first (object files on
    the line of a .hip source would be read as HIP source).  Content-stamped like the library.  Built by the test that runs it, not by
    build(): the library build depends on nothing under tests/."""
    import hashlib
    exe, stamp = os.path.join(PROBE_DIR, name), os.path.join(PROBE_DIR, f".{name}_stamp")
    build(verbose=verbose)
    h = hashlib.sha256(_sources_digest().encode())
    for src in (name + ".hip",) + PROBES[name] + PROBE_SHARED:
        path = os.path.join(PROBE_DIR, src)
        if src.endswith(".hip") or os.path.exists(path):               # a header that is not there is included by nothing that compiles
            with open(path, "rb") as f:
                h.update(f.read())
    if os.path.exists(exe) and os.path.exists(stamp) and open(stamp).read().strip() == h.hexdigest():
        return exe
    parts = kernel_objects()
    if not all(os.path.exists(p) for p in parts):
        build(force=True, verbose=verbose)
    obj = compile_probe(name, os.path.join(PROBE_DIR, name + ".o"))
    cmd = [_hipcc(), "--offload-arch=gfx950", obj] + parts + ["-o", exe]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(stamp, "w") as f:
        f.write(h.hexdigest())
    return exe


# The per-probe names of earlier revisions, which test modules of those revisions still call: compile_row_probe(obj), build_row_probe(verbose=False), ...
for _name in PROBES:
    globals()["compile_" + _name] = functools.partial(compile_probe, _name)
    globals()["build_" + _name] = functools.partial(build_probe, _name)


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)

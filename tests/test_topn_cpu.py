"""CPU: the host-only side of top-n lists on the device (include/rwkv_abi.h `rwkv_topn_rows` / `rwkv_infer_topn` / `rwkv_gen_set_topn` /
`rwkv_gen_run_topn`, additive under ABI 9): the exports, the agreement of the header, the Rust `-sys` crate and runtime.py, argument checking
that never aborts, and the C++ Scheduler's `top_logprobs` option on a fake engine.  No compute call is made: the library loads without a GPU."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

from ai00_server_amd import harness, runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rwkv_topn_rows", "rwkv_infer_topn", "rwkv_gen_set_topn", "rwkv_gen_run_topn")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_four_symbols_are_exported_and_the_abi_version_is_still_9(built_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    script = read("ai00_server_amd", "csrc", "rwkv_abi.map")
    globs = [p.strip() for p in re.search(r"global:(.*?)local:", script, re.S).group(1).split(";") if p.strip()]
    for name in NEW:
        assert name in exported and hasattr(rt.lib(), name)
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), (name, globs)
    assert rt.lib().rwkv_abi_version() == 9
    header = read("include", "rwkv_abi.h")
    assert re.search(r"#define\s+RWKV_ABI_VERSION\s+9\b", header)
    assert re.search(r"additive under 9: rwkv_topn_rows, rwkv_infer_topn, rwkv_gen_set_topn, rwkv_gen_run_topn", header), "the version comment names the four symbols"


def c_decl(header, name):
    m = re.search(r"rwkv_status\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def rust_decl(rs, name):
    m = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)\s*->\s*rwkv_status\s*;", rs)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_sys_crate_and_runtime_py_agree_on_the_new_functions():
    header = read("include", "rwkv_abi.h")
    rs = read("integration", "rwkv-hip-sys", "src", "lib.rs")
    u32p, f32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    want = {
        "rwkv_topn_rows": (["rwkv_engine *e", "const float *const *in", "int32_t n", "uint32_t *out_ids", "float *out_logp", "size_t n_rows"],
                           ["e: *mut rwkv_engine", "inp: *const *const f32", "n: i32", "out_ids: *mut u32", "out_logp: *mut c_float", "n_rows: usize"],
                           [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, u32p, f32p, C.c_size_t]),
        "rwkv_infer_topn": (["rwkv_engine *e", "const rwkv_slot_input *in", "int32_t n", "uint32_t *const *out_ids", "float *const *out_logp",
                             "const uint32_t *const *targets", "float *const *out_tok_logp", "size_t *n_rows", "size_t *n_consumed"],
                            ["e: *mut rwkv_engine", "inp: *const rwkv_slot_input", "n: i32", "out_ids: *const *mut u32", "out_logp: *const *mut c_float",
                             "targets: *const *const u32", "out_tok_logp: *const *mut c_float", "n_rows: *mut usize", "n_consumed: *mut usize"],
                            [C.c_void_p, C.POINTER(rt._SlotInC), C.c_int32, C.POINTER(u32p), C.POINTER(f32p), C.POINTER(u32p), C.POINTER(f32p),
                             C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "rwkv_gen_set_topn": (["rwkv_engine *e", "int32_t slot", "int32_t n"], ["e: *mut rwkv_engine", "slot: i32", "n: i32"], [C.c_void_p, C.c_int32, C.c_int32]),
        "rwkv_gen_run_topn": (["rwkv_engine *e", "int32_t n_steps", "uint32_t *out_tokens", "float *out_probs", "int32_t *n_emitted", "int32_t *finish",
                               "int32_t n_top", "float *out_tok_logp", "uint32_t *out_top_ids", "float *out_top_logp"],
                              ["e: *mut rwkv_engine", "n_steps: i32", "out_tokens: *mut u32", "out_probs: *mut c_float", "n_emitted: *mut i32", "finish: *mut i32",
                               "n_top: i32", "out_tok_logp: *mut c_float", "out_top_ids: *mut u32", "out_top_logp: *mut c_float"],
                              [C.c_void_p, C.c_int32, u32p, f32p, i32p, i32p, C.c_int32, f32p, u32p, f32p]),
    }
    for name, (c_args, r_args, py_args) in want.items():
        assert c_decl(header, name) == c_args
        assert rust_decl(rs, name) == r_args
        res, args = rt.ABI_SYMBOLS[name]
        assert res is C.c_int32 and args == py_args
    # rwkv_gen_run_topn's first six arguments are rwkv_gen_run's
    assert c_decl(header, "rwkv_gen_run_topn")[:6] == c_decl(header, "rwkv_gen_run")
    # the constants: one value in the header, the sys crate, the kernels' header and runtime.py
    top = int(re.search(r"#define\s+RWKV_TOPN_MAX\s+(\d+)\b", header).group(1))
    none = int(re.search(r"#define\s+RWKV_TOPN_NONE\s+(\d+)u", header).group(1))
    assert (top, none) == (32, 0xFFFFFFFF) == (rt.TOPN_MAX, rt.TOPN_NONE)
    assert int(re.search(r"pub const RWKV_TOPN_MAX: i32 = (\d+);", rs).group(1)) == top
    assert int(re.search(r"pub const RWKV_TOPN_NONE: u32 = (\d+);", rs).group(1)) == none
    kh = read("ai00_server_amd", "csrc", "rwkv_kernels.h")
    assert re.search(r"constexpr int TOPN_MAX = 32;", kh) and re.search(r"constexpr unsigned TOPN_NONE = 0xFFFFFFFFu;", kh)
    # the safe wrapper, the C++ Runtime, the C++ Scheduler, the harness and the Python Runtime all spell the calls
    safe = read("integration", "rwkv-hip", "src", "lib.rs")
    hpp = read("include", "rwkv_runtime.hpp")
    for needle in ("topn_rows", "infer_topn", "gen_set_topn"):
        assert f"pub fn {needle}" in safe and needle in hpp and hasattr(rt.Runtime, needle)
    assert "pub fn gen_run_topn" in safe and "rwkv_gen_run_topn" in hpp and "top" in rt.Runtime.gen_run.__code__.co_varnames
    assert "top_logprobs" in read("include", "rwkv_scheduler.hpp") and "top_logprobs" in harness.generate_resident.__code__.co_varnames
    md = read("INTEGRATION.md")
    assert all(name in md for name in NEW)
    assert "rwkv_infer_sample returns no lists" in header                # the out-of-scope case and what its caller does instead


def test_new_calls_reject_null_and_out_of_range_arguments_without_aborting(built_lib):
    l = rt.lib()
    B = 2
    ins = (rt._SlotInC * B)()
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    ids, lp = (C.c_uint32 * 64)(*([7] * 64)), (C.c_float * 64)(*([7.0] * 64))
    row = np.zeros(16, np.float32)
    rows = (C.c_void_p * 1)(row.ctypes.data)
    pid, plp = (u32p * B)(), (f32p * B)()
    n_rows, consumed = (C.c_size_t * B)(5, 5), (C.c_size_t * B)(5, 5)
    fake = C.c_void_p(0x1000)                                          # never dereferenced: the range check comes first
    calls = [
        (l.rwkv_topn_rows, (None, rows, 5, ids, lp, 1)),
        (l.rwkv_topn_rows, (fake, None, 5, ids, lp, 1)),
        (l.rwkv_topn_rows, (fake, rows, 5, None, lp, 1)),
        (l.rwkv_topn_rows, (fake, rows, 5, ids, None, 1)),
        (l.rwkv_topn_rows, (fake, rows, 0, ids, lp, 1)),
        (l.rwkv_topn_rows, (fake, rows, 33, ids, lp, 1)),
        (l.rwkv_topn_rows, (fake, rows, -1, ids, lp, 0)),
        (l.rwkv_infer_topn, (None, ins, 5, pid, plp, None, None, n_rows, consumed)),
        (l.rwkv_infer_topn, (fake, None, 5, pid, plp, None, None, n_rows, consumed)),
        (l.rwkv_infer_topn, (fake, ins, 5, None, plp, None, None, n_rows, consumed)),
        (l.rwkv_infer_topn, (fake, ins, 5, pid, None, None, None, n_rows, consumed)),
        (l.rwkv_infer_topn, (fake, ins, 5, pid, plp, None, None, None, consumed)),
        (l.rwkv_infer_topn, (fake, ins, 5, pid, plp, None, None, n_rows, None)),
        (l.rwkv_infer_topn, (fake, ins, 0, pid, plp, None, None, n_rows, consumed)),
        (l.rwkv_infer_topn, (fake, ins, 33, pid, plp, None, None, n_rows, consumed)),
        (l.rwkv_gen_set_topn, (None, 0, 5)),
        (l.rwkv_gen_run_topn, (None, 1, ids, lp, None, None, 5, lp, ids, lp)),
        (l.rwkv_gen_run_topn, (fake, 1, ids, lp, None, None, 5, None, ids, lp)),
        (l.rwkv_gen_run_topn, (fake, 1, ids, lp, None, None, 5, lp, None, lp)),
        (l.rwkv_gen_run_topn, (fake, 1, ids, lp, None, None, 5, lp, ids, None)),
        (l.rwkv_gen_run_topn, (fake, 1, ids, lp, None, None, 0, lp, ids, lp)),
        (l.rwkv_gen_run_topn, (fake, 1, ids, lp, None, None, 33, lp, ids, lp)),
        (l.rwkv_gen_run_topn, (fake, 0, ids, lp, None, None, 5, lp, ids, lp)),
    ]
    for call, args in calls:
        assert call(*args) == -1, (call.__name__, args)
        assert l.rwkv_last_error() != b"", call.__name__
    # nothing was written
    assert list(ids) == [7] * 64 and list(lp) == [7.0] * 64 and list(n_rows) == [5, 5] and list(consumed) == [5, 5]


def test_cpp_scheduler_top_logprobs_reaches_gen_set_topn_on_a_fake_engine(built_lib, tmp_path):
    """include/rwkv_scheduler.hpp `arm_with_stops(..., top_logprobs)` (tests/cpp/topn_scheduler_test.cpp): the option reaches gen_set_topn
    behind the arm, 0 tells the engine nothing, a count out of range is refused before the slot is armed."""
    exe = str(tmp_path / "topn_scheduler_test")
    pkg = os.path.join(ROOT, "ai00_server_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "topn_scheduler_test.cpp"), "-o", exe,
                           "-L" + pkg, "-lrwkv_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "topn_scheduler_test: ok" in out.stdout, out.stdout + out.stderr

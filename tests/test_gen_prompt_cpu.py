"""CPU: the host-only side of admission into resident generation (ABI 9, include/rwkv_abi.h `rwkv_gen_arm_prompt` /
`rwkv_gen_prompt_left`): the version, the exports, the agreement of the header, the Rust `-sys` crate and runtime.py on the two new
functions, argument checking that never aborts, and the first draw's uniform (draw 0), which must not have moved.
No compute call is made: the library loads without a GPU."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

from ai00_server_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rwkv_gen_arm_prompt", "rwkv_gen_prompt_left")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_abi_version_is_9_and_the_header_history_says_why(built_lib):
    assert rt.lib().rwkv_abi_version() == 9
    header = read("include", "rwkv_abi.h")
    assert re.search(r"#define\s+RWKV_ABI_VERSION\s+9\b", header)
    assert re.search(r"^\s*\*\s*9:.*rwkv_gen_arm_prompt", header, re.M), "the version comment needs its '9:' line"


def test_both_symbols_are_exported_and_covered_by_the_version_script(built_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert name in exported
        assert hasattr(rt.lib(), name)
    # the version script exports by pattern: every new name must match one of its `global:` patterns
    script = read("ai00_server_amd", "csrc", "rwkv_abi.map")
    pats = re.search(r"global:(.*?)local:", script, re.S).group(1)
    globs = [p.strip() for p in pats.split(";") if p.strip()]
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), (name, globs)


def c_decl(header, name):
    m = re.search(r"rwkv_status\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def rust_decl(rs, name):
    m = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)\s*->\s*rwkv_status\s*;", rs)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_sys_crate_and_runtime_py_agree_on_the_new_functions():
    header = read("include", "rwkv_abi.h")
    rs = read("integration", "rwkv-hip-sys", "src", "lib.rs")
    want = {
        "rwkv_gen_arm_prompt": (["rwkv_engine *e", "int32_t slot", "const uint32_t *tokens", "size_t n_tokens", "const rwkv_gen_params *p"],
                                ["e: *mut rwkv_engine", "slot: i32", "tokens: *const u32", "n_tokens: usize", "p: *const rwkv_gen_params"],
                                [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(rt._GenParamsC)]),
        "rwkv_gen_prompt_left": (["const rwkv_engine *e", "int32_t slot", "size_t *left"],
                                 ["e: *const rwkv_engine", "slot: i32", "left: *mut usize"],
                                 [C.c_void_p, C.c_int32, C.POINTER(C.c_size_t)]),
    }
    for name, (c_args, r_args, py_args) in want.items():
        assert c_decl(header, name) == c_args
        assert rust_decl(rs, name) == r_args
        res, args = rt.ABI_SYMBOLS[name]
        assert res is C.c_int32 and args == py_args
    # the safe wrapper, the C++ Runtime and the Python Runtime all spell the pair
    safe = read("integration", "rwkv-hip", "src", "lib.rs")
    hpp = read("include", "rwkv_runtime.hpp")
    for needle in ("gen_arm_prompt", "gen_prompt_left"):
        assert f"pub fn {needle}" in safe and needle in hpp and hasattr(rt.Runtime, needle)
    assert "gen_params_for_prompt" in read("include", "rwkv_sampler.hpp")
    assert 'version = "0.9.' in read("integration", "rwkv-hip-sys", "Cargo.toml")


def test_new_calls_reject_null_arguments_without_aborting(built_lib):
    l = rt.lib()
    p = rt._GenParamsC()
    toks = (C.c_uint32 * 4)(1, 2, 3, 4)
    left = C.c_size_t(7)
    assert l.rwkv_gen_arm_prompt(None, 0, toks, 4, C.byref(p)) == -1 and l.rwkv_last_error() == b"null engine"
    assert l.rwkv_gen_arm_prompt(None, 0, None, 0, None) == -1
    assert l.rwkv_gen_prompt_left(None, 0, C.byref(left)) == -1 and l.rwkv_last_error() == b"null engine"
    assert left.value == 7


def test_draw_zero_of_a_stream_is_unchanged(built_lib):
    """The first token of an admitted slot is drawn with step 0 of (seed, stream): the counter function's value there, restated."""
    def restate(seed, stream, step):
        M = (1 << 64) - 1
        z = (seed + 0x9E3779B97F4A7C15 * ((((stream << 32) | step) + 1) & M)) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        return np.float32(z >> 40) * np.float32(2.0 ** -24)
    for seed, stream in [(0, 0), (20251024, 3), ((1 << 64) - 1, (1 << 32) - 1), (7, 31)]:
        got = np.float32(rt.gen_uniform(seed, stream, 0))
        assert got.view(np.uint32) == restate(seed, stream, 0).view(np.uint32)
        assert np.float32(rt.gen_uniform(seed, stream, 0, 3)[0]).view(np.uint32) == got.view(np.uint32)
    # pinned: worked by hand from the formula in include/rwkv_abi.h for seed 0, stream 0, step 0:
    #   z = 0x9E3779B97F4A7C15 -> (z ^ z >> 30) * 0xBF58476D1CE4E5B9 -> (z ^ z >> 27) * 0x94D049BB133111EB -> z ^ z >> 31 = 0xE220A8397B1DCDAF
    #   u = (z >> 40) * 2^-24 = 0xE220A8 / 16777216
    assert rt.gen_uniform(0, 0, 0) == 0xE220A8 / 16777216.0

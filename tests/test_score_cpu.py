"""CPU: the host-only side of on-device scoring (include/rwkv_abi.h `rwkv_infer_score` / `rwkv_score_rows`, additive under ABI 9): the
exports, the agreement of the header, the Rust `-sys` crate and runtime.py, argument checking that never aborts, `harness.perplexity_scored`
against the reference formula on an oracle-backed runtime, and the C++ `Scheduler::choose_scored` against `choose` on a fake engine.
No compute call is made: the library loads without a GPU."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

from ai00_server_amd import runtime as rt
from ai00_server_amd.harness import InferLoop, perplexity, perplexity_scored
from oracle import rwkv_ref as R
from tests.fakes import OracleRuntime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rwkv_infer_score", "rwkv_score_rows")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_both_symbols_are_exported_and_the_abi_version_is_still_9(built_lib):
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
    assert re.search(r"additive under 9.*rwkv_infer_score, rwkv_score_rows", header), "the version comment records the additive symbols under 9"
    assert 'version = "0.9.0"' in read("integration", "rwkv-hip-sys", "Cargo.toml")


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
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    want = {
        "rwkv_score_rows": (["rwkv_engine *e", "const float *const *in", "const uint32_t *targets", "float *out_logp", "size_t n_rows"],
                            ["e: *mut rwkv_engine", "inp: *const *const f32", "targets: *const u32", "out_logp: *mut c_float", "n_rows: usize"],
                            [C.c_void_p, C.POINTER(C.c_void_p), u32p, f32p, C.c_size_t]),
        "rwkv_infer_score": (["rwkv_engine *e", "const rwkv_slot_input *in", "const uint32_t *const *targets", "float *const *out_logp", "size_t *n_consumed"],
                             ["e: *mut rwkv_engine", "inp: *const rwkv_slot_input", "targets: *const *const u32", "out_logp: *const *mut c_float",
                              "n_consumed: *mut usize"],
                             [C.c_void_p, C.POINTER(rt._SlotInC), C.POINTER(u32p), C.POINTER(f32p), C.POINTER(C.c_size_t)]),
    }
    for name, (c_args, r_args, py_args) in want.items():
        assert c_decl(header, name) == c_args
        assert rust_decl(rs, name) == r_args
        res, args = rt.ABI_SYMBOLS[name]
        assert res is C.c_int32 and args == py_args
    # the constant: one value in the header, the sys crate and runtime.py
    skip = int(re.search(r"#define\s+RWKV_SCORE_SKIP\s+(\d+)u", header).group(1))
    assert skip == 0xFFFFFFFF == rt.SCORE_SKIP
    assert int(re.search(r"pub const RWKV_SCORE_SKIP: u32 = (\d+);", rs).group(1)) == skip
    # the safe wrapper, the C++ Runtime, the C++ Scheduler and the Python side all spell the calls
    safe = read("integration", "rwkv-hip", "src", "lib.rs")
    hpp = read("include", "rwkv_runtime.hpp")
    for needle in ("infer_score", "score_rows"):
        assert f"pub fn {needle}" in safe and needle in hpp and hasattr(rt.Runtime, needle)
    sched = read("include", "rwkv_scheduler.hpp")
    assert "perplexity_scored" in sched and "choose_scored" in sched
    md = read("INTEGRATION.md")
    assert "rwkv_infer_score" in md and "rwkv_score_rows" in md and "699-755" in md and "936-982" in md


def test_new_calls_reject_null_arguments_without_aborting(built_lib):
    l = rt.lib()
    B = 2
    ins = (rt._SlotInC * B)()
    tp, op = (C.POINTER(C.c_uint32) * B)(), (C.POINTER(C.c_float) * B)()
    consumed = (C.c_size_t * B)(7, 7)
    assert l.rwkv_infer_score(None, ins, tp, op, consumed) == -1 and l.rwkv_last_error() == b"null argument"
    assert l.rwkv_infer_score(None, None, None, None, None) == -1
    assert list(consumed) == [7, 7]
    row = np.zeros(16, np.float32)
    pi = (C.c_void_p * 1)(row.ctypes.data)
    tg = (C.c_uint32 * 1)(3)
    out = (C.c_float * 1)(5.0)
    assert l.rwkv_score_rows(None, pi, tg, out, 1) == -1 and l.rwkv_last_error() == b"null argument"
    assert l.rwkv_score_rows(None, None, None, None, 1) == -1
    assert out[0] == 5.0


class ScoringOracleRuntime(OracleRuntime):
    """OracleRuntime plus `infer_score` / `score_rows`: the oracle's `Full` rows scored with a float64 log-softmax."""

    @staticmethod
    def _logp(row, t):
        x = row.astype(np.float64)
        m = x.max()
        return float((x[t] - m) - np.log(np.exp(x - m).sum()))

    def infer_score(self, inp, targets):
        for b, ib in enumerate(inp.batches):
            if targets[b] is not None:
                assert len(targets[b]) == len(ib.tokens)
                ib.option = rt.RnnOption.Full
            else:
                assert not len(ib.tokens) or ib.option == rt.RnnOption.NoOutput
        inp, outs = self.infer(inp)
        rest, scores = [], []
        for b, rows in enumerate(outs):
            if targets[b] is None:
                rest.append(None)
                scores.append(np.empty(0, np.float32))
                continue
            n = len(rows)
            scores.append(np.array([np.nan if t == rt.SCORE_SKIP else self._logp(r, t) for r, t in zip(rows, targets[b][:n])], np.float32))
            rest.append(targets[b][n:])
        return inp, rest, scores

    def score_rows(self, rows, targets):
        return np.array([self._logp(np.asarray(r), t) for r, t in zip(rows, targets)], np.float32)


def test_perplexity_scored_matches_the_reference_formula_with_and_without_head():
    ref = R.RwkvRef(R.synth_named("v7-tiny"))
    V = ref.info.num_vocab
    choice = [t % V for t in R.synth_prompt(4, 7)]
    # without head: token 0 is prepended and counted in the denominator
    rt_ = ScoringOracleRuntime(ref, max_batch=2, token_chunk_size=4)
    got = perplexity_scored(InferLoop(rt_), 1, choice)
    rows = ref.forward([0] + choice, ref.init_state(), full=True)
    want = R.perplexity_ref(rows, choice)
    assert abs(got - want) < 1e-5, (got, want)
    assert rt_.calls >= 2                                            # 8 tokens through a 4-token chunk: the request straddles calls
    assert abs(perplexity_scored(ScoringOracleRuntime(ref, max_batch=1, token_chunk_size=4), 0, choice) - want) < 1e-5   # a bare runtime works too
    # with head: the probability of choice[0] on the prompt's last row
    prompt = [t % V for t in R.synth_prompt(5, 9)]
    s = ref.init_state()
    last = ref.forward(prompt, s)[-1]
    rt_ = ScoringOracleRuntime(ref, max_batch=1, token_chunk_size=4)
    rt_.states[0] = s.copy()
    head = float(np.exp(rt_.score_rows([last], [choice[0]])[0]))
    got = perplexity_scored(rt_, 0, choice, head=head)
    want = R.perplexity_ref(ref.forward(choice, s, full=True), choice, head)
    assert abs(got - want) < 1e-5, (got, want)
    # and it is the old path's answer
    s2 = ref.init_state()
    ref.forward(prompt, s2)
    rt_.states[0] = s2
    assert abs(perplexity(InferLoop(rt_), 0, choice, head) - got) < 1e-5


def test_cpp_choose_scored_equals_choose_on_a_fake_engine(built_lib, tmp_path):
    """include/rwkv_scheduler.hpp `choose_scored` / `perplexity_scored` against `choose` / `perplexity` (tests/cpp/score_scheduler_test.cpp):
    with and without `calibrate` the same ranking, values within 1e-5, the slot's state restored."""
    exe = str(tmp_path / "score_scheduler_test")
    pkg = os.path.join(ROOT, "ai00_server_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "score_scheduler_test.cpp"), "-o", exe,
                           "-L" + pkg, "-lrwkv_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "score_scheduler_test: ok" in out.stdout, out.stdout + out.stderr

"""CPU: the record ring of a watch (rwkv_gen_watch_*; ai00_server_amd/csrc/gen_watch.h) and its surface.

The protocol — a sequence lock per record, a writer that never waits, a reader that never returns a torn record — is one header of
host/device functions.  tests/cpp/gen_watch_test.cpp compiles that header with g++ and drives the writer gen_publish_kernel uses and the
reader rwkv_gen_watch_read uses, on one thread and on two.  It is built three times: plain, with ThreadSanitizer (on the host every
payload word is a relaxed atomic, so the protocol is race-free in the C++ sense and the sanitizer holds it to that) and with
AddressSanitizer + UBSan.  The programs stand alone: nothing is loaded into Python.  The device side runs in tests/test_gpu_gen_watch.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "gen_watch_test.cpp")
N = 100000
BUILDS = {"plain": [], "tsan": ["-g", "-fsanitize=thread", "-Wno-tsan"], "asan_ubsan": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gen_watch") / f"gen_watch_test_{request.param}")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + BUILDS[request.param] + [SRC, "-o", exe])
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "WARNING: ThreadSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-400:] + r.stderr[-2000:]
    return r.stdout


def test_single_thread_cases(program):
    """empty ring, in-order reads, ring_steps = 1, a reader exactly ring_steps behind (loses nothing) and ring_steps + 3 behind (lost = 3,
    the oldest record then intact), max_steps smaller than what is available; cursor and head after each"""
    assert run(program, "single") == "single ok\n"


def test_two_threads_without_a_lap_lose_nothing(program):
    """N records of 3 slots into a ring of N steps while the reader drains: lost == 0, all N back in order, every word its function"""
    out = run(program, "nolap", str(N))
    assert out == f"nolap ok: ring_steps {N}, records {N}, returned {N}, lost 0\n"


def test_two_threads_with_an_unpaced_writer_never_see_a_torn_record(program):
    """ring_steps = 8 and a writer that does not wait: every record returned matches its function (the program exits non-zero on the first
    word that does not), the sequence numbers strictly increase, returned + lost == N.  No share of returned records is asked for."""
    out = run(program, "lap", str(N))
    m = re.fullmatch(r"lap ok: ring_steps 8, records (\d+), returned (\d+), lost (\d+)\n", out)
    assert m, out
    n, returned, lost = map(int, m.groups())
    assert n == N and returned + lost == N


def test_the_surface_is_additive_and_checks_its_arguments(built_lib):
    l = rt.lib()
    names = ("rwkv_gen_watch_open", "rwkv_gen_watch_close", "rwkv_gen_watch_head", "rwkv_gen_watch_read", "rwkv_gen_watch_cancel")
    for name in names:
        assert hasattr(C.CDLL(built_lib), name) and name in rt.ABI_SYMBOLS
    assert l.rwkv_abi_version() == 9                                      # additive: no existing symbol or struct changed
    h, seq, n, lost, cur = C.c_void_p(5), C.c_uint64(7), C.c_int32(7), C.c_uint64(7), C.c_uint64(7)
    tok = (C.c_uint32 * 4)()
    assert l.rwkv_gen_watch_open(None, 4, C.byref(h)) == -1 and l.rwkv_last_error() == b"null engine / out"
    assert l.rwkv_gen_watch_close(None, None) == -1
    assert l.rwkv_gen_watch_head(None, C.byref(seq)) == -1 and seq.value == 7
    assert l.rwkv_gen_watch_read(None, C.byref(cur), 1, tok, None, None, C.byref(n), C.byref(lost)) == -1 and (cur.value, n.value, lost.value) == (7, 7, 7)
    assert l.rwkv_gen_watch_cancel(None, 0) == -1 and l.rwkv_last_error() == b"null watch"
    assert rt.GenFinish.Cancelled == 4 and rt.GEN_WATCH_MAX_STEPS == 65536
    hdr = open(os.path.join(ROOT, "include", "rwkv_abi.h")).read()
    lim = {k: int(v) for k, v in re.findall(r"#define\s+(RWKV_GEN_\w+)\s+(\d+)", hdr)}
    assert lim["RWKV_GEN_CANCELLED"] == 4 and lim["RWKV_GEN_WATCH_MAX_STEPS"] == 65536
    for ref in ("run.rs:1009", "run.rs:934-935"):                           # the two lines of the reference's loop this stands for
        assert ref in hdr
    gw = open(os.path.join(ROOT, "ai00_server_amd", "csrc", "gen_watch.h")).read()
    assert re.search(r"GEN_FIN_CANCELLED\s*=\s*4", gw) and re.search(r"GEN_WATCH_MAX_STEPS\s*=\s*65536", gw)
    for name in ("gen_watch_open", ):
        assert callable(getattr(rt.Runtime, name))
    for name in ("read", "head", "cancel", "close"):
        assert callable(getattr(rt.GenWatch, name))
    assert callable(H.generate_resident_stream)
    hpp = open(os.path.join(ROOT, "include", "rwkv_runtime.hpp")).read()
    assert "class GenWatch" in hpp and all(n in hpp for n in names)

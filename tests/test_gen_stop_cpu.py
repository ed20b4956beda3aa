"""CPU: stop strings of resident generation (rwkv_gen_set_token_bytes / _set_stops / _stop_tail, additive under ABI 9) — everything of it
that runs without a GPU.

`ref_process` (tests/stop_ref.py) is a LITERAL transcription of the reference's per-token stop logic (crates/ai00-core/src/run.rs:855-869, 899-932,
990-1011) with `bytes.decode("utf-8")` standing for `String::from_utf8`.  Held to it, token by token (decision, head, buffer afterwards):
  - `harness.StopMatcher` (the Python host matcher),
  - `rwkv::StopMatcher` (include/rwkv_scheduler.hpp), and
  - the functions of ai00_server_amd/csrc/gen_stop.h driven in the kernel's order (append, scan per lane, order-keeping butterfly, decide,
    validate, trim) by tests/cpp/gen_stop_test.cpp — a stand-alone g++ program, which is also what a sanitizer build runs.
The device's one addition to the reference is its bounded buffer: a token whose bytes do not fit RWKV_GEN_STOP_BUF finishes with
RWKV_GEN_HANDBACK; that is asserted to happen exactly when the reference's buffer would pass the bound."""
import ctypes as C
import json
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt
from tests.stop_ref import CAP, expected, ref_min_by, ref_process, ref_scan   # noqa: F401  (the literal transcription: stated once, there)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_python(stops, tokens, max_tokens, tail=b"", emitted=0):
    m = H.StopMatcher(stops, tail, cap=CAP)
    out = []
    for i, (token, word) in enumerate(tokens):
        fin, content = m.advance(word, stop_token=token == 0, at_max=emitted + i + 1 >= max_tokens)
        out.append((fin, content, m.tail()))
        if fin:
            break
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gen_stop") / "gen_stop_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "gen_stop_test.cpp"), "-o", exe])
    return exe


def run_driver(exe, cases):
    """cases: [(stops, tokens, max_tokens, tail, emitted)] -> per case (kernel-order trace, rwkv::StopMatcher trace)"""
    hx = lambda b: b.hex() if b else "-"
    lines = []
    for stops, tokens, max_tokens, tail, emitted in cases:
        lines += ["case"] + ["stop " + hx(s) for s in stops] + ["tail " + hx(tail), f"max {max_tokens}", f"emitted {emitted}"]
        lines += [f"tok {'?' if w is None else hx(w)} {int(t == 0)}" for t, w in tokens]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("gen_stop_test: ok\n"), r.stdout[-400:] + r.stderr[-400:]
    un = lambda s: b"" if s == "-" else bytes.fromhex(s)
    res = []
    for ln in r.stdout.splitlines()[:-1]:
        if ln == "case":
            res.append(([], []))
            continue
        side, fin, head, buf = ln.split()
        res[-1][0 if side == "k" else 1].append((int(fin), un(head), un(buf)))
    return res


def same(got, want):
    assert len(got) == len(want), (got, want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[2] == w[2] and (w[1] is None or g[1] == w[1]), (i, g, w)


def check_all(driver, cases):
    res = run_driver(driver, cases)
    assert len(res) == len(cases)
    for case, (k, c) in zip(cases, res):
        want = expected(*case)
        same(run_python(*case), want)
        same(k, want)
        same(c, want)
    return [expected(*case) for case in cases]


def toks(*words, first_id=1):
    return [(first_id + i, w) for i, w in enumerate(words)]


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------
def test_new_calls_are_exported_additively_and_check_their_arguments(built_lib):
    l = rt.lib()
    for name in ("rwkv_gen_set_token_bytes", "rwkv_gen_set_stops", "rwkv_gen_stop_tail"):
        assert hasattr(C.CDLL(built_lib), name) and name in rt.ABI_SYMBOLS
    assert l.rwkv_abi_version() == 9                                      # additive: no existing symbol or struct changed
    lens = (C.c_int32 * 2)(1, 1)
    data = (C.c_uint8 * 2)(97, 98)
    assert l.rwkv_gen_set_token_bytes(None, data, lens, 2) == -1 and l.rwkv_last_error() == b"null engine"
    s = rt._GenStopsC()
    assert l.rwkv_gen_set_stops(None, 0, C.byref(s)) == -1 and l.rwkv_last_error() == b"null engine"
    n = C.c_size_t(7)
    assert l.rwkv_gen_stop_tail(None, 0, None, 0, C.byref(n)) == -1 and l.rwkv_last_error() == b"null engine" and n.value == 7
    assert rt.GenFinish.Handback == 3 == H.StopMatcher.HANDBACK
    hdr = open(os.path.join(ROOT, "include", "rwkv_abi.h")).read()
    lim = {k: int(v) for k, v in re.findall(r"#define\s+(RWKV_GEN_\w+)\s+(\d+)", hdr)}
    assert (lim["RWKV_GEN_MAX_STOP_STR"], lim["RWKV_GEN_STOP_LEN"], lim["RWKV_GEN_STOP_BUF"], lim["RWKV_GEN_TOKEN_LEN"]) == \
           (rt.GEN_MAX_STOP_STR, rt.GEN_STOP_LEN, rt.GEN_STOP_BUF, rt.GEN_TOKEN_LEN) == (8, 128, CAP, 256)
    assert re.search(r"RWKV_GEN_HANDBACK\s*=\s*3", hdr)
    assert "Stop STRINGS stay with the caller" not in hdr                  # the sentence that sent such callers to n_steps = 1
    body = re.search(r"struct rwkv_gen_stops\s*\{([^}]*)\}\s*;", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S), re.S).group(1)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in rt._GenStopsC._fields_] == ["strs", "lens", "n", "tail", "n_tail"]
    rs = open(os.path.join(ROOT, "integration", "rwkv-hip-sys", "src", "lib.rs")).read()
    rbody = re.search(r"#\[repr\(C\)\][^\n]*\n\s*pub struct rwkv_gen_stops\s*\{([^}]*)\}", rs, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", rbody) == names and C.sizeof(rt._GenStopsC) == 40


# ---- 2. named cases ----------------------------------------------------------------------------------------------------------------
def test_the_walk_is_not_a_substring_search(driver):
    case = ([b"ab"], toks(b"a", b"a", b"b", b"c"), 99, b"", 0)
    (want,) = check_all(driver, [case])
    assert [w[0] for w in want] == [0, 0, 0, 0] and b"ab" in b"aabc"      # a substring search would have stopped at the third token
    (want,) = check_all(driver, [([b"aab"], toks(b"a", b"a", b"a", b"b"), 99, b"", 0)])
    assert [w[0] for w in want] == [0, 0, 0, 0]
    (want,) = check_all(driver, [([b"ab"], toks(b"a", b"b"), 99, b"", 0)])
    assert [w[0] for w in want] == [0, 1] and want[1][1] == b""


def test_a_stop_that_spans_three_tokens(driver):
    (want,) = check_all(driver, [([b"\n\nUser:"], toks(b"Hi.", b"\n", b"\nUs", b"er:", b" x"), 99, b"", 0)])
    assert [w[0] for w in want] == [0, 0, 0, 1]
    assert [w[1] for w in want] == [b"Hi.", b"", b"", b""] and want[2][2] == b"\n\nUs"


def test_min_by_prefers_a_match_then_the_smaller_index_then_the_first(driver):
    # "xab": stop 0 ("zz") is unmatched with index_safe 3, stop 1 ("ab") matches at 1: matched first, though its index is smaller anyway ...
    (w1,) = check_all(driver, [([b"zz", b"ab"], toks(b"xab"), 99, b"", 0)])
    assert w1 == [(1, b"x", b"")]
    # ... and a matched stop with the LARGER index still beats an unmatched one with a smaller index
    (w2,) = check_all(driver, [([b"abq", b"b"], toks(b"ab"), 99, b"", 0)])      # "abq": unmatched, index 0; "b": matched at 1
    assert w2 == [(1, b"a", b"")]
    # a tie on (unmatched, index): the first stop is taken; both give index 0 over "a"
    (w3,) = check_all(driver, [([b"ab", b"ac"], toks(b"a", b"c"), 99, b"", 0)])
    assert w3 == [(0, b"", b"a"), (1, b"", b"a")]
    # two matched stops: the smaller index wins ("bc" matches at 1, "c" matches at 2)
    (w4,) = check_all(driver, [([b"c", b"bc"], toks(b"abc"), 99, b"", 0)])
    assert w4[0][:2] == (1, b"a")


def test_a_character_split_over_two_tokens_is_held_back_and_released(driver):
    zhong = "中".encode()                                                   # e4 b8 ad
    (want,) = check_all(driver, [([b"STOP"], toks(b"a", zhong[:2], zhong[2:] + b"b"), 99, b"", 0)])
    assert want == [(0, b"a", b""), (0, b"", zhong[:2]), (0, zhong + b"b", b"")]
    # overlong forms, surrogates and code points above U+10FFFF are not UTF-8 either: held, not sent
    for bad in (b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xe0\x80\xaf"):
        (want,) = check_all(driver, [([b"STOP"], toks(bad), 99, b"", 0)])
        assert want == [(0, b"", bad)]
        with pytest.raises(UnicodeDecodeError):
            bad.decode("utf-8")


def test_an_invalid_byte_grows_the_buffer_until_handback(driver):
    words = [b"\xff"] + [b"abcdefgh"] * 70
    (want,) = check_all(driver, [([b"never"], toks(*words), 999, b"", 0)])
    assert want[-1][0] == 3 and len(want) == 1 + 64 and len(want[-1][2]) == 1 + 63 * 8 == 505     # the 64th word would make 513 bytes
    assert all(w[0] == 0 and w[1] == b"" for w in want[:-1])
    # exactly full is still decided on the device
    (want,) = check_all(driver, [([b"never"], toks(b"\xff" + b"a" * 255, b"b" * 256, b"c"), 999, b"", 0)])
    assert [w[0] for w in want] == [0, 0, 3] and len(want[1][2]) == CAP


def test_empty_stop_unknown_id_token_zero_length_and_initial_tail(driver):
    (w,) = check_all(driver, [([b"x", b""], toks(b"hello"), 99, b"", 0)])
    assert w == [(1, b"", b"")]                                            # the empty stop string matches at once, at index 0
    (w,) = check_all(driver, [([b"zz"], [(5, b"a"), (6, None), (7, b"b")], 99, b"", 0)])
    assert [x[0] for x in w] == [0, 1]                                     # decode error: stop
    (w,) = check_all(driver, [([b"zz"], [(5, b"a"), (0, b"q"), (7, b"b")], 99, b"", 0)])
    assert [x[0] for x in w] == [0, 1]                                     # token 0 stops, whatever bytes the table gives it
    (w,) = check_all(driver, [([b"ab"], toks(b"a", b"b"), 2, b"", 0)])
    assert [x[0] for x in w] == [0, 1]                                     # max_tokens on the token of a match: Stop, not Length
    (w,) = check_all(driver, [([b"ab"], toks(b"a", b"c"), 2, b"", 0)])
    assert [x[0] for x in w] == [0, 2]
    (w,) = check_all(driver, [([b"\n\nUser:"], toks(b"User", b":"), 99, b"\n\n", 1)])   # the caller matched "\n\n" itself before arming
    assert [x[0] for x in w] == [0, 1]
    (w,) = check_all(driver, [([b"\n\nUser:"], toks(b"User", b":"), 99, b"", 1)])
    assert [x[0] for x in w] == [0, 0]
    assert H.StopMatcher([b"ab"]).replay([b"x", b"a", b"b", b"y"]) == ([b"x", b"", b""], 1)
    m = H.StopMatcher([b"ab"])
    assert m.push(b"xa") == (False, b"x") and m.tail() == b"a" and m.push(None) == (True, b"") and m.tail() == b"a"


# ---- 3. seeded fuzz -----------------------------------------------------------------------------------------------------------------
def test_seeded_fuzz_against_the_transcription(driver):
    rng = np.random.default_rng(20251110)
    frags = [b"a", b"b", b"c", "é".encode()[:1], "é".encode()[1:], "中".encode()[:2], "中".encode()[2:], "中".encode()[:1], b"\xff"]
    pick = lambda lo, hi: b"".join(frags[int(i)] for i in rng.integers(0, len(frags), int(rng.integers(lo, hi + 1))))[:6] or b"a"
    cases = []
    for c in range(400):
        abc = lambda lo, hi: bytes(rng.choice([97, 98, 99], int(rng.integers(lo, hi + 1))).tolist())
        stops = [abc(1, 6) if rng.random() < 0.8 else pick(1, 3) for _ in range(int(rng.integers(1, 9)))]
        if c % 8 == 0:
            stops = [b"z" + s for s in stops]                              # never matches: the alphabet has no z
        tokens = []
        for i in range(64):
            u = rng.random()
            word = abc(1, 6) if u < 0.55 else pick(1, 4)
            tokens.append((0, word) if u > 0.998 else (i + 1, None) if u > 0.996 else (i + 1, word))
        tail = b""
        if c % 8 == 0:                                                     # a buffer that is already long and cannot be sent: towards HANDBACK
            tail = b"\xff" + bytes(rng.choice([120, 121], int(rng.integers(250, 500))).tolist())
        cases.append((stops, tokens, int(rng.integers(40, 200)), tail, int(rng.integers(0, 3))))
    wants = check_all(driver, cases)
    count = dict(matched=0, substring_only=0, held=0, handback=0, length=0)
    for (stops, tokens, mx, tail, em), want in zip(cases, wants):
        buffer = tail
        for (tok, word), (fin, content, after) in zip(tokens, want):
            grown = buffer + (word or b"")
            if fin == 0 and any(s in grown for s in stops):
                count["substring_only"] += 1                               # a substring search would have stopped here
            if fin == 0 and content == b"" and after == grown and grown:
                try:
                    grown[:H.StopMatcher(stops).split(grown)[0]].decode()
                except UnicodeDecodeError:
                    count["held"] += 1
            if fin == 1 and tok != 0 and word is not None:
                count["matched"] += 1
            count["handback"] += fin == 3
            count["length"] += fin == 2
            buffer = after
    print(count)
    assert all(count[k] > 0 for k in ("matched", "substring_only", "held", "handback")), count   # a generator that stops biting fails here


# ---- 4. the real vocabulary ---------------------------------------------------------------------------------------------------------
def test_every_token_of_the_world_vocabulary_fits_the_token_table():
    raw = lzma.open(os.path.join(ROOT, "tests", "golden", "rwkv_vocab_v20230424.json.xz"), "rt", encoding="utf-8").read()
    vocab = {int(k): (v.encode("utf-8") if isinstance(v, str) else bytes(v)) for k, v in json.loads(raw).items()}
    longest = max(len(b) for b in vocab.values())
    print("longest token of the World vocabulary:", longest, "bytes")
    assert len(vocab) == 65529 and 0 < longest <= rt.GEN_TOKEN_LEN

"""CPU: the byte automata of the resident-generation constraint (rwkv_dfa_*, additive under ABI 9) — everything of it that runs without a
GPU, through ctypes on the library's host functions.

  - `rwkv_dfa_compile` against Python's `re` in bytes mode as the independent oracle.  `to_re` translates the dialect: `[^...]` and `.`
    become the explicit alternation of well-formed UTF-8 characters (Unicode table 3-7) outside the ASCII set, `\\s` the dialect's four
    bytes, a literal multi-byte character one group.  Acceptance = the walk from the start state ends in an accepting state.
  - canonical form: equivalent spellings give byte-identical tables.
  - `rwkv_dfa_allow` against a numpy walk written here, over the real World vocabulary.
  - every refusal of the header, the liveness rule included.
  - tests/cpp/gen_dfa_test.cpp (csrc/gen_dfa.h in the kernels' order) and tests/cpp/fuzz_dfa.cpp (stand-alone, built WITH the compiler's
    source under -fsanitize=address,undefined; nothing is preloaded into Python)."""
import json
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UTF8_TAIL = (rb"[\xC2-\xDF][\x80-\xBF]|\xE0[\xA0-\xBF][\x80-\xBF]|[\xE1-\xEC][\x80-\xBF][\x80-\xBF]|\xED[\x80-\x9F][\x80-\xBF]|[\xEE-\xEF][\x80-\xBF][\x80-\xBF]"
             rb"|\xF0[\x90-\xBF][\x80-\xBF][\x80-\xBF]|[\xF1-\xF3][\x80-\xBF][\x80-\xBF][\x80-\xBF]|\xF4[\x80-\x8F][\x80-\xBF][\x80-\xBF]")
CLASS_ESC = {ord("d"): set(range(48, 58)), ord("w"): set(range(48, 58)) | set(range(65, 91)) | set(range(97, 123)) | {95}, ord("s"): {32, 9, 13, 10}}
CHAR_ESC = {ord("n"): 10, ord("r"): 13, ord("t"): 9}


def _byte_re(c):
    return b"\\x%02x" % c


def _set_re(members):
    return b"[" + b"".join(_byte_re(c) for c in sorted(members)) + b"]" if members else b"(?!)"


def to_re(pat: bytes) -> bytes:
    """the dialect of rwkv_dfa_compile as a Python bytes regex (an independent reading of the header's description)"""
    out, i = [], 0
    while i < len(pat):
        c = pat[i]
        if c == 0x5C:                                                   # backslash
            e = pat[i + 1]
            if e in CLASS_ESC:
                out.append(_set_re(CLASS_ESC[e]))
                i += 2
            elif e == ord("x"):
                out.append(_byte_re(int(pat[i + 2:i + 4], 16)))
                i += 4
            else:
                out.append(_byte_re(CHAR_ESC.get(e, e)))
                i += 2
        elif c == ord("["):
            i += 1
            neg = pat[i] == ord("^")
            i += neg
            members = set()

            def one():
                nonlocal i
                if pat[i] == 0x5C:
                    e = pat[i + 1]
                    if e in CLASS_ESC:
                        i += 2
                        return CLASS_ESC[e]
                    if e == ord("x"):
                        v = int(pat[i + 2:i + 4], 16)
                        i += 4
                        return v
                    i += 2
                    return CHAR_ESC.get(e, e)
                i += 1
                return pat[i - 1]
            while pat[i] != ord("]"):
                lo = one()
                if isinstance(lo, set):
                    members |= lo
                    continue
                hi = lo
                if pat[i] == ord("-") and pat[i + 1] != ord("]"):
                    i += 1
                    hi = one()
                members |= set(range(lo, hi + 1))
            i += 1
            out.append(b"(?:" + _set_re(set(range(128)) - members) + b"|" + UTF8_TAIL + b")" if neg else _set_re(members))
        elif c == ord("."):
            out.append(b"(?:" + _set_re(set(range(128)) - {10}) + b"|" + UTF8_TAIL + b")")
            i += 1
        elif c >= 0x80:
            n = 2 if c < 0xE0 else 3 if c < 0xF0 else 4
            out.append(b"(?:" + b"".join(_byte_re(b) for b in pat[i:i + n]) + b")")
            i += n
        elif c in b"()|*+?":
            out.append(bytes([c]))
            i += 1
        elif c == ord("{"):
            j = pat.index(b"}", i)
            out.append(pat[i:j + 1])
            i = j + 1
        else:
            out.append(_byte_re(c))
            i += 1
    return b"".join(out)


ZH = "中".encode()
# (pattern, alphabet the random strings are drawn from, strings of the language)
PATTERNS = [
    (rb"abc", b"abcd", [b"abc"]),
    (rb"a{2,4}b{3}c{1,}", b"abc", [b"aabbbc", b"aaaabbbccc"]),
    (rb"(ab|cd)*e+f?", b"abcdef", [b"e", b"abcdeef", b"cdabe"]),
    (rb"(true|false|null)", b"truefalsn", [b"true", b"false", b"null"]),
    (rb"-?(0|[1-9]\d*)(\.\d+)?([eE][+-]?\d+)?", b"-0123456789.eE+", [b"0", b"-12.50", b"3e+8", b"10.0E-3"]),
    (rb"\d{4}-\d{2}-\d{2}", b"0123456789-", [b"2025-11-10"]),
    (rb'"([^"\\]|\\["\\/bfnrt]|\\u[0-9a-fA-F]{4})*"', b'"\\abnu0f/ \n' + ZH + b"\xff\x80", [b'""', b'"a\\n"', b'"' + ZH + b'\\u00fF"', b'"\\\\\\""']),
    (rb'\{"name":"[a-z]{1,8}","age":\d{1,3},"ok":(true|false)\}', b'{}"nameagok:,truefls0123456789', [b'{"name":"bo","age":41,"ok":true}', b'{"name":"abcdefgh","age":7,"ok":false}']),
    ("(中文|日本語)+é?".encode(), "中文日本語é".encode() + b"a", ["中文".encode(), "日本語中文é".encode()]),
    (rb"[^a-c]{2}" + ZH + rb"*", b"abcdxyz\n" + ZH + "é😀".encode() + b"\xed\xa0\x80\xc0\xaf", [b"xy", "é😀".encode() + ZH + ZH, b"d\n", ZH + ZH + ZH]),
    (rb".*\n", b"ab\n" + ZH + b"\xe4\xb8\xf0", [b"\n", b"ab" + ZH + b"\n"]),
    (rb"\w+\s\w+([.]|\x21|\?)?", b"aZ_9 \t\r\n\x0b.!?", [b"a b", b"Z_9\t9?", b"x\ny!", b"a\rb."]),
    (rb"(a|b|)c{0,2}[x\-z\]\\]", b"abcx-z]\\y", [b"x", b"acc-", b"bc]", b"c\\"]),
    (rb"[\x00-\x1f]\t[\d\-a]+", bytes(range(0, 32)) + b"\t09-ab", [b"\x00\t0", b"\x1f\t-a9"]),
]


def accepts(d, acc, s: bytes) -> bool:
    return bool(acc[d.walk(d.start, s)])


def mutations(rng, s: bytes, alphabet: bytes):
    for _ in range(24):
        b = bytearray(s)
        k = int(rng.integers(0, 4))
        at = int(rng.integers(0, len(b) + 1))
        if k == 0 and b:
            del b[min(at, len(b) - 1)]
        elif k == 1:
            b.insert(at, alphabet[int(rng.integers(0, len(alphabet)))])
        elif k == 2 and b:
            b[min(at, len(b) - 1)] = alphabet[int(rng.integers(0, len(alphabet)))]
        else:
            b = b[:at] + b[:at][::-1][:2] + b[at:]
        yield bytes(b)


@pytest.mark.parametrize("pat,alphabet,members", PATTERNS, ids=[str(i) for i in range(len(PATTERNS))])
def test_compile_agrees_with_re_fullmatch(built_lib, pat, alphabet, members):
    d = rt.Dfa.compile(pat)
    _, acc = d.table()
    oracle = re.compile(to_re(pat), re.S)
    rng = np.random.default_rng(len(pat))
    cases = [b""] + list(members)
    for m in members:
        assert oracle.fullmatch(m), (pat, m)                              # the oracle itself reads the members as members
        cases += list(mutations(rng, m, alphabet))
    for _ in range(400):
        cases.append(bytes(alphabet[int(k)] for k in rng.integers(0, len(alphabet), int(rng.integers(0, 13)))))
    seen = {True: 0, False: 0}
    for s in cases:
        want = oracle.fullmatch(s) is not None
        assert accepts(d, acc, s) == want, (pat, s, want)
        seen[want] += 1
    assert seen[True] >= len(members) and seen[False] >= 20, seen
    # trimmed: a prefix that cannot be completed is DEAD already, a prefix of a member is live
    for m in members:
        assert all(d.walk(d.start, m[:k]) != 0 for k in range(len(m) + 1))


def test_equivalent_spellings_have_one_table(built_lib):
    groups = [(rb"a{2}", rb"aa", rb"(a)(a)", rb"a{1}a{1,1}"), (rb"(a|b)", rb"[ab]", rb"[a-b]", rb"(b|a|a)", rb"\x61|\x62"),
              (rb"a*", rb"(a*)*", rb"(a|)*", rb"(a+)?", rb"a{0,}"), (rb"\d+", rb"[0-9][0-9]*", rb"\d\d*|\d", rb"[0-9]{1,}"),
              (rb"(ab|ac)", rb"a[bc]", rb"a(b|c)"), (rb".", rb"[^\n]"), ("é".encode(), rb"\xc3\xa9"), (rb"a?b", rb"(ab|b)", rb"a{0,1}b")]
    tables = []
    for g in groups:
        ts = [rt.Dfa.compile(p).table() for p in g]
        for (t, a), p in zip(ts[1:], g[1:]):
            assert t.tobytes() == ts[0][0].tobytes() and a.tobytes() == ts[0][1].tobytes(), (g[0], p)
        tables.append(ts[0][0].tobytes())
    assert len(set(tables)) == len(groups)                                # ... and different languages differ
    # the numbering itself: breadth-first from the start state, bytes ascending, start = 1, DEAD = 0
    d = rt.Dfa.compile(rb"(b|a)c")
    t, a = d.table()
    assert d.start == 1 and d.num_states == 4 and not t[0].any() and list(a) == [0, 0, 0, 1]
    assert t[1, ord("a")] == 2 and t[1, ord("b")] == 2 and t[2, ord("c")] == 3 and t.astype(bool).sum() == 3
    d = rt.Dfa.compile(rb"bx|ay")
    t, _ = d.table()
    assert t[1, ord("a")] == 2 and t[1, ord("b")] == 3                    # 'a' < 'b': its target is numbered first
    # from_table keeps what it is given: no trim, no renumbering
    tt = np.zeros((4, 256), np.uint16)
    tt[3, 65] = 2
    tt[2, 66] = 1                                                         # state 1 accepts nothing and leads nowhere: kept as it is
    f = rt.Dfa.from_table(tt, [0, 0, 1, 0], start=3)
    t2, a2 = f.table()
    assert f.start == 3 and f.num_states == 4 and (t2 == tt).all() and list(a2) == [0, 0, 1, 0]
    assert f.walk(3, b"A") == 2 and f.walk(3, b"AB") == 1 and f.walk(3, b"ABA") == 0 and f.walk(0, b"") == 0


# ---- the World vocabulary --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    raw = lzma.open(os.path.join(ROOT, "tests", "golden", "rwkv_vocab_v20230424.json.xz"), "rt", encoding="utf-8").read()
    vocab = {int(k): (v.encode("utf-8") if isinstance(v, str) else bytes(v)) for k, v in json.loads(raw).items()}
    table = [vocab.get(i) for i in range(max(vocab) + 1)]                 # id 0 is not in the vocabulary
    return table


def numpy_allow(trans, state, table, num_vocab):
    """every token walks its bytes at once: one gather per byte position"""
    n = len(table)
    lens = np.array([len(b) if b is not None else -1 for b in table])
    width = int(lens.max())
    grid = np.zeros((n, width), np.uint8)
    for i, b in enumerate(table):
        if b:
            grid[i, :len(b)] = np.frombuffer(b, np.uint8)
    q = np.full(n, state, np.int64)
    for k in range(width):
        go = lens > k
        q[go] = trans[q[go], grid[go, k]]
    allow = np.zeros(num_vocab, np.uint8)
    allow[:n] = (lens > 0) & (q != 0)
    allow[0] = 0
    return allow


def test_allow_on_the_world_vocabulary_equals_a_numpy_walk(built_lib, world):
    singles = {b[0] for b in world if b is not None and len(b) == 1}
    assert singles == set(range(256))                                     # what makes every trimmed automaton pass the liveness rule
    V = 65536
    n_checked = 0
    for pat, prefixes in ((rb'\{"name":"[^"\\]{1,12}","age":\d{1,3}\}', [b"", b'{"name":"', b'{"name":"Bo","age":', b'{"name":"Bo","age":41']),
                          (rb"(-?\d+(\.\d+)?|true|false|null|" + "中文".encode() + rb")( [a-z]+)*", [b"", b"-", b"tr", b"12.5 ab", "中".encode()])):
        d = rt.Dfa.compile(pat)
        trans, _ = d.table()
        d.check_live(world)
        d.check_live(world, halt=rt.DfaHalt.Accept)
        for pre in prefixes:
            q = d.walk(d.start, pre)
            assert q != 0
            got = d.allow(q, world, V)
            want = numpy_allow(trans, q, world, V)
            np.testing.assert_array_equal(got, want)
            assert 0 < int(got.sum()) < len(world) and not got[len(world):].any() and got[0] == 0
            fm = H.DfaFormatter(d, world, V, state=q)
            np.testing.assert_array_equal(fm.transform(), got)
            n_checked += 1
        # a few drawn tokens through the Formatter: allowed ones advance as the walk says, a forbidden one is rejected in place
        fm = H.DfaFormatter(d, world, V)
        ok = np.flatnonzero(fm.transform())
        tok = int(ok[len(ok) // 2])
        before = fm.state
        bad = int(np.flatnonzero(fm.transform() == 0)[5])
        assert fm.update(bad) is False and fm.state == before and fm.update(0) is False and fm.update(V - 1) is False and fm.state == before
        fm.update(tok)
        assert fm.state == d.walk(before, world[tok]) != 0
    assert n_checked >= 6
    # dead state: nothing is allowed; a table shorter than the vocabulary masks the rest
    d = rt.Dfa.compile(rb"a+")
    assert not d.allow(0, world, V).any()
    small = d.allow(1, [None, b"a", b"", b"aa", b"ab", None], 16)
    assert list(small) == [0, 1, 0, 1, 0, 0] + [0] * 10
    assert list(d.allow(1, [b"a", b"a"], 4)) == [0, 1, 0, 0]              # token 0 is never allowed, whatever its bytes


def test_halt_predicates_of_the_formatter(built_lib):
    d = rt.Dfa.compile(rb"ab?")
    tab = [None, b"a", b"b", b"ab"]
    f, a = H.DfaFormatter(d, tab, 4, halt=rt.DfaHalt.Final), H.DfaFormatter(d, tab, 4, halt=rt.DfaHalt.Accept)
    assert f.update(1) is False and a.update(1) is True                   # "a" accepts, but b may follow
    assert f.update(2) is True                                            # "ab": nothing leads on
    g = H.DfaFormatter(d, tab, 4)
    assert g.update(3) is True and g.update(1) is False                   # a rejected token behind the end does not halt again


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(rt.RwkvError) as e:
        fn()
    return e.value.code, str(e.value)


def test_every_refusal(built_lib, world):
    ok = np.zeros((3, 256), np.uint16)
    ok[1, 97] = 2
    acc = [0, 0, 1]
    assert rt.Dfa.from_table(ok, acc).num_states == 3
    bad = ok.copy(); bad[0, 5] = 1
    assert _code(lambda: rt.Dfa.from_table(bad, acc))[0] == -1            # state 0 is not dead
    assert _code(lambda: rt.Dfa.from_table(ok, [1, 0, 1]))[0] == -1        # ... or accepts
    bad = ok.copy(); bad[2, 0] = 3
    assert _code(lambda: rt.Dfa.from_table(bad, acc))[0] == -1            # a target past the table
    for start in (0, 3, -1):
        assert _code(lambda: rt.Dfa.from_table(ok, acc, start=start))[0] == -1
    assert _code(lambda: rt.Dfa.from_table(np.zeros((1, 256), np.uint16), [0]))[0] == -1
    big = np.zeros((rt.DFA_MAX_STATES + 1, 256), np.uint16)
    assert _code(lambda: rt.Dfa.from_table(big, np.zeros(rt.DFA_MAX_STATES + 1, np.uint8)))[0] == -3
    assert rt.Dfa.from_table(big[:-1], np.zeros(rt.DFA_MAX_STATES, np.uint8), start=rt.DFA_MAX_STATES - 1).num_states == rt.DFA_MAX_STATES
    # malformed patterns: RWKV_ERR_INVALID with the offset
    for pat, off in ((rb"ab(cd", 2), (rb"ab)", 2), (rb"a[bc", 1), (rb"*a", 0), (rb"ab\q", 2), (rb"a{3", 1), (rb"a{5,2}", 1), (rb"a{256}", 1), (rb"x[z-a]", 3),
                     (rb"ab\x4", 2), (b"a\xffb", 1), (b"[\xc3\xa9]", 1), (rb"a**", 2), (rb"a^", 1), (b"ab\\", 2), (rb"a{,3}", 1), (b"\xe4\xb8", 0)):
        code, msg = _code(lambda: rt.Dfa.compile(pat))
        assert code == -1 and msg.endswith(f"at offset {off}"), (pat, code, msg)
    # the empty language and too many states: RWKV_ERR_UNSUPPORTED
    for pat in (rb"[]", rb"a[]b", rb"(a|b)*a(a|b){12}", rb"(a{200}){200}", b"(" * 200 + b"a" + b")" * 200):
        assert _code(lambda: rt.Dfa.compile(pat))[0] == -3, pat
    assert rt.Dfa.compile(rb"a[]|b").num_states == 3                      # a dead branch is not an empty language
    assert rt.Dfa.compile(rb"(a|b)*a(a|b){10}").num_states == 2 ** 11 + 1
    assert rt.Dfa.compile(b"").num_states == 2                            # the empty pattern matches the empty output
    # walk / allow with a bad state
    d = rt.Dfa.compile(rb"ab")
    assert _code(lambda: d.walk(4, b"a"))[0] == -1 and _code(lambda: d.walk(-1, b"a"))[0] == -1
    assert _code(lambda: d.allow(9, [b"a"], 4))[0] == -1
    assert _code(lambda: d.allow(1, [b"a" * 257], 4))[0] == -3
    # LIVENESS: the World vocabulary carries every automaton the compiler makes; drop the one single-byte token a state needs and it is refused
    j = rt.Dfa.compile(rb'\{"k":\d+\}')
    j.check_live(world)
    without = list(world)
    without[next(i for i, b in enumerate(world) if b == b":")] = None
    assert any(b is not None and b.startswith(b'":') for b in without)    # multi-byte tokens over ':' remain: they do not count
    assert _code(lambda: j.check_live(without))[0] == -3
    j.check_live(without, state=j.walk(1, b'{"k":'))                      # behind the colon nothing needs it any more
    # an untrimmed table with a live dead end: FINAL cannot leave state 2 (not accepting, no way on)
    stuck = np.zeros((4, 256), np.uint16)
    stuck[1, 97] = 2
    stuck[1, 98] = 3
    s = rt.Dfa.from_table(stuck, [0, 0, 0, 1])
    assert _code(lambda: s.check_live(world))[0] == -3
    # HALT_ACCEPT rests nowhere behind an accepting state, FINAL does: ab* with no token "b" behind the a
    aplus = rt.Dfa.compile(rb"ab*")
    tab = [None, b"a", b"c"]
    aplus.check_live(tab, halt=rt.DfaHalt.Accept)
    assert _code(lambda: aplus.check_live(tab, halt=rt.DfaHalt.Final))[0] == -3
    assert _code(lambda: aplus.check_live(tab, state=0))[0] == -1 and _code(lambda: aplus.check_live(tab, halt=2))[0] == -1


# ---- the stand-alone programs ----------------------------------------------------------------------------------------------------------
def test_gen_dfa_header_in_the_kernels_order(tmp_path):
    exe = str(tmp_path / "gen_dfa_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "gen_dfa_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.endswith("gen_dfa_test: ok\n"), r.stdout[-800:] + r.stderr[-400:]


def test_fuzzed_patterns_and_tables_only_ever_get_a_status(tmp_path):
    """tests/cpp/fuzz_dfa.cpp + csrc/rwkv_dfa.cpp as ONE stand-alone program under AddressSanitizer and UBSan (host code, CPU only)."""
    exe = str(tmp_path / "fuzz_dfa")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",           # the runtimes inside the program: it stands alone, whatever else is loaded
                           os.path.join(ROOT, "tests", "cpp", "fuzz_dfa.cpp"), os.path.join(ROOT, "ai00_server_amd", "csrc", "rwkv_dfa.cpp"), "-o", exe])
    r = subprocess.run([exe, "1200", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "no crash" in r.stdout, r.stdout[-800:] + r.stderr[-3000:]

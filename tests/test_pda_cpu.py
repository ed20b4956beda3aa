"""CPU: the byte automata with a return-state stack of the resident-generation constraint (rwkv_pda_*, additive under ABI 9) — everything of
it that runs without a GPU, through ctypes on the library's host functions.

  - `Pda.json` against Python's `json` as the independent oracle, on a generated and mutated corpus: a document is valid when it decodes as
    strict UTF-8 and `json.loads` takes it with `parse_constant` raising (no NaN / Infinity).  Acceptance = the walk from the start ends in an
    accepting state with an empty stack.  Every prefix of an accepted document is live.
  - the two flags, the depth limit, the canonical numbering.
  - `rwkv_pda_allow` against `PdaWalker`, a numpy walk written here (an array stack per token, not the library's shift register), over the
    real World vocabulary.  tests/test_gpu_gen_pda.py uses the same walker for the per-token engine.
  - every refusal of the header, the liveness rule included.
  - tests/cpp/gen_pda_test.cpp (csrc/gen_pda.h in the kernels' order) and tests/cpp/fuzz_pda.cpp (stand-alone, built WITH rwkv_pda.cpp under
    -fsanitize=address,undefined; nothing is preloaded into Python)."""
import json
import lzma
import os
import random
import subprocess

import numpy as np
import pytest

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POP, SPAN = rt.PDA_POP, rt.PDA_TOKEN_SPAN
J = rt.PdaJson


class PdaWalker:
    """the numpy walk: every token of the table from one configuration at once, one gather per byte position; each token keeps the entries it
    pushed itself in a row of `own`, and reads the configuration's stack below the lowest depth it reached"""

    def __init__(self, tab, V):
        self.tab, self.V, n = tab, V, len(tab)
        self.lens = np.array([-1 if w is None else len(w) for w in tab])
        self.grid = np.zeros((n, max(1, int(self.lens.max()))), np.uint8)
        for i, w in enumerate(tab):
            if w:
                self.grid[i, :len(w)] = np.frombuffer(w, np.uint8)

    def walk(self, nxt, act, max_depth, q, stack):
        """(end state [V] with 0 = not allowed, depth [n], low [n], own [n, SPAN]) of every id from (q, stack)"""
        n = len(self.tab)
        base = np.array(list(stack) + [0], np.int64)
        s, d = np.full(n, q, np.int64), np.full(n, len(stack), np.int64)
        low, own = d.copy(), np.zeros((n, SPAN), np.int64)
        for k in range(self.grid.shape[1]):
            idx = np.flatnonzero((self.lens > k) & (s != 0))
            if not idx.size:
                break
            b = self.grid[idx, k]
            a, t = act[s[idx], b].astype(np.int64), nxt[s[idx], b].astype(np.int64)
            ns = np.where(a == 0, t, 0)
            pop, push = a == POP, (a != 0) & (a != POP)
            ip, cnt = idx[pop], (d - low)[idx[pop]]
            mine, under = cnt > 0, (cnt == 0) & (d[ip] > 0)
            got = np.zeros(ip.size, np.int64)
            got[mine] = own[ip[mine], cnt[mine] - 1]
            got[under] = base[d[ip[under]] - 1]
            low[ip[under]] -= 1
            d[ip[mine | under]] -= 1
            ns[pop] = got
            iq, cnt = idx[push], (d - low)[idx[push]]
            ok = (t[push] != 0) & (d[iq] < max_depth) & (cnt < SPAN)
            own[iq[ok], cnt[ok]] = a[push][ok]
            d[iq[ok]] += 1
            ns[push] = np.where(ok, t[push], 0)
            s[idx] = ns
        s[self.lens <= 0] = 0
        s[0] = 0                                                     # token 0 is never allowed
        end = np.zeros(self.V, np.int64)
        end[:n] = s
        return end, d, low, own

    def config_behind(self, walked, stack, tok):
        end, d, low, own = walked
        return int(end[tok]), [int(x) for x in stack[:int(low[tok])]] + [int(x) for x in own[tok, :int(d[tok] - low[tok])]]


def is_end(nxt, act, q):
    return not ((act[q] != POP) & (nxt[q] != 0)).any()


def ok_py(data: bytes) -> bool:
    try:
        s = data.decode("utf-8")
    except UnicodeDecodeError:
        return False

    def bad(x):
        raise ValueError(x)
    try:
        json.loads(s, parse_constant=bad)
        return True
    except (ValueError, RecursionError):
        return False


def accepts(p, acc, data: bytes) -> bool:
    q, st = p.walk(data)
    return bool(q and acc[q] and not st)


def corpus(n, seed=1):
    rng = random.Random(seed)

    def gen(d=0):
        r = rng.random()
        if d > 4 or r < 0.35:
            return rng.choice([1, -0.5, 1e10, "a\u00e9\U0001F600\"\\\n", True, None, 0, "", -12, False, 2.5e-3, "\u4e2d\x7f/"])
        if r < 0.65:
            return [gen(d + 1) for _ in range(rng.randint(0, 3))]
        return {rng.choice(["k", "", "\u4e2d", "a b"]): gen(d + 1) for _ in range(rng.randint(0, 3))}
    out = []
    for _ in range(n):
        doc = json.dumps(gen(), ensure_ascii=rng.random() < 0.5, indent=rng.choice([None, 1])).encode()
        if rng.random() < 0.6:
            doc = bytearray(doc)
            for _ in range(rng.randint(1, 3)):
                p, k = rng.randrange(len(doc) + 1), rng.random()
                if k < 0.4 and doc:
                    del doc[min(p, len(doc) - 1)]
                elif k < 0.8:
                    doc.insert(p, rng.choice(b' ,:[]{}"\\0-1.eEtn\x80\xc3\x01u'))
                elif doc:
                    doc[min(p, len(doc) - 1)] = rng.randrange(256)
            doc = bytes(doc)
        out.append(doc)
    return out


def test_json_agrees_with_pythons_json_on_a_generated_and_mutated_corpus(built_lib):
    p = rt.Pda.json()
    assert p.start == 1 and p.max_depth == rt.PDA_MAX_DEPTH and 100 < p.num_states < 200
    _, _, acc = p.table()
    docs = corpus(4000) + [b"", b" ", b"0", b"-0", b"01", b"1.", b".5", b"1e5", b"1E+", b"-", b"+1", b"tru", b"nul", b"null ", b"\tnull", b"[1,]", b"{,}",
                           b'{"a":1,}', b'{"a"}', b"{1:2}", b'"\\u12G4"', b'"\\ud800"', b'"\\x41"', b'"a\tb"', b'"\x1f"', b'"\x7f"', b"NaN", b"Infinity",
                           b"-Infinity", b'\xef\xbb\xbf"a"', b'"\xed\xa0\x80"', b'"\xc0\xaf"', b'"\xf4\x90\x80\x80"', b'"\xf4\x8f\xbf\xbf"', b"[] []", b"1 2",
                           b'"a" ', b"[\n]", b"{ }", b"1e-05", b"0e0", b"0.0E+00", b"00", b"-01", b"1.e1", b"\x0c1", b"\xa01"]
    seen = {True: 0, False: 0}
    live_checked = 0
    for doc in docs:
        want = ok_py(doc)
        assert accepts(p, acc, doc) == want, (doc, want)
        seen[want] += 1
        if want and live_checked < 300:
            live_checked += 1
            assert all(p.walk(doc[:k])[0] != 0 for k in range(len(doc) + 1)), doc       # every prefix of an accepted document is LIVE
    print("accepted", seen[True], "rejected", seen[False])
    assert seen[True] * 3 >= len(docs) and seen[False] * 3 >= len(docs), seen


def test_object_and_compact_do_what_they_say(built_lib):
    plain, obj, compact, both = (rt.Pda.json(f) for f in (0, J.Object, J.Compact, J.Object | J.Compact))
    accs = {id(p): p.table()[2] for p in (plain, obj, compact, both)}

    def ok(p, doc):
        return accepts(p, accs[id(p)], doc)
    for doc in (b"1", b'"s"', b"true", b"null", b" 12 "):
        assert ok(plain, doc) and not ok(obj, doc) and not ok(both, doc), doc
    for doc in (b"[1]", b'{"a":[true,{"b":null}]}', b"[]", b"{}"):
        assert all(ok(p, doc) for p in (plain, obj, compact, both)), doc
    for doc in (b" [1]", b"[1] ", b"[1, 2]", b'{"a": 1}', b'{ "a":1}', b"[\n]", b'{"a" :1}', b"1 "):
        assert ok(plain, doc) and not ok(compact, doc) and not ok(both, doc), doc
    assert ok(obj, b' {"a" : [ 1 , 2 ] } ') and ok(compact, b'{" a ":" "}') and ok(both, b'[" ,\\n "]') and ok(compact, b"-1.5e+3")
    # COMPACT is exactly "valid, and no whitespace outside its strings"; OBJECT exactly "valid, and the first byte behind whitespace is a bracket"
    for doc in corpus(1500, seed=2):
        valid = ok_py(doc)
        assert ok(compact, doc) == bool(valid and not any(c in b" \t\n\r" for c in strip_strings(doc))), doc
        assert ok(obj, doc) == bool(valid and doc.lstrip(b" \t\n\r")[:1] in (b"[", b"{")), doc
    # under OBJECT | COMPACT the state behind the closing bracket accepts and is END: HALT_FINAL halts there, and only there
    n, a, acc = both.table()
    q, st = both.walk(b'{"a":[1,2]}')
    assert acc[q] and not st and is_end(n, a, q)
    q, st = both.walk(b'{"a":[1,2]')
    assert q and st and not is_end(n, a, q)
    q, _ = plain.walk(b"[]")
    assert plain.table()[2][q] and not is_end(*plain.table()[:2], q)       # whitespace may follow: never FINAL, ACCEPT is the mode to use


def strip_strings(doc: bytes) -> bytes:
    """a valid document without its string literals"""
    out, i, inside = bytearray(), 0, False
    while i < len(doc):
        c = doc[i]
        if inside:
            if c == 0x5C:
                i += 1
            elif c == 0x22:
                inside = False
        elif c == 0x22:
            inside = True
        else:
            out.append(c)
        i += 1
    return bytes(out)


def test_the_depth_limit_and_the_canonical_numbering(built_lib):
    for md in (1, 3, 64):
        p = rt.Pda.json(0, md)
        acc = p.table()[2]
        for open_, close in ((b"[", b"]"), (b'{"k":', b"}")):
            assert accepts(p, acc, open_ * (md - 1) + b"[" + b"]" + close * (md - 1))
            q, st = p.walk(open_ * (md - 1) + b"[")
            assert q and len(st) == md
            assert p.walk(open_ * md + b"[")[0] == 0 and p.walk(open_ * md + b"{")[0] == 0       # max_depth + 1 is refused
            assert not accepts(p, acc, open_ * md + b"[]" + close * md)
    # one table per flags, whatever max_depth; different flags differ
    tables = []
    for f in (0, 1, 2, 3):
        a, b = rt.Pda.json(f, 2), rt.Pda.json(f, 64)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.table(), b.table())) and (a.max_depth, b.max_depth) == (2, 64)
        tables.append(a.table()[0].tobytes() + a.table()[1].tobytes())
    assert len(set(tables)) == 4
    # breadth-first from the start, bytes ascending: under COMPACT the first byte with an entry is `"` (0x22), whose target is state 2
    n, a, _ = rt.Pda.json(J.Compact).table()
    assert n[1, 0x22] == 2 and a[1, 0x22] == 0 and n[1, ord("-")] == 3 and not n[0].any() and not a[0].any()
    assert a[1, ord("[")] not in (0, POP) and a[1, ord("{")] == a[1, ord("[")]                  # both brackets return to the state behind the value


# ---- the World vocabulary --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    raw = lzma.open(os.path.join(ROOT, "tests", "golden", "rwkv_vocab_v20230424.json.xz"), "rt", encoding="utf-8").read()
    vocab = {int(k): (v.encode("utf-8") if isinstance(v, str) else bytes(v)) for k, v in json.loads(raw).items()}
    return [vocab.get(i) for i in range(max(vocab) + 1)]              # id 0 is not in the vocabulary


def test_allow_on_the_world_vocabulary_equals_a_numpy_walk(built_lib, world):
    V = 65536
    w = PdaWalker(world, V)
    n_checked = 0
    for flags, md, prefixes in ((0, 64, [b"", b"[", b'{"name":', b'{"a":[1,{"b":"x', b'[[[{"k":[12', b"[1.5e", b'["\\u00', b'["\xe4\xb8', b"[[]", b" {} "]),
                                (J.Object | J.Compact, 3, [b"", b"[[[", b'[{"a":[', b'{"a":{"b":{"c":1', b"[[[]]]"]),
                                (J.Compact, 10, [b"[" * 10, b"[" * 9, b"[" * 2, b'[[[["a"']), (0, 9, [b"[", b""])):
        p = rt.Pda.json(flags, md)
        nxt, act, _ = p.table()
        p.check_live(world)
        for pre in prefixes:
            q, st = p.walk(pre)
            assert q != 0, pre
            got = p.allow(q, st, world, V)
            walked = w.walk(nxt, act, md, q, st)
            np.testing.assert_array_equal(got, (walked[0] != 0).astype(np.uint8), err_msg=repr(pre))
            assert not got[len(world):].any() and got[0] == 0
            fm = H.PdaFormatter(p, world, V, state=q, stack=st)
            np.testing.assert_array_equal(fm.transform(), got)
            # what the numpy walk leaves behind a few allowed tokens is what the byte walk of the library leaves
            for tok in np.flatnonzero(got)[:: max(1, int(got.sum()) // 40)]:
                assert w.config_behind(walked, st, int(tok)) == p.walk(world[int(tok)], q, st), (pre, world[int(tok)])
            n_checked += 1
    assert n_checked >= 20
    # the span rule on real tokens: the vocabulary's longest run of `[` is allowed at depth 0 iff it owns at most SPAN entries
    p = rt.Pda.json(0, 64)
    got = p.allow(p.start, [], world, V)
    runs = [(i, len(b)) for i, b in enumerate(world) if b and set(b) == {ord("[")}]
    assert runs and all(bool(got[i]) == (k <= SPAN) for i, k in runs)
    # a drawn token through the Formatter: allowed ones commit as the walk says, a forbidden one is rejected in place
    fm = H.PdaFormatter(p, world, V)
    tok = next(i for i, b in enumerate(world) if b == b'{"')
    bad = next(i for i, b in enumerate(world) if b == b"}")
    assert fm.update(bad) is False and fm.update(0) is False and fm.update(V - 1) is False and (fm.state, fm.stack) == (p.start, [])
    assert fm.update(tok) is False and (fm.state, fm.stack) == p.walk(b'{"') and len(fm.stack) == 1
    both = rt.Pda.json(J.Object | J.Compact)
    f, a = H.PdaFormatter(both, world, V, halt=rt.PdaHalt.Final), H.PdaFormatter(both, world, V, halt=rt.PdaHalt.Accept)
    for fmt in (f, a):
        assert fmt.update(next(i for i, b in enumerate(world) if b == b"[]")) is True
    g = H.PdaFormatter(rt.Pda.json(), world, V, halt=rt.PdaHalt.Final)
    assert g.update(next(i for i, b in enumerate(world) if b == b"[]")) is False          # whitespace may follow
    # a dead configuration allows nothing; a table shorter than the vocabulary masks the rest; token 0 whatever its bytes
    assert not p.allow(0, [], world, V).any()
    assert list(p.allow(p.start, [], [b"1", b"1", b"", b"[1", b"]", None, b"[" * 8, b"[" * 9], 12)) == [0, 1, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(rt.RwkvError) as e:
        fn()
    return e.value.code, str(e.value)


def brackets(max_depth=3):
    """letters and balanced brackets: 1 TOP (accepts; `a` stays, `[` pushes 1 -> 2), 2 IN (`a` `,` stay, `[` pushes 2, `]` pops)"""
    n, a = np.zeros((3, 256), np.uint16), np.zeros((3, 256), np.uint16)
    n[1, ord("a")] = 1
    n[1, ord("[")], a[1, ord("[")] = 2, 1
    n[2, ord("a")] = n[2, ord(",")] = 2
    n[2, ord("[")], a[2, ord("[")] = 2, 2
    a[2, ord("]")] = POP
    return n, a, [0, 1, 0]


def test_every_refusal(built_lib, world):
    n, a, acc = brackets()
    p = rt.Pda.from_table(n, a, acc, max_depth=3)
    assert (p.num_states, p.start, p.max_depth) == (3, 1, 3) and all((x == y).all() for x, y in zip(p.table(), (n, a, np.array(acc))))
    assert p.walk(b"a[a[,]a]a") == (1, []) and p.walk(b"[[[") == (2, [1, 2, 2]) and p.walk(b"[[[[")[0] == 0 and p.walk(b"]")[0] == 0
    assert p.walk(b"],[", 2, [1, 2]) == (2, [1, 2]) and p.walk(b"],[", 2, [1])[0] == 0
    for plane in (0, 1):                                                   # state 0 is not dead, in either plane
        bn, ba = n.copy(), a.copy()
        (bn, ba)[plane][0, 5] = 1
        assert _code(lambda: rt.Pda.from_table(bn, ba, acc))[0] == -1
    assert _code(lambda: rt.Pda.from_table(n, a, [1, 1, 0]))[0] == -1       # ... or accepts
    bn = n.copy(); bn[2, 0] = 3
    assert _code(lambda: rt.Pda.from_table(bn, a, acc))[0] == -1            # a target past the table
    ba = a.copy(); ba[2, ord("[")] = 3
    assert _code(lambda: rt.Pda.from_table(n, ba, acc))[0] == -1            # an act that is no state, not 0 and not POP
    ba = a.copy(); ba[2, ord("[")] = POP - 1
    assert _code(lambda: rt.Pda.from_table(n, ba, acc))[0] == -1
    ba = a.copy(); ba[1, ord("x")] = 2
    assert _code(lambda: rt.Pda.from_table(n, ba, acc))[0] == -1            # a push with next == 0
    bn = n.copy(); bn[2, ord("]")] = 999
    assert rt.Pda.from_table(bn, a, acc).walk(b"[]") == (1, [])             # `next` of a pop is ignored
    for start in (0, 3, -1):
        assert _code(lambda: rt.Pda.from_table(n, a, acc, start=start))[0] == -1
    for md in (0, -1, rt.PDA_MAX_DEPTH + 1):
        assert _code(lambda: rt.Pda.from_table(n, a, acc, max_depth=md))[0] == -1
        assert _code(lambda: rt.Pda.json(0, md))[0] == -1
    assert _code(lambda: rt.Pda.json(4))[0] == -1                           # an unknown flag
    z = np.zeros((1, 256), np.uint16)
    assert _code(lambda: rt.Pda.from_table(z, z, [0]))[0] == -1
    big = np.zeros((rt.PDA_MAX_STATES + 1, 256), np.uint16)
    assert _code(lambda: rt.Pda.from_table(big, big, np.zeros(rt.PDA_MAX_STATES + 1, np.uint8)))[0] == -3
    assert rt.Pda.from_table(big[:-1], big[:-1], np.zeros(rt.PDA_MAX_STATES, np.uint8), start=rt.PDA_MAX_STATES - 1).num_states == rt.PDA_MAX_STATES
    # walk / allow / check_live from a bad configuration
    assert _code(lambda: p.walk(b"a", 3))[0] == -1 and _code(lambda: p.walk(b"a", -1))[0] == -1
    assert _code(lambda: p.walk(b"a", 2, [1, 2, 2, 2]))[0] == -1            # deeper than max_depth
    assert _code(lambda: p.walk(b"a", 2, [0]))[0] == -1 and _code(lambda: p.walk(b"a", 2, [3]))[0] == -1
    assert _code(lambda: p.allow(9, [], [b"a"], 4))[0] == -1 and _code(lambda: p.allow(2, [7], [b"a"], 4))[0] == -1
    assert _code(lambda: p.allow(1, [], [b"a" * 257], 4))[0] == -3
    tab = [None, b"a", b"[", b"]", b","]
    assert _code(lambda: p.check_live(tab, 0))[0] == -1 and _code(lambda: p.check_live(tab, 2, [5]))[0] == -1
    # LIVENESS.  The bracket language passes with `a`, and without it: IN keeps the plain `,`, and TOP, which is only ever entered with an
    # empty stack, may take its push for a way on.  TOP at depth 1 (a configuration the table never reaches itself) may not; IN without
    # `a` and `,` has only a push and a pop left.
    p.check_live(tab)
    p.check_live(tab, 2, [1, 2, 2])
    no_a = [None, b"[", b"]", b","]
    p.check_live(no_a)
    p.check_live(no_a, 2, [1])
    p.check_live(tab, 1, [1])
    assert _code(lambda: p.check_live(no_a, 1, [1]))[0] == -3
    assert _code(lambda: p.check_live([None, b"[", b"]"]))[0] == -3
    # a pop-only state: 2 may only close.  At depth max_depth it could not push anyway; with an empty stack the pop is dead: refused
    n2, a2 = n.copy(), a.copy()
    n2[2], a2[2] = 0, 0
    a2[2, ord("]")] = POP
    assert _code(lambda: rt.Pda.from_table(n2, a2, acc).check_live(tab))[0] == -3
    # push-only above the floor: 2 may only open.  Dead at max_depth: refused, although a push is a way on for TOP
    n3, a3 = n.copy(), a.copy()
    n3[2], a3[2] = 0, 0
    n3[2, ord("[")], a3[2, ord("[")] = 2, 2
    assert _code(lambda: rt.Pda.from_table(n3, a3, acc).check_live(tab))[0] == -3
    # a token table lacking a needed single byte: JSON without the token `:` (multi-byte tokens over ':' remain: they do not count)
    j = rt.Pda.json(J.Object | J.Compact)
    j.check_live(world)
    without = list(world)
    without[next(i for i, b in enumerate(world) if b == b":")] = None
    assert any(b is not None and b.startswith(b'":') for b in without)
    assert _code(lambda: j.check_live(without))[0] == -3
    # the configuration's own state is never exempt: behind the closing bracket nothing leads on, a slot set there would mask its whole row
    q, st = j.walk(b"[]")
    assert _code(lambda: j.check_live(world, q, st))[0] == -3
    rt.Pda.json().check_live(world, *rt.Pda.json().walk(b"[]"))             # with whitespace allowed there is a way on


# ---- the stand-alone programs ----------------------------------------------------------------------------------------------------------
def test_gen_pda_header_in_the_kernels_order(tmp_path):
    exe = str(tmp_path / "gen_pda_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "gen_pda_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.endswith("gen_pda_test: ok\n"), r.stdout[-800:] + r.stderr[-400:]


def test_fuzzed_tables_and_configurations_only_ever_get_a_status(tmp_path):
    """tests/cpp/fuzz_pda.cpp + csrc/rwkv_pda.cpp as ONE stand-alone program under AddressSanitizer and UBSan (host code, CPU only)."""
    exe = str(tmp_path / "fuzz_pda")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",           # the runtimes inside the program: it stands alone, whatever else is loaded
                           os.path.join(ROOT, "tests", "cpp", "fuzz_pda.cpp"), os.path.join(ROOT, "ai00_server_amd", "csrc", "rwkv_pda.cpp"), "-o", exe])
    r = subprocess.run([exe, "1500", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "no crash" in r.stdout, r.stdout[-800:] + r.stderr[-3000:]

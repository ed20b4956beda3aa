"""CPU: the visit list of tests/gen_churn.py really takes `gen_graphs` past its capacity.  The keys the GPU test's visits have — slot-mask
words and flag word, as tests/gen_churn.py computes them from the seats, sampler kinds and features of each visit — are written to a file and
put through the real rwkv::GraphCache (ai00_server_amd/csrc/graph_cache.h, compiled with g++ like tests/test_graph_cache_cpp.py) in the order
gen_decode_steps uses it: find, then should_capture, then insert.  These are conditions on the SCHEDULE; the GPU test shows that the tokens
are right under it."""
import os
import subprocess

import pytest

from tests import gen_churn as CH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    d = tmp_path_factory.mktemp("gen_churn")
    exe, path = str(d / "graph_cache_replay"), str(d / "keys.txt")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "graph_cache_replay.cpp"), "-o", exe])
    with open(path, "w") as f:
        for k in CH.keys():
            f.write(" ".join(f"{w:x}" for w in k) + "\n")
    out = subprocess.run([exe, str(CH.CAPACITY), path], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    visits = [(int(v), what, int(ev), int(n)) for v, what, ev, n in (ln.split() for ln in lines[:-1])]
    assert [v for v, _, _, _ in visits] == list(range(len(CH.VISITS)))
    return visits, int(lines[-1].split()[1])


def test_the_keys_are_what_the_visit_list_says():
    keys = CH.keys()
    assert len(CH.SETS) == 70 and len(set(CH.SETS)) == 70 and len(CH.VISITS) == 76 and len(set(keys[:70])) == 70
    assert all(len(k) == 3 for k in keys)                              # two mask words for 72 slots, one flag word
    assert keys[70:73] == keys[:3] and keys[73:] == keys[67:70]        # the revisits carry the flags of the first visit: the same keys
    assert any(k[0] == 0 for k in keys) and all(k[0] | k[1] for k in keys)   # a row set that lives in the second mask word alone (seats 64, 65, 71)
    assert sum(1 for k in keys if k[1]) >= 60                          # ... and most reach into it
    assert {k[2] & 3 for k in keys} == {1, 3}                          # nucleus / typical rows alone, or with Mirostat rows (seats 31 and 65) beside them
    for v, k in enumerate(keys):
        want = {"watch": CH.WATCH, "topn": CH.TOPN, "stops": CH.STOPS, None: 0}[CH.band(v)]
        assert k[2] >> 32 == want >> 32, v
        assert sum(bin(w).count("1") for w in k[:2]) == len(CH.VISITS[v])
    assert [sum(CH.band(v) == b for v in range(76)) for b in ("watch", "topn", "stops")] == [10, 10, 10]


def test_the_schedule_evicts_captures_again_and_replays(trace):
    visits, deleted = trace
    evicted = [ev for _, _, ev, _ in visits if ev >= 0]
    print("evicted", evicted, "outcomes", "".join(w for _, w, _, _ in visits))
    assert len(evicted) >= 6
    again = [v for v, what, _, _ in visits if what == "c" and any(CH.key(e) == CH.key(v) for e in evicted if e < v)]
    assert len(again) >= 3                                             # inserts of a key that was evicted earlier
    late = [v for v, what, _, n in visits if what == "r" and n > CH.CAPACITY]
    assert len(late) >= 3                                              # finds that hit after more than 64 inserts
    # the whole trace, as the module docstring of tests/gen_churn.py tells it
    assert "".join(w for _, w, _, _ in visits) == "d" * 70 + "c" * 3 + "r" * 3
    assert evicted == list(range(9))                                   # the least recently used: visits 0 .. 5 by the first 70, 6 .. 8 by the three that return
    assert visits[-1][3] == 73 and deleted == 73

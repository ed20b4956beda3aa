"""CPU: the key of a captured decode step as the engine forms it (rwkv::gen_step_key, ai00_server_amd/csrc/gen_host.h, which gen_decode_steps
calls) against the Python model of it in tests/gen_churn.py, which the replay test and the GPU churn test rest on.  The header is compiled
with g++ alone — it is host-only, like graph_cache.h — into tests/cpp/gen_key_dump.cpp; the driver gets the seats, sampler kinds and band of
each of the 76 visits (never the model's key) and prints the words."""
import os
import subprocess

import pytest

from tests import gen_churn as CH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEED = {"nucleus": "nt", "typical": "nt", "mirostat": "miro"}           # the header's name for the sampler kernel a kind needs


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gen_key") / "gen_key_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "gen_key_dump.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        keys = [tuple(int(w, 16) for w in ln.split()) for ln in out.stdout.splitlines()]
        assert len(keys) == len(lines)
        return keys
    return run


def test_every_visit_of_the_churn_list_has_the_key_the_model_says(dump):
    lines = []
    for v, row_set in enumerate(CH.VISITS):
        needs = "+".join(sorted({NEED[CH.KINDS[i % 3]] for i in row_set}))
        slots = sorted(CH.SEATS[i] for i in row_set)
        lines.append(f"{CH.MAX_BATCH} {needs} {CH.band(v) or '0'} " + " ".join(str(b) for b in slots))
    assert len(lines) == 76
    keys = dump(lines)
    for v, k in enumerate(keys):
        assert k == CH.key(v), (v, lines[v])


def test_hand_written_keys(dump):
    k = dump(["64 nt 0 63",
              "65 nt 0 64",
              "8 wide stops+dfa+topn+pda+watch+capture 0",
              "8 nt 0 0 3",
              "8 4 3f00000000 0",
              "8 nt stops 0", "8 nt dfa 0", "8 nt topn 0", "8 nt pda 0", "8 nt watch 0", "8 nt capture 0",
              "8 miro 0 0", "72 3 1400000000 1 70"])
    assert k[0] == (0x8000000000000000, 1)                            # one mask word: the last slot of it
    assert k[1] == (0, 1, 1)                                          # two: the first slot of the second
    assert k[2] == (1, 0x3F00000004)                                  # every feature bit (32 .. 37) beside NEEDS_WIDE
    assert k[3] == (0b1001, 1)                                        # an empty feature word: the sampler bits alone
    assert k[4] == k[2]                                               # the same flag word, given as numbers
    assert [w for _, w in k[5:11]] == [(1 << bit) | 1 for bit in (32, 33, 34, 35, 36, 37)]   # each feature bit on its own, in the key's order
    assert k[11] == (1, 2)                                            # NEEDS_MIRO alone
    assert k[12] == (2, 1 << 6, 0x1400000003)                         # numbers again: two mask words, top-n and watch beside both sampler bits

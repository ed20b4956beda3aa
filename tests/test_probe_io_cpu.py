"""CPU: the container parser of the kernel probes (tests/cpp/probe_case.h) against the Python side of the same format (tests/probe_io.py).

tests/cpp/probe_case_test.cpp includes probe_case.h alone and is built as ONE stand-alone program under AddressSanitizer and UBSan (host code,
CPU only; nothing is preloaded and nothing of it is loaded into Python).  It must read what the real tables write exactly as read_cases does,
end with status 2 and the "ends early" message on a file cut anywhere, and end with status 2 on every bad header."""
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import gen_cases as G, mix_cases as M, probe_io as P, row_cases as R, sample_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# program, magic, K_COUNT, the parameter-count limit, R_COUNT, the small element size: the ProbeSpec of each probe's main()
SPEC = {"row": ("row_probe", 0x42525052, len(R.KIND_NAME), 16, len(R.ROLE), 2), "mix": ("mix_probe", 0x4252504D, len(M.KIND_NAME), 32, len(M.ROLE), 2),
        "sample": ("sample_probe", 0x42525053, len(S.KIND_NAME), 8, len(S.ROLE), 1), "gen": ("gen_probe", G.MAGIC, len(G.KIND_NAME), len(G.PARAMS), len(G.ROLE), 1)}
SMALLEST = {"row": (R, "state_pack"), "mix": (M, "commit"), "sample": (S, "routing"), "gen": (G, "step")}
# the smallest group of each family that holds buffers with an image and buffers the probe fills with the pattern (gen: `tokens` and `publish` are
# smaller, but every buffer of theirs carries an image)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("probe_case") / "probe_case_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",           # the runtimes inside the program: it stands alone, whatever else is loaded
                           os.path.join(ROOT, "tests", "cpp", "probe_case_test.cpp"), "-o", out])
    return out


def parse(exe, path, family):
    spec = SPEC[family]
    return subprocess.run([exe, str(path), spec[0], hex(spec[1])] + [str(v) for v in spec[2:]], capture_output=True, text=True, timeout=120)


def clean(r):
    return "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def write_group(family, path):
    mod, group = SMALLEST[family]
    cases = [c for c in mod.all_cases() if c.group == group]
    mod.write_cases(path, cases, [mod.make(c) for c in cases])
    return cases


@pytest.mark.parametrize("family", list(SPEC))
def test_the_parser_reads_what_read_cases_reads(exe, tmp_path, family):
    path = str(tmp_path / "cases.bin")
    cases = write_group(family, path)
    r = parse(exe, path, family)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = [json.loads(l) for l in r.stdout.splitlines()]
    want = []
    for name, kind, par, bufs in P.read_cases(path, SPEC[family][1]):
        rows = []
        for role, esize, flags, nbytes, off, img in bufs:
            img = np.full(nbytes // esize, P.SENT[esize], P.UINT[esize]) if flags & 2 else img      # the pattern this side expects
            rows.append([role, esize, flags, nbytes, off, zlib.crc32(img.tobytes())])
        want.append({"name": name, "kind": kind, "params": list(par), "bufs": rows})
    assert [w["name"] for w in want] == [c.name for c in cases] and got == want
    assert any(b[2] & 2 for w in want for b in w["bufs"]) and any(not b[2] & 2 for w in want for b in w["bufs"])


def header_boundaries(raw, ncases):
    """Offsets at which a header of the first `ncases` cases begins or ends: the file's, each case's fields, each buffer's header and image."""
    cuts, pos = [0, 4, 8], 8
    for _ in range(ncases):
        nl, = struct.unpack_from("<i", raw, pos)
        cuts += [pos + 4, pos + 4 + nl, pos + 12 + nl]
        pos += 12 + nl
        npar, = struct.unpack_from("<i", raw, pos - 4)
        cuts += [pos + 8 * npar, pos + 8 * npar + 4]
        pos += 8 * npar + 4
        nb, = struct.unpack_from("<i", raw, pos - 4)
        for _ in range(nb):
            _, _, flags, nbytes, _ = struct.unpack_from("<iiiqq", raw, pos)
            pos += 28
            cuts.append(pos)
            if not flags & 2:
                pos += nbytes
                cuts.append(pos)
    return sorted(set(cuts))


def test_a_file_cut_anywhere_ends_with_status_2(exe, tmp_path):
    path = str(tmp_path / "cases.bin")
    write_group("sample", path)
    raw = open(path, "rb").read()
    cuts = [c for c in header_boundaries(raw, 2) if c < len(raw)]
    assert 20 <= len(cuts) < 64
    rest = [int(x) for x in np.linspace(0, len(raw), 64 - len(cuts) + 2)[1:-1]]
    cuts = sorted(set(cuts + rest))
    assert len(cuts) == 64 and cuts[0] == 0 and cuts[-1] < len(raw)
    cut = str(tmp_path / "cut.bin")
    for n in cuts:
        with open(cut, "wb") as f:
            f.write(raw[:n])
        r = parse(exe, cut, "sample")
        assert r.returncode == 2 and r.stderr == "sample_probe: case file ends early\n" and clean(r), (n, r.returncode, r.stderr[-2000:])


def one_case(magic=0x42525053, ncases=1, name_len=1, kind=0, nparam=2, nbuf=1, esize=4, nbytes=16):
    """A case file of one case with one pattern-filled buffer, any header field replaced.  Counts beyond what follows are never reached: the
    parser refuses them first."""
    return (struct.pack("<iii", magic, ncases, name_len) + b"x" + struct.pack("<ii2qi", kind, nparam, 3, 16, nbuf)
            + struct.pack("<iiiqq", 0, esize, 2, nbytes, 0))


BAD = {"magic": dict(magic=0x42525052), "ncases -1": dict(ncases=-1), "ncases 4097": dict(ncases=4097), "name length 257": dict(name_len=257),
       "kind past the table": dict(kind=6), "one parameter too many": dict(nparam=9), "one buffer too many": dict(nbuf=15), "nbytes 0": dict(nbytes=0),
       "nbytes 2^31": dict(nbytes=1 << 31), "esize 3": dict(esize=3, nbytes=12), "nbytes no multiple of esize": dict(nbytes=18)}


def test_every_bad_header_ends_with_status_2(exe, tmp_path):
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(one_case())
    r = parse(exe, path, "sample")
    assert r.returncode == 0 and json.loads(r.stdout) == {"name": "x", "kind": 0, "params": [3, 16], "bufs": [[0, 4, 2, 16, 0, zlib.crc32(struct.pack("<4I", *[P.SENT32] * 4))]]}
    assert SPEC["sample"][3] == 8 and SPEC["sample"][4] == 14                       # what "one too many" above is one above
    for what, change in BAD.items():
        with open(path, "wb") as f:
            f.write(one_case(**change))
        r = parse(exe, path, "sample")
        assert r.returncode == 2 and r.stderr.startswith("sample_probe: bad ") and r.stdout == "" and clean(r), (what, r.returncode, r.stderr[-2000:])

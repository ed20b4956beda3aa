"""The case file and the result file of the role-buffer probes (tests/cpp/probe_case.h reads and writes the same format; DESIGN.md "Probe
container" states it), and the buffers the case tables are made of.  tests/row_cases.py, mix_cases.py and sample_cases.py bind their magic,
parameter order and role table to these.  A plain module, no fixtures."""
import struct
from dataclasses import dataclass

import numpy as np

GUARD = 256                                                        # elements on BOTH sides of every buffer
SENT32, SENT16, SENT8 = 0x7FC0DEAD, 0x7EAD, 0xAD
SENT = {4: SENT32, 2: SENT16, 1: SENT8}                            # the pattern of an element size
UINT = {4: np.uint32, 2: np.uint16, 1: np.uint8}


@dataclass
class Buf:
    role: str
    esize: int
    flags: int                                                     # 1: copied back, 2: the probe fills the pattern
    n: int                                                         # elements between the guard bands (spare rows included)
    off: int = 0                                                   # elements from the first guard band's end to the launcher's pointer
    image: np.ndarray = None                                       # bits, guard bands included (None with flags & 2)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize]).reshape(-1)


def b_in(role, a, back=False, spare=0):
    """`a` between guard bands; with spare > 0 one spare row / entry of `spare` pattern elements on both sides, the pointer behind the first."""
    b = bits(a)
    s = SENT[b.dtype.itemsize]
    g, sp = np.full(GUARD, s, b.dtype), np.full(spare, s, b.dtype)
    return Buf(role, b.dtype.itemsize, 1 if back else 0, b.size + 2 * spare, spare, np.concatenate([g, sp, b, sp, g]))


def b_out(role, n, esize=4, spare=0):
    return Buf(role, esize, 3, int(n) + 2 * spare, spare)


def own(res, b):
    """The elements behind the launcher's pointer, spare rows and guard bands cut off."""
    a = res[b.role]
    return a[GUARD + b.off: a.size - GUARD - b.off]


def write_cases(path, magic, cases, datas, params_of, role_index):
    """`params_of(case)`: the names of the case's parameters in the probe's order; `role_index`: the probe's Role enum by name."""
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", magic, len(cases)))
        for c, d in zip(cases, datas):
            nm = c.name.encode()
            vals = [int(c.p[k]) for k in params_of(c)]
            f.write(struct.pack("<i", len(nm)) + nm + struct.pack("<ii", c.kind, len(vals)) + struct.pack(f"<{len(vals)}q", *vals))
            f.write(struct.pack("<i", len(d["bufs"])))
            for b in d["bufs"]:
                f.write(struct.pack("<iiiqq", role_index[b.role], b.esize, b.flags, (b.n + 2 * GUARD) * b.esize, (GUARD + b.off) * b.esize))
                if not b.flags & 2:
                    assert b.image.size == b.n + 2 * GUARD and b.image.dtype.itemsize == b.esize
                    f.write(b.image.tobytes())


def read_cases(path, magic):
    """The case file back as (name, kind, params, [(role, esize, flags, nbytes, off, image or None)]): the round trip of write_cases."""
    out = []
    with open(path, "rb") as f:
        got, n = struct.unpack("<ii", f.read(8))
        assert got == magic
        for _ in range(n):
            nl, = struct.unpack("<i", f.read(4))
            name = f.read(nl).decode()
            kind, npar = struct.unpack("<ii", f.read(8))
            par = struct.unpack(f"<{npar}q", f.read(8 * npar))
            nb, = struct.unpack("<i", f.read(4))
            bufs = []
            for _ in range(nb):
                role, esize, flags, nbytes, off = struct.unpack("<iiiqq", f.read(28))
                img = None if flags & 2 else np.frombuffer(f.read(nbytes), UINT[esize])
                bufs.append((role, esize, flags, nbytes, off, img))
            out.append((name, kind, par, bufs))
        assert f.read(1) == b""
    return out


def read_results(path, cases, datas):
    out = []
    with open(path, "rb") as f:
        for c, d in zip(cases, datas):
            res = {}
            for b in d["bufs"]:
                if b.flags & 1:
                    nb = (b.n + 2 * GUARD) * b.esize
                    raw = f.read(nb)
                    assert len(raw) == nb, f"{c.name}: the result file ends inside {b.role}"
                    res[b.role] = np.frombuffer(raw, UINT[b.esize])
            out.append(res)
        assert f.read(1) == b"", "the result file is longer than the table"
    return out


def untouched(d):
    """What the probe returns when no kernel writes anything: every copied-back buffer as it went in (the CPU tests start from this)."""
    res = {}
    for b in d["bufs"]:
        if b.flags & 1:
            res[b.role] = np.full(b.n + 2 * GUARD, SENT[b.esize], UINT[b.esize]) if b.flags & 2 else b.image.copy()
    return res

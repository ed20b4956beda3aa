"""CPU: the host-only parts of device-resident sampled generation (ABI 8, include/rwkv_abi.h `rwkv_gen_*`): the counter-based
uniform draw, argument checking that never aborts, the hand-over of a host sampler's state (`gen_params_for`,
include/rwkv_sampler.hpp), and the layout of `rwkv_gen_params` on the three sides that spell it (C header, ctypes, Rust sys crate).
No compute call is made: the library loads without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from ai00_server_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def uniform_np(seed, stream, step):
    """The formula of include/rwkv_abi.h restated on numpy uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        seed, stream, step = (np.asarray(x, dtype=np.uint64) for x in (seed, stream, step))
        z = seed + np.uint64(0x9E3779B97F4A7C15) * (((stream << np.uint64(32)) | step) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def test_gen_uniform_is_the_documented_counter_function(built_lib):
    rng = np.random.default_rng(8)
    n = 10_000
    seeds = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    streams = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    steps = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    seeds[:4] = [0, 2 ** 64 - 1, 1, 0x9E3779B97F4A7C15]                    # the corners: wrap-around of every term
    streams[:4] = [0, 2 ** 32 - 1, 0, 2 ** 32 - 1]
    steps[:4] = [0, 2 ** 32 - 1, 2 ** 32 - 1, 0]
    got = np.array([rt.gen_uniform(int(a), int(b), int(c)) for a, b, c in zip(seeds, streams, steps)], np.float32)
    want = uniform_np(seeds, streams, steps)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got.min() >= 0.0 and got.max() < 1.0
    # consecutive steps of one stream, through the batch form; three sigma of the mean of 2^16 uniforms is 0.0034
    run = rt.gen_uniform(1234567, 3, 0, 1 << 16)
    np.testing.assert_array_equal(run.view(np.uint32), uniform_np(np.full(1 << 16, 1234567), np.full(1 << 16, 3), np.arange(1 << 16)).view(np.uint32))
    assert run.min() >= 0.0 and run.max() < 1.0
    assert abs(float(run.mean(dtype=np.float64)) - 0.5) < 0.01
    assert rt.gen_uniform(5, 1, 7) == float(rt.gen_uniform(5, 1, 0, 8)[7])      # `first_step + i`
    assert rt.lib().rwkv_gen_uniform(1, 2, 3, 4, None) == -1                    # RWKV_ERR_INVALID


def test_gen_calls_reject_null_arguments_without_aborting(built_lib):
    l = rt.lib()
    p = rt._GenParamsC()
    toks = (C.c_uint32 * 4)()
    for call, args in [(l.rwkv_gen_arm, (None, 0, C.byref(p))), (l.rwkv_gen_disarm, (None, 0)),
                       (l.rwkv_gen_run, (None, 1, toks, None, None, None))]:
        assert call(*args) == -1                                              # RWKV_ERR_INVALID
        assert l.rwkv_last_error() in (b"null engine", b"bad arguments"), l.rwkv_last_error()
    assert l.rwkv_gen_arm(None, 0, None) == -1 and l.rwkv_last_error() == b"null engine"
    assert l.rwkv_abi_version() >= 8


PROBE = r'''
#include <cstdio>
#include <cstring>
#include "rwkv_sampler.hpp"
static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
int main() {
    const std::vector<uint32_t> prompt = {5, 9, 5, 300, 9, 5, 77, 1000, 5};
    rwkv::NucleusSampler n;
    n.presence_penalty = 0.f;                          // entries exist with value frequency * decay^i only
    n.init(prompt);
    const rwkv::SamplerAdjust adj = n.adjustments();   // no bias: exactly -penalty
    rwkv::GenArrays keep;
    const rwkv_gen_params g = n.gen_params_for(42, 17, 99, 3, keep, {11, 12});
    std::printf("adj"); for (size_t i = 0; i < adj.tokens.size(); ++i) std::printf(" %u:%08x", adj.tokens[i], bits(adj.values[i])); std::printf("\n");
    std::printf("pen"); for (size_t i = 0; i < g.n_penalty; ++i) std::printf(" %u:%08x", g.penalty_tokens[i], bits(g.penalty_values[i])); std::printf("\n");
    std::printf("nuc %u %d %d %08x %d %08x %08x %08x %08x %zu %zu %llu %u %d\n", g.first_token, g.max_tokens, g.kind, bits(g.top_p), g.top_k, bits(g.temperature),
                bits(g.presence_penalty), bits(g.frequency_penalty), bits(g.penalty_decay), g.n_bias, g.n_stop, (unsigned long long)g.seed, g.stream, g.allow == nullptr);
    rwkv::TypicalSampler t;
    t.bias[7] = 1.5f;
    t.init(prompt);
    const rwkv_gen_params gt = t.gen_params_for(1, 2, 3, 4, keep);
    std::printf("typ %d %08x %08x %zu %zu %u:%08x\n", gt.kind, bits(gt.top_p), bits(gt.tau), gt.n_penalty, gt.n_bias, gt.bias_tokens[0], bits(gt.bias_values[0]));
    rwkv::MirostatSampler m(3.0f, 0.1f);
    m.update(4.25f);
    const rwkv_gen_params gm = m.gen_params_for(1, 2, 3, 4, keep);
    std::printf("mir %d %08x %08x %08x %08x %zu\n", gm.kind, bits(gm.tau), bits(m.max_surprise), bits(gm.miro_target), bits(gm.miro_rate), gm.n_penalty);
    return 0;
}
'''


def test_gen_params_for_hands_over_the_map_the_host_would_have_had(tmp_path):
    """`NucleusSampler::init(prompt)` followed by `gen_params_for` yields the penalty list of `adjustments()` with the sign flipped
    (the device negates it like `transform`, nucleus.rs:61-67); the Python mirror agrees bit for bit."""
    from ai00_server_amd import harness as H
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = {ln.split()[0]: ln.split()[1:] for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    adj = [(int(a.split(":")[0]), int(a.split(":")[1], 16)) for a in lines["adj"]]
    pen = [(int(a.split(":")[0]), int(a.split(":")[1], 16)) for a in lines["pen"]]
    assert len(pen) == 5 and [t for t, _ in pen] == [t for t, _ in adj]
    assert all(p ^ 0x80000000 == a for (_, p), (_, a) in zip(pen, adj))        # sign bit flipped, nothing else
    f32 = lambda x: int(np.float32(x).view(np.uint32))
    assert lines["nuc"] == ["42", "17", "0", f"{f32(0.5):08x}", "128", f"{f32(1.0):08x}", f"{f32(0.0):08x}", f"{f32(0.3):08x}",
                            f"{f32(0.99654026):08x}", "0", "2", "99", "3", "1"]
    assert lines["typ"] == ["1", f"{f32(0.0):08x}", f"{f32(0.5):08x}", "5", "1", f"7:{f32(1.5):08x}"]
    assert lines["mir"][0] == "2" and lines["mir"][1] == lines["mir"][2] and lines["mir"][3:] == [f"{f32(3.0):08x}", f"{f32(0.1):08x}", "0"]
    # the Python mirror holds the same map (same f32 operations in the same order)
    h = H.NucleusSampler(presence_penalty=0.0)
    h.init([5, 9, 5, 300, 9, 5, 77, 1000, 5])
    assert sorted((t, int(np.float32(v).view(np.uint32))) for t, v in h.penalties.items()) == pen
    m = H.MirostatSampler(3.0, 0.1)
    m.update(4.25)
    assert f"{int(np.float32(m.max_surprise).view(np.uint32)):08x}" == lines["mir"][1]


def test_gen_params_layout_agrees_between_header_ctypes_and_the_sys_crate(tmp_path):
    """`rwkv_gen_params` by the rules tests/test_ffi_layout.py applies to the other structs: field names and order, offsets, sizes."""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rwkv_abi.h")).read(), flags=re.S)
    body = re.search(r"struct rwkv_gen_params\s*\{([^}]*)\}\s*;", hdr, re.S).group(1)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in rt._GenParamsC._fields_]
    rs = open(os.path.join(ROOT, "integration", "rwkv-hip-sys", "src", "lib.rs")).read()
    rbody = re.search(r"pub struct rwkv_gen_params\s*\{([^}]*)\}", rs, re.S).group(1)
    sizes = {"u32": 4, "i32": 4, "c_float": 4, "usize": 8, "u64": 8}
    rust, off = [], 0
    for f in re.finditer(r"pub\s+(\w+)\s*:\s*([^,}]+)", rbody):
        size = 8 if f.group(2).strip().startswith("*") else sizes[f.group(2).strip()]
        off = (off + size - 1) // size * size                                 # every field's alignment is its size here
        rust.append((f.group(1), off, size))
        off += size
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rwkv_abi.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(rwkv_gen_params));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof(rwkv_gen_params, {n}), sizeof(((rwkv_gen_params *)0)->{n}));' for n in names]
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.splitlines()
    c = [(ln.split()[0], int(ln.split()[1]), int(ln.split()[2])) for ln in out[1:]]
    assert rust == c
    assert [(n, getattr(rt._GenParamsC, n).offset, getattr(rt._GenParamsC, n).size) for n in names] == c
    assert int(out[0]) == C.sizeof(rt._GenParamsC) == (off + 7) // 8 * 8

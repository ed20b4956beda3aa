"""CPU: the host-only parts of wide on-device sampling (any top_k, exact Mirostat): `gen_params_for` (include/rwkv_sampler.hpp) opts a
sampler with top_k > 256 into the wide kernel through RWKV_GEN_WIDE_TOP_K in `rwkv_gen_params.reserved`, and the header, the Rust
sys crate and the Python binding spell that constant alike.  No compute call is made."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r'''
#include <cstdio>
#include "rwkv_sampler.hpp"
int main() {
    rwkv::GenArrays keep;
    const int ks[] = {0, 1, 128, 256, 257, 1000, 65536};
    for (int k : ks) {
        rwkv::NucleusSampler n;
        n.top_k = k;
        rwkv::TypicalSampler t;
        t.top_k = k;
        const rwkv_gen_params gn = n.gen_params_for(1, 2, 3, 4, keep), gt = t.gen_params_for(1, 2, 3, 4, keep),
                              gp = n.gen_params_for_prompt(2, 3, 4, keep);
        std::printf("%d %u %u %u %d %d\n", k, gn.reserved, gt.reserved, gp.reserved, gn.top_k, gt.top_k);
    }
    rwkv::MirostatSampler m(5.0f, 0.1f);                 // max_surprise may reach 20: routed by the engine, no flag
    std::printf("miro %u\n", m.gen_params_for(1, 2, 3, 4, keep).reserved);
    std::printf("flag %u\n", (unsigned)RWKV_GEN_WIDE_TOP_K);
    return 0;
}
'''


def test_gen_params_for_sets_the_wide_flag_exactly_above_256(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    flag = int(lines[-1][1])
    assert lines[-1][0] == "flag" and flag == 1
    assert lines[-2] == ["miro", "0"]
    rows = lines[:-2]
    assert [int(r[0]) for r in rows] == [0, 1, 128, 256, 257, 1000, 65536]
    for k, gn, gt, gp, kn, kt in (map(int, r) for r in rows):
        want = flag if k > 256 else 0                               # `reserved` stays 0 otherwise
        assert (gn, gt, gp) == (want, want, want), (k, gn, gt, gp)
        assert kn == k and kt == k                                  # top_k itself is handed over as it is


def test_the_header_the_sys_crate_and_the_binding_agree_on_the_flag():
    hdr = open(os.path.join(ROOT, "include", "rwkv_abi.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rwkv-hip-sys", "src", "lib.rs")).read()
    c = int(re.search(r"#define\s+RWKV_GEN_WIDE_TOP_K\s+(\d+)", hdr).group(1))
    r = re.search(r"pub const RWKV_GEN_WIDE_TOP_K\s*:\s*(\w+)\s*=\s*(\d+)\s*;", rs)
    assert r and r.group(1) == "u32" and int(r.group(2)) == c == 1   # the type of `reserved`; bit 0
    assert int(re.search(r"#define\s+RWKV_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9      # additive: no new ABI version
    from ai00_server_amd import runtime as rt
    assert rt.GEN_WIDE_TOP_K == c
    import inspect
    for f in (rt.Runtime.gen_arm, rt.Runtime.gen_arm_prompt):
        assert inspect.signature(f).parameters["wide_top_k"].default is False
    wrap = open(os.path.join(ROOT, "integration", "rwkv-hip", "src", "lib.rs")).read()
    assert "sys::RWKV_GEN_WIDE_TOP_K" in wrap

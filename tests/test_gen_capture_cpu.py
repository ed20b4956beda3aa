"""No GPU: the surface of captures and items (rwkv_gen_set_capture / _take_item / _item_free / _item_state / _item_back / _item_from_host /
rwkv_gen_arm_item) is spelled the same way in every layer that names it."""
import fnmatch
import inspect
import os
import re

from ai00_server_amd import harness as H
from ai00_server_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rwkv_gen_set_capture", "rwkv_gen_take_item", "rwkv_gen_item_free", "rwkv_gen_item_state", "rwkv_gen_item_back",
         "rwkv_gen_item_from_host", "rwkv_gen_arm_item"]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_seven_functions_are_exported_bound_and_declared_in_both_crates():
    exported = re.search(r"global:\s*([^;]+);", read("ai00_server_amd", "csrc", "rwkv_abi.map")).group(1).split()
    sys_rs, safe_rs = read("integration", "rwkv-hip-sys", "src", "lib.rs"), read("integration", "rwkv-hip", "src", "lib.rs")
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), f"{name} is not in the export list {exported}"
        assert name in rt.ABI_SYMBOLS
        assert re.search(r"pub fn %s\(" % name, sys_rs), f"{name} is not declared in rwkv-hip-sys"
        assert "sys::%s(" % name in safe_rs, f"{name} is not used by the safe crate"
    assert "pub struct GenItem" in safe_rs and "impl Drop for GenItem" in safe_rs
    assert re.search(r'^version = "0\.9\.\d+"', read("integration", "rwkv-hip-sys", "Cargo.toml"), re.M)


def test_the_header_has_the_flags_and_the_typedef_and_stays_at_abi_9():
    hdr = read("include", "rwkv_abi.h")
    assert re.search(r"#define\s+RWKV_GEN_CAPTURE_PROMPT\s+1u\b", hdr) and re.search(r"#define\s+RWKV_GEN_CAPTURE_FINISH\s+2u\b", hdr)
    assert re.search(r"typedef\s+struct\s+rwkv_gen_item\s+rwkv_gen_item\s*;", hdr)
    assert re.search(r"#define\s+RWKV_ABI_VERSION\s+9\b", hdr)
    assert int(rt.GenCapture.Prompt) == 1 and int(rt.GenCapture.Finish) == 2 and issubclass(rt.GenCapture, __import__("enum").IntFlag)
    cpp = read("include", "rwkv_runtime.hpp")
    for word in ("GenItem", "gen_set_capture", "gen_take_item", "gen_arm_item"):
        assert word in cpp, word


def test_freeing_a_null_item_returns(built_lib):
    l = rt.lib()
    assert l.rwkv_gen_item_free(None) is None
    assert not l.rwkv_gen_item_state(None)
    assert l.rwkv_gen_take_item(None, 0, 1, None) == -1 and l.rwkv_gen_set_capture(None, 0, 1) == -1
    assert l.rwkv_gen_arm_item(None, 0, None, None) == -1 and l.rwkv_gen_item_back(None, None, None, None) == -1
    assert l.rwkv_gen_item_from_host(None, None, None, None) == -1


def test_generate_resident_takes_capture_and_item():
    sig = inspect.signature(H.generate_resident)
    assert sig.parameters["capture"].default == rt.GenCapture(0) and sig.parameters["item"].default is None
    for name in ("state", "row", "back", "from_host", "close"):
        assert callable(getattr(rt.GenItem, name))
    for name in ("gen_set_capture", "gen_take_item", "gen_arm_item"):
        assert callable(getattr(rt.Runtime, name))
    assert "--capture" in read("scripts", "gen_resident_bench.py")

"""The launch geometry of v6_mix_kernel's one-launch forms (gemm_plan.h v6_mix_plan), checked on the CPU: the host function is compiled into
tests/cpp/v6_mix_plan_test.cpp with AddressSanitizer and UBSan and walked with the kernel's own strip rule.

For C in {512, 1024, 2560, 4096}, Dm in {32, 64} and every T of 1 .. 32:
  * every (mix, token tile, strip) is owned by exactly one (block, wave), no block owns a strip past C/16 or more strips than it has waves;
  * the token tiles of the grid cover the step's rows, 16 per tile;
  * 17 .. 32 rows (the token-tile form): at most 256 blocks where the shape allows it — a group holds at most 8 strips, so C = 4096 (256 strips) needs
    32 groups and 320 blocks; below that the grid is the largest that one block per CU allows (250 = 5 x 2 x 25);
  * T <= 16: groups of 8 strips and one token tile, as before the token-tile form;
  * the dynamic LDS stays under 160 KiB.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = (512, 1024, 2560, 4096)
DMS = (32, 64)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("v6_mix_plan") / "v6_mix_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "v6_mix_plan_test.cpp"), "-o", exe])
    keys = [(T, C, Dm) for C in CS for Dm in DMS for T in range(1, 33)]
    out = subprocess.run([exe], input="".join(f"{T} {C} {Dm}\n" for T, C, Dm in keys), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines()]
    assert len(lines) == len(keys)
    return dict(zip(keys, lines))


def test_every_strip_of_every_token_tile_is_owned_once(plans):
    for key, p in plans.items():
        assert (p["owners_min"], p["owners_max"], p["beyond"]) == (1, 1, 0), (key, p)
        assert p["max_group"] <= 8, (key, p)
        assert p["NT"] == 1 and p["grid"][2] == p["token_tiles"] == (key[0] + 15) // 16, (key, p)


def test_token_tile_form_fills_the_chip_without_a_second_round(plans):
    for (T, C, Dm), p in plans.items():
        if T <= 16:
            continue
        blocks = p["grid"][0] * 5 * p["grid"][2]
        need = 5 * 2 * ((C // 16 + 7) // 8)                       # a group holds at most 8 strips
        assert blocks <= max(256, need), ((T, C, Dm), p)
        if need <= 256:
            assert blocks == 5 * 2 * min(25, C // 16), ((T, C, Dm), p)
        else:
            assert blocks == need, ((T, C, Dm), p)
    assert plans[(32, 2560, 32)]["grid"] == [25, 5, 2] and (plans[(32, 2560, 32)]["sq"], plans[(32, 2560, 32)]["sr"]) == (6, 10)
    assert plans[(17, 512, 32)]["grid"] == [25, 5, 2] and (plans[(17, 512, 32)]["sq"], plans[(17, 512, 32)]["sr"]) == (1, 7)


def test_up_to_16_rows_keep_groups_of_8_strips(plans):
    for (T, C, Dm), p in plans.items():
        if T <= 16:
            assert p["grid"] == [C // 128, 5, 1] and (p["sq"], p["sr"]) == (8, 0), ((T, C, Dm), p)


def test_lds_under_160_kib(plans):
    for key, p in plans.items():
        assert 0 < p["lds"] < 160 * 1024, (key, p)
        assert p["lds"] == 8 * 4 * 64 * 16 + 2 * 16 * (key[2] + 8) * 2, (key, p)

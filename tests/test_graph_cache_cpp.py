"""CPU: the policy for keeping captured step graphs (ai00_server_amd/csrc/graph_cache.h) with integer handles and a deleter that records
what it is given.  Compiled with g++, no GPU and no HIP involved; tests/cpp/graph_cache_test.cpp holds the cases."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("graph_cache") / "graph_cache_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "graph_cache_test.cpp"), "-o", path])
    return path


def run(exe, case):
    out = subprocess.run([exe, case], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == f"{case}: ok", out.stdout + out.stderr


def test_a_key_is_captured_on_second_sight_not_on_first(exe):
    run(exe, "second_sight")


def test_the_65th_insert_evicts_the_entry_with_the_oldest_find_not_the_oldest_insert(exe):
    run(exe, "evicts_oldest_find")


def test_find_refreshes_an_entry(exe):
    run(exe, "find_refreshes")


def test_the_seen_set_clears_past_4096_and_the_key_that_caused_it_is_captured_on_its_next_visit(exe):
    run(exe, "seen_set_clears")


def test_the_deleter_runs_once_per_handle_over_eviction_and_teardown(exe):
    run(exe, "deleter_once")


def test_a_cache_with_room_for_every_key_never_calls_the_deleter_before_teardown(exe):
    run(exe, "never_evicts_within_capacity")


def test_the_header_includes_nothing_of_hip():
    src = open(os.path.join(ROOT, "ai00_server_amd", "csrc", "graph_cache.h")).read()
    assert "#include <hip" not in src and "hipGraph" not in src.split("#pragma once")[1]

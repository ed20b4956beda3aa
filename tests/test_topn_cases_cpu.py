"""CPU: the top-n reference and case table of tests/topn_cases.py, proved before they judge a kernel (tests/test_gpu_topn_exact.py,
tests/test_gpu_topn.py): `topn_ref` on hand-written rows, the table on both sides of the kernel's one data-dependent branch, and the checker
against a correct result and against one mistake at a time."""
import math

import numpy as np
import pytest

from tests import topn_cases as T

F32, INF, NONE = np.float32, np.inf, T.TOPN_NONE


def ref(row, n):
    ids, lp = T.topn_ref(np.asarray(row, F32), n)
    return ids.tolist(), lp


def test_all_equal_row_lists_the_first_ids_at_minus_ln_v():
    ids, lp = ref([2.5] * 16, 5)
    assert ids == [0, 1, 2, 3, 4] and np.allclose(lp, -math.log(16), rtol=0, atol=1e-15)


def test_a_tie_straddling_the_last_place_goes_to_the_lower_ids():
    row = [0.0] * 16
    row[9] = 3.0
    for i in (2, 12, 5, 14):
        row[i] = 1.0
    ids, lp = ref(row, 3)                                          # 9, then two of the four ties: the two lowest ids
    assert ids == [9, 2, 5] and lp[1] == lp[2] and lp[0] > lp[1]


def test_the_two_zeros_are_one_value():
    row = [-1.0] * 16
    row[11], row[3], row[7] = 0.0, -0.0, 0.0
    assert ref(row, 4)[0] == [3, 7, 11, 0]


def test_different_logits_never_tie_even_when_their_probabilities_do():
    row = [-INF] * 16
    row[4], row[9], row[2] = 1000.0, -1000.0, np.nextafter(F32(-1000.0), F32(0))   # both underflow to p = 0
    ids, lp = ref(row, 3)
    assert ids == [4, 2, 9] and lp[0] == 0.0


def test_masked_entries_short_rows_and_n_beyond_v():
    row = [-INF] * 16
    row[6], row[1] = 0.5, 0.5
    ids, lp = ref(row, 4)
    assert ids == [1, 6, NONE, NONE] and np.allclose(lp[:2], -math.log(2)) and (lp[2:] == -INF).all()
    ids, lp = ref(np.arange(16), 20)
    assert ids == list(range(15, -1, -1)) + [NONE] * 4 and (lp[16:] == -INF).all() and np.isfinite(lp[:16]).all()
    ids, lp = ref([-INF] * 16, 3)
    assert ids == [NONE] * 3 and (lp == -INF).all()


@pytest.mark.parametrize("bad", [np.nan, INF])
def test_poisoned_rows_list_nothing(bad):
    row = [0.0] * 16
    row[5] = bad
    ids, lp = ref(row, 4)
    assert ids == [NONE] * 4 and np.isnan(lp).all()


def test_the_table_holds_rows_on_both_sides_of_the_search_branch():
    """`striped` takes the exact search at both large vocabularies for every n but 1 (lane l owns 256 entries of value -l: the bound admits
    256 (n - 1) + 1 of them); every other row, and every row of the small vocabularies, does not."""
    for V in T.VOCABS:
        for nm, x in T.rows_of(V).items():
            if nm in ("nan", "pos_inf"):
                continue
            for n in T.NS:
                over = T.candidates(x, n) > T.TOPN_CAND
                assert over == (nm == "striped" and V >= 65520 and n >= 5), (V, nm, n, T.candidates(x, n))
    # the model itself: an all-equal row admits ids 0 .. 4 (n - 1) = the first entry of n lanes and all before it
    assert T.candidates(np.zeros(65536, F32), 32) == 125 and T.candidates(np.zeros(16, F32), 32) == 16


def test_the_table_covers_what_the_issue_lists():
    cases = T.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    assert {c.p["V"] for c in cases} == set(T.VOCABS) and {c.p["n"] for c in cases} == set(T.NS)
    assert {c.p["n_rows"] for c in cases} >= {1, 5} and {c.p["side"] for c in cases} == {0, 1}
    for V in T.VOCABS:
        R = T.rows_of(V)
        assert sum(k.startswith("normal") for k in R) == 8
        assert {"equal", "tie40", "alt_inf", "spike", "zeros", "nan", "pos_inf", "all_inf", "three_live", "striped"} <= set(R)
        assert np.unique(R["tie40"][T.tie_ids(V)]).size == 1 and R["tie40"][T.tie_ids(V)][0] > np.delete(R["tie40"], T.tie_ids(V)).max(initial=-INF)
        lanes = {(i >> 2) % 256 for i in T.tie_ids(V)}
        assert len(T.tie_ids(V)) == min(40, V) and (V < 4096 or (len(lanes) > 8 and {i >> 8 for i in T.tie_ids(V)} > {0}))


SMALL = [c for c in T.all_cases() if c.p["V"] in (16, 272)] + [c for c in T.all_cases() if c.p["V"] == 65536 and c.p["n"] == 20 and c.p["n_rows"] != 1]


def test_the_checker_accepts_the_reference_and_the_untouched_state_fails():
    for c in SMALL:
        d = T.make(c)
        assert T.check_case(c, d, T.reference_results(c, d), T.plan_line(c)) == [], c.name
        assert T.check_case(c, d, T.untouched(d), T.plan_line(c)), c.name


def mutate(c, d, role, f):
    res = T.reference_results(c, d)
    b = {x.role: x for x in d["bufs"]}[role]
    res[role] = res[role].copy()
    f(T.own(res, b), res[role])
    return T.check_case(c, d, res, T.plan_line(c))


def test_the_checker_finds_one_mistake_at_a_time():
    c = next(c for c in T.all_cases() if c.name == "V272_n20_all")
    d = T.make(c)
    n, r = 20, c.o["rows"].index("tie40")

    def swap(o, _):                                                # two ties in the wrong order
        o[r * n], o[r * n + 1] = o[r * n + 1], o[r * n]
    assert any("ids differ" in m for m in mutate(c, d, "out_ids", swap))

    def off(o, _):                                                 # 4e-5 relative on a listed ln-probability
        v = o[0:1].view(F32)
        v[0] = v[0] * F32(1 + 4e-5) - F32(4e-5)
    assert any("logp of place 0" in m for m in mutate(c, d, "out_logp", off))

    def spare(_, whole):                                           # a write into the spare list in front
        whole[T.GUARD + 3] = 7
    assert any("guard band or spare row of out_ids" in m for m in mutate(c, d, "out_ids", spare))

    def pad(o, _):                                                 # NaN instead of -inf behind a short row
        rr = c.o["rows"].index("three_live")
        o[rr * n + 5] = 0x7FC00000
    assert any("must hold -inf" in m for m in mutate(c, d, "out_logp", pad))

    def copy(o, _):
        o[5] ^= 1
    assert any("side copy" in m for m in mutate(c, d, "side_rows", copy))

    def lns(o, _):                                                 # ln S one ulp off: the lists are no longer its bits
        o[2 * c.o["rows"].index("normal3") + 1] += 1
    assert any("bit for bit" in m for m in mutate(c, d, "side_ms", lns))


def test_cross_check_sees_a_row_that_depends_on_its_launch():
    cases = [c for c in T.all_cases() if c.name in ("V272_n5_all", "V272_n5_five")]
    datas = [T.make(c) for c in cases]
    results = [T.reference_results(c, d) for c, d in zip(cases, datas)]
    assert T.cross_checks(cases, results, datas) == []
    b = {x.role: x for x in datas[1]["bufs"]}["out_logp"]
    results[1]["out_logp"] = results[1]["out_logp"].copy()
    T.own(results[1], b)[0] ^= 1
    assert len(T.cross_checks(cases, results, datas)) == 1

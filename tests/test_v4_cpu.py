"""RWKV-4 without a GPU: what the loader says about a V4 file, what it refuses, and the two checkers of the V4 arithmetic
(tests/v4_ref.py, tests/v4_literal.py) against each other."""
import os
import sys
import tempfile

import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import v4_ref
from tests.v4_literal import LiteralV4

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_converted as MC  # noqa: E402
import make_converted_v4 as MC4  # noqa: E402

GREEDY_PROMPT_SLOT, GREEDY_PROMPT_LEN, GREEDY_STEPS = v4_ref.GREEDY_RUN


def fixture_bytes():
    with open(MC4.FIXTURE, "rb") as f:
        return f.read()


def info_tuple(st_bytes):
    i = rt.Loader.info(st_bytes)
    return (int(i.version), i.num_layer, i.num_emb, i.num_hidden, i.num_vocab, i.num_head, i.head_size)


@pytest.mark.parametrize("name", sorted(v4_ref.CONFIGS))
def test_loader_info_on_a_synthetic_v4_checkpoint(built_lib, name):
    _, L, C, F, V = v4_ref.CONFIGS[name]
    assert info_tuple(R.st_serialize(v4_ref.synth_v4(name))) == (4, L, C, F, V, 1, C)


def test_loader_info_on_the_reference_converters_v4_file(built_lib):
    _, L, C, F, V, _ = MC4.CASE
    assert info_tuple(fixture_bytes()) == (4, L, C, F, V, 1, C)
    assert rt.ModelVersion.V4 == 4


def refused(tensors):
    with pytest.raises(rt.RwkvError) as e:
        rt.Loader.info(R.st_serialize(tensors))
    return e.value


def test_v4_is_detected_on_positive_evidence_only(built_lib):
    base = v4_ref.synth_v4("v4-tiny")
    C = base["emb.weight"].shape[1]
    assert info_tuple(R.st_serialize(base))[0] == 4                 # the control: every case below is this file with one thing changed
    t = dict(base)
    del t["blocks.0.att.time_mix_r"]
    e = refused(t)
    assert e.code == -3 and "unsupported model version" in str(e)
    # a tensor of a later version: the file is no V4, and what it is instead is answered as before
    t = dict(base)
    t["blocks.0.att.ln_x.weight"] = np.ones(C, np.float16)
    e = refused(t)
    assert e.code == -3 and "v4 or unknown tensor naming" in str(e)
    t["blocks.0.att.gate.weight"] = np.zeros((C, C), np.float16)
    e = refused(t)
    assert e.code == -3 and "v5.0/v5.1" in str(e)                   # time_decay is a plain vector: the V5.x answer
    t = dict(base)
    t["blocks.0.att.time_first"] = base["blocks.0.att.time_first"][:C // 2].copy()
    e = refused(t)
    assert e.code in (-3, -2) and len(str(e)) > len("rwkv error -3: ")
    # the rules on the dimensions hold for V4 as well: the 50277-token Pile vocabulary is no multiple of 16
    t = dict(base)
    t["emb.weight"] = np.zeros((50277, C), np.float16)
    t["head.weight"] = np.zeros((50277, C), np.float16)
    assert refused(t).code == -3


def test_v4_ref_equals_the_literal_blinkdl_functions_on_the_original_tensors():
    src = MC4.source()
    ref = v4_ref.V4Ref(R.st_deserialize(fixture_bytes()))
    lit = LiteralV4(src)
    V = ref.info.num_vocab
    toks = v4_ref.prompt(V, 21, 12)
    s, ls = ref.init_state(), lit.new_state()
    np.testing.assert_array_equal(s, lit.to_slab_order(ls))
    for t in toks:
        got, want = ref.forward([t], s)[-1], lit.forward(t, ls)
        assert np.abs(got - want).max() <= 1e-9 * max(1.0, float(np.abs(want).max()))
        slab = lit.to_slab_order(ls)
        for row in range(5):                                        # att shift, aa, bb, pp, ffn shift
            g, w = s[row::5], slab[row::5]
            assert np.abs(g - w).max() <= 1e-9 * max(1.0, float(np.abs(w).max())), row


@pytest.mark.skipif(not os.path.exists(MC.CONVERTER), reason="the reference checkout is not on this machine")
def test_committed_v4_fixture_is_the_reference_converters_output():
    with tempfile.TemporaryDirectory() as d:
        assert MC.run_converter(MC4.source(), d) == fixture_bytes()


def test_converter_output_is_the_layout_v4_ref_assumes():
    want, got = MC4.source(), R.st_deserialize(fixture_bytes())
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == np.float16 and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_greedy_ids_of_the_gpu_test_do_not_hang_on_a_near_tie():
    """The GPU test compares greedy ids of an fp16-class engine with the float64 oracle exactly.  That is only a fair demand where no step of
    the run is decided by a margin the arithmetic cannot resolve: an fp32 evaluation of the same oracle must pick the same 96 ids (if it
    did not, the prompt seed would have to change; no step is skipped)."""
    t = v4_ref.synth_v4("v4-tiny")
    p = v4_ref.prompt(v4_ref.CONFIGS["v4-tiny"][4], GREEDY_PROMPT_SLOT, GREEDY_PROMPT_LEN)
    want, _ = v4_ref.V4Ref(t).greedy(p, GREEDY_STEPS)
    got, _ = v4_ref.V4Ref(t, dtype=np.float32).greedy(p, GREEDY_STEPS)
    assert got == want

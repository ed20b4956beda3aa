"""GPU (-m gpu): Quant::SF4 — the load-time quantiser's bytes, every GEMM kernel family on SF4 problems bit for bit, launches that carry fp16, NF4
and SF4 problems side by side, whole models against the oracle, the prefab image and the weight accounting.

The kernel cases run in tests/cpp/sf4_probe.hip, a stand-alone program linked against the kernel objects of the library build: the product's
load-time kernel on raw weights, the engine's own planner, one launch per case, every buffer copied back whole.  The inputs (tests/sf4_cases.py,
proved on the CPU by tests/test_sf4_cpu.py) are one-hot: every output is ONE product of a dequantised weight and a power of two, so the fp64
reference (tests/sf4_ref.py) must be met in EVERY BIT, and whatever a launch does not own must still hold the NaN pattern it was filled with.
One probe process per test, each under its own time limit; a process that does not end normally is recorded and every later probe test of this
module fails at once, starting nothing on the GPU (tests/probe_run.py).  Nothing is retried.

The model tests evaluate the oracle with QUANT_NONE on the `prequantise`d checkpoint — fp16 values, so that is exactly the SF4 model — and hold
the engine (Precision.Fp32) to the project's Fp32 bound, 2e-5 * max(1, |ref|_inf), the `tol` of tests/test_gpu_parity.py."""
import os

import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import sf4_cases as SC
from tests import sf4_ref as S
from tests import v4_ref
from tests.probe_run import require_alive, run_probe

pytestmark = pytest.mark.gpu
CASES = SC.cases()
_STATE = {"dead": None, "plans": {}}
FP32_TOL = 2e-5


@pytest.fixture(scope="module")
def probe():
    from ai00_server_amd import build as B
    return B.build_probe("sf4_probe", verbose=False)


def run_group(probe, tmp_path, group):
    cases = [c for c in CASES if c.group == group]
    datas = [SC.make(c) for c in cases]
    plans, inp, out = run_probe(_STATE, probe, tmp_path, group, cases, lambda path: SC.write_cases(path, cases, datas))
    results = SC.read_results(out, cases, datas)
    os.remove(inp), os.remove(out)
    msgs = []
    for c, d, res, plan in zip(cases, datas, results, plans):
        assert plan["case"] == c.name
        _STATE["plans"][c.name] = plan
        msgs += SC.check_case(c, d, res, plan)
    assert not msgs, f"{len(msgs)} findings in {group}:\n" + "\n".join(msgs[:12])
    return cases, plans


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
def test_quantiser_bytes(probe, tmp_path):
    """48 x 512 arbitrary fp16 weights (scales that are no powers of two, constant blocks, zero blocks): the payload and the scales
    launch_quant_sf4 wrote equal tests/sf4_ref.py's, tiled as NF4 is, in every byte (check_case compares them for every case)."""
    cases, plans = run_group(probe, tmp_path, "quant")
    assert len(cases) == 1 and plans[0]["fmts"] == [SC.SF4]


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
def test_onehot_sf4_bit_for_bit(probe, tmp_path):
    cases, plans = run_group(probe, tmp_path, "onehot")
    assert len(cases) == 13


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
def test_mixed_launches_fp16_nf4_sf4(probe, tmp_path):
    cases, plans = run_group(probe, tmp_path, "mixed")
    assert [p["fmts"] for p in plans] == [[SC.F16, SC.NF4, SC.SF4]] * 2 and [p["path"] for p in plans] == ["decode", "tile"]


def test_the_table_took_the_paths_it_exists_for():
    require_alive(_STATE)
    missing = [c.name for c in CASES if c.name not in _STATE["plans"]]
    assert not missing, f"no plan line for {missing[:8]} (run the whole module)"
    gaps = SC.coverage_gaps(CASES, [_STATE["plans"][c.name] for c in CASES])
    assert not gaps, gaps


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
def tol(want):
    return FP32_TOL * max(1.0, float(np.abs(want).max()))


def err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())


def feed(eng, tokens, chunk=None):
    """slot 0 consumes `tokens`, `chunk` at a time (None: as one request); the last row, copied out of the engine's arena"""
    row = None
    step = chunk or len(tokens)
    for i in range(0, len(tokens), step):
        inp = rt.RnnInput([rt.RnnInputBatch(list(tokens[i:i + step]), rt.RnnOption.Last)])
        while inp.num_token() > 0:
            inp, outs = eng.infer(inp)
            if len(outs[0]):
                row = np.array(outs[0][-1], np.float32)
    return row


MODELS = {"v6-small": 2, "v7-small": 3, "v5-small": 2, "v4-small": 2}     # SF4 layers
PROMPT, LONG, SINGLES = 19, 200, 8
_REF = {}


def model(name):
    """(tensors, tokens, oracle rows after the prompt / the long step / each single-token step) — computed once per model."""
    if name not in _REF:
        if name.startswith("v4"):
            t = v4_ref.synth_v4(name)
            V = t["emb.weight"].shape[0]
            ref = v4_ref.V4Ref(S.prequantise(t, MODELS[name], names=v4_ref.QUANT_NAMES))
            toks = v4_ref.prompt(V, 7, PROMPT + LONG + SINGLES)
        else:
            t = R.synth_named(name)
            ref = R.RwkvRef(S.prequantise(t, MODELS[name]))
            toks = [tk % ref.info.num_vocab for tk in R.synth_prompt(7, PROMPT + LONG + SINGLES)]
        toks = [int(x) for x in toks]
        s = ref.init_state()
        want = [ref.forward(toks[:PROMPT], s)[-1].copy(), ref.forward(toks[PROMPT:PROMPT + LONG], s)[-1].copy()]
        for tk in toks[PROMPT + LONG:]:
            want.append(ref.forward([tk], s)[-1].copy())
        _REF[name] = (t, toks, want)
    return _REF[name]


def build(t, quant, layers):
    return rt.ModelBuilder(R.st_serialize(t)).quant(layers if quant else 0, rt.Quant(quant)).build(max_batch=1, token_chunk_size=256, precision=rt.Precision.Fp32)


@pytest.mark.parametrize("name", list(MODELS))
def test_models_match_the_oracle_on_the_prequantised_checkpoint(name):
    """A 19-token prompt in chunks of 8, one step of 200 rows (the prefill tile kernels), eight single-token steps: the logits after each
    against the oracle at the Fp32 bound.  And the engine ran neither NF4 nor nothing: its logits after the prompt differ from the NF4
    engine's and from the unquantised engine's by more than 1e-2 (the CPU oracle gives 0.068 / 0.121 / 0.081 against NF4 and
    0.057 / 0.081 / 0.063 against unquantised for v6-small / v7-small / v5-small)."""
    t, toks, want = model(name)
    eng = build(t, 3, MODELS[name])
    got = [feed(eng, toks[:PROMPT], 8), feed(eng, toks[PROMPT:PROMPT + LONG])]
    got += [feed(eng, [tk]) for tk in toks[PROMPT + LONG:]]
    eng.close()
    for i, (g, w) in enumerate(zip(got, want)):
        print(f"{name} step {i}: logits err {err(g, w):.3e} (bound {tol(w):.3e})")
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(g).all() and err(g, w) <= tol(w), (name, i, err(g, w), tol(w))
    for other, what in ((2, "NF4"), (0, "unquantised")):
        e2 = build(t, other, MODELS[name])
        row = feed(e2, toks[:PROMPT], 8)
        e2.close()
        print(f"{name}: SF4 against {what}: {err(got[0], row):.3f}")
        assert err(got[0], row) > 1e-2, (name, what)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_prefab_round_trip_weight_bytes_and_the_refused_quant_type(tmp_path):
    t, toks, _ = model("v6-small")
    eng = build(t, 3, 2)
    a = feed(eng, toks[:PROMPT], 8)
    path = str(tmp_path / "sf4.prefab")
    eng.save_prefab(path)
    info, wb = eng.info, eng.weight_bytes
    eng.close()
    nf4 = build(t, 2, 2)
    assert nf4.weight_bytes == wb
    nf4.close()
    image = open(path, "rb").read()
    eng2 = rt.ModelBuilder(image).build(max_batch=1, token_chunk_size=256, precision=rt.Precision.Fp32)   # quant settings come from the image
    assert eng2.info == info and eng2.weight_bytes == wb
    np.testing.assert_array_equal(feed(eng2, toks[:PROMPT], 8), a)
    eng2.close()
    b = rt.ModelBuilder(R.st_serialize(t)).quant(2, rt.Quant.SF4)
    b._quant_type = 4                                                # no `Quant` has this value
    with pytest.raises(rt.RwkvError) as e:
        b.build(max_batch=1)
    assert e.value.code == -3

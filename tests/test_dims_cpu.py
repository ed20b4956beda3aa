"""CPU: what the dimension sweep of tests/test_gpu_dims.py stands on (tests/dims_table.py holds the table and the recipes).

  * the reference is valid at these dims: the numpy restatement (RwkvRefBatch) and the compiled one (oracle/cpu_backend.c) — two independent
    codes of the formulas — agree at every row of the table, LoRA ranks the synthetic checkpoints never had included, quantised forms too;
  * `synth_checkpoint(lora_dims=None)` draws what it always drew;
  * the sampler draws of the GPU test stay clear of CDF boundaries on the oracle's own logits;
  * the GEMM planner's geometry covers every launch the sweep makes exactly, and takes no path whose kernel cannot run the shape."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import rwkv_ref as R
from tests import dims_table as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# sha256 over (name, shape, bytes) of every tensor, recorded before `lora_dims` existed
DEFAULT_SYNTH = {
    "v5-tiny": "14b3254145145efddb3f9c6c01a99ac3b1827f83efc3d3baca41ec82a50d83b2",
    "v6-tiny": "eea93651523724922598b04c72e02cdc14f35549fe261bbd6b07aed0b2dc813b",
    "v7-tiny": "95eb26573cc83c64e56a0a53753815ab988a379d1e75b537064ebb2f4d38402f",
    "v6-small": "08f044b063f4d7a5a3dfc063cb35a5b2bd84c8505f773009bbccafbcf85f2a2f",
    "v5-small": "4cdf4da5dbad18ed7f0799416b3ab1b6afbed097e2dc94c962dc24c0f206d66c",
    "v7-small": "450ff878399e8bf797c76ce91a0c9a0b5968fbf5b964c08dc21316aea62fe0f9",
    # the other branches of the default ranks (V6 at C >= 4096, V7 at C >= 2560 and at 1024 <= C < 2560), one layer, small F and V
    (6, 1, 4096, 256, 16): "aecdf105a333eb6ec549221d852aead8ee78af4a0a77301e96bec286ac8c5b68",
    (7, 1, 2560, 256, 16): "1eeb706d65b5da348796fda11eb95959b815ac62f4fb44bb1bcbd411ddbc1add",
    (7, 1, 1024, 256, 16): "4c46e72c987ff3da69b63edbd65d8b36a8feb976348ceb5cec18f92af1e0238b",
}


@pytest.mark.parametrize("key", list(DEFAULT_SYNTH), ids=[str(k) for k in DEFAULT_SYNTH])
def test_default_synthetic_checkpoints_did_not_move(key):
    t = R.synth_checkpoint(*(R.CONFIGS[key] if isinstance(key, str) else key))
    h = hashlib.sha256()
    for k, v in t.items():
        h.update(k.encode()); h.update(str(v.shape).encode()); h.update(v.tobytes())
    assert h.hexdigest() == DEFAULT_SYNTH[key]


def test_lora_dims_set_the_ranks_and_nothing_else():
    for i, r in enumerate(D.TABLE):
        if r.lora is None:
            continue
        t = R.synth_checkpoint(r.ver, 1, r.C, r.F, r.V, lora_dims=r.lora, shapes_only=True)
        if r.ver == 6:
            assert t["blocks.0.att.time_mix_w1"] == (5 * r.lora[0], r.C) and t["blocks.0.att.time_mix_w2"] == (5, r.C, r.lora[0])
            assert t["blocks.0.att.time_decay_w1"] == (r.lora[1], r.C) and t["blocks.0.att.time_decay_w2"] == (r.C, r.lora[1])
        else:
            for n, d in zip("wavg", (r.lora[0], r.lora[1], r.lora[2], r.lora[3])):
                assert t[f"blocks.0.att.{n}1"] == (d, r.C) and t[f"blocks.0.att.{n}2"] == (r.C, d)


def _cross_check(tens, quant):
    """Ragged prefill of five slots, then 8 lock-step decode steps (arg-max fed back): logits and state slabs of the two restatements, with the
    bounds of tests/test_oracle.py test_compiled_restatement_agrees_with_the_numpy_one."""
    from oracle.cpu_backend import CpuBackend
    rb, cb = R.RwkvRefBatch(tens, *quant), CpuBackend(tens, *quant)
    B, V = 5, rb.info.num_vocab
    ps = [[x % V for x in R.synth_prompt(30 + s, 2 + 3 * s)] for s in range(B)]
    s1, s2 = rb.init_states(B), cb.init_states(B)
    last = [None] * B
    for t in range(max(len(p) for p in ps)):
        act = [b for b in range(B) if t < len(ps[b])]
        u1, u2 = np.ascontiguousarray(s1[act]), np.ascontiguousarray(s2[act])
        a, b_ = rb.step([ps[b][t] for b in act], u1), cb.step([ps[b][t] for b in act], u2)
        s1[act], s2[act] = u1, u2
        assert np.abs(a - b_).max() <= 1e-5 * max(1.0, float(np.abs(a).max())), ("prefill", t)
        for j, b in enumerate(act):
            last[b] = a[j]
    cur = [int(np.argmax(x)) for x in last]
    for step in range(8):
        a, b_ = rb.step(cur, s1), cb.step(cur, s2)
        assert np.abs(a - b_).max() <= 1e-5 * max(1.0, float(np.abs(a).max())), step
        assert (np.argmax(a, axis=1) == np.argmax(b_, axis=1)).all()
        assert np.abs(s1 - s2).max() <= 2e-5 * max(1.0, float(np.abs(s1).max()))
        cur = [int(x) for x in np.argmax(a, axis=1)]


@pytest.mark.parametrize("i", range(len(D.TABLE)), ids=[D.row_id(i) for i in range(len(D.TABLE))])
def test_the_two_restatements_agree_at_every_row(i):
    """Every row, the ones the loader refuses included (the oracle has no such limit: its GEMM takes any K)."""
    tens = D.tensors(i)
    _cross_check(tens, (0, 0))
    if D.quantisable(D.TABLE[i]):
        _cross_check(tens, (2, R.QUANT_INT8))
        _cross_check(tens, (2, R.QUANT_NF4))


@pytest.mark.parametrize("i", D.SAMPLER_ROWS, ids=[D.row_id(i) for i in D.SAMPLER_ROWS])
def test_sampler_draws_keep_their_margin_on_the_oracles_logits(i):
    """The draws of test_gpu_dims.test_on_device_sampling_at_small_vocabularies on the ORACLE's logits: at most 1 in 16 within the margin
    at which that test stops comparing ids — half its own cap of 1 in 8, the other half is the device's rounding."""
    rb = R.RwkvRefBatch(D.tensors(i))
    draws = skipped = 0
    for kind, margin in D.sampler_walk(i, lambda toks, states: rb.step(toks, states), rb.init_states(len(D.sampler_configs(D.TABLE[i].V)))):
        draws += 1
        skipped += margin <= D.SAMPLER_MARGIN[kind]
    assert draws == D.SAMPLER_STEPS * len(D.sampler_configs(D.TABLE[i].V))
    assert skipped * 16 <= draws, (skipped, draws)


# ------------------------------------------------------------------------------------------------
# planner invariants over every launch of the sweep
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "gemm_plan_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "gemm_plan_test.cpp"), "-o", exe])
    cases, seen = [], set()
    for c in D.sweep_launches():
        line = " ".join(str(w) for w in [c["T"], c["hilo"], c["commit"], 0, -1, 1, -1, len(c["probs"])] + [x for p in c["probs"] for x in p])
        if line not in seen:
            seen.add(line)
            cases.append((c, line))
    out = subprocess.run([exe, "geometry"], input="\n".join(l for _, l in cases) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(cases)
    plans = []
    for (c, _), g in zip(cases, got):
        w = g.split()
        kind, (variant, grid, threads, ksplit, total, spt, bt, n) = w[0], (int(x) for x in w[1:9])
        probs = [dict(zip(("Kb", "ksb", "nslice", "nblk_strip", "spb", "nw", "block_begin", "tile_blocks"), (int(x) for x in w[9 + 8 * j:17 + 8 * j]))) for j in range(n)]
        plans.append((c, dict(kind=kind, variant=variant, grid=grid, threads=threads, ksplit=ksplit, total=total, spt=spt, bt=bt, probs=probs)))
    return plans


def test_planner_geometry_covers_every_launch_of_the_sweep(planned):
    assert len(planned) > 500
    kinds = set()
    for c, p in planned:
        ctx = (D.row_id(c["row"]), c["name"], c["T"], c["hilo"], c["quant"], p)
        kinds.add(p["kind"])
        assert p["ksplit"] >= 1, ("a linear problem's K cannot be split", ctx)
        begin = 0
        for (rows, K, fmt, partial, kcopies, smallk), g in zip(c["probs"], p["probs"]):
            assert rows % 16 == 0 and K % 32 == 0, ctx
            assert g["block_begin"] == begin, ctx                                   # contiguous
            if p["kind"] == "decode":
                assert g["Kb"] * g["ksb"] == K, ctx
                assert g["Kb"] % (32 if fmt == 0 else 256) == 0, ctx                 # a block's K range is whole k-tiles / quantisation groups
                assert g["nslice"] * 256 >= g["Kb"] and (g["nslice"] - 1) * 256 < g["Kb"], ctx
                assert g["nblk_strip"] * g["spb"] >= rows // 16 and (g["nblk_strip"] - 1) * g["spb"] < rows // 16, ctx
                assert partial or g["ksb"] == 1, ctx                                 # only a linear epilogue may sum slabs
                assert 1 <= g["nw"] <= 16 and g["nw"] * 64 <= p["threads"], ctx
                begin += g["nblk_strip"] * g["ksb"]
            elif p["kind"] == "smallk":
                assert K <= D.SK_KMAX and K % 32 == 0 and rows % 16 == 0 and fmt == 0 and smallk and not partial, ctx
                assert g["Kb"] == K and g["ksb"] == 1 and g["nblk_strip"] == rows // 16, ctx
                begin += rows // 16
            else:
                assert c["T"] >= 193, ctx
                assert g["tile_blocks"] == -(-(rows // 16) // p["spt"]) * -(-c["T"] // p["bt"]), ctx   # every strip and every token tile has a block
                assert g["ksb"] == p["ksplit"] and (p["ksplit"] == 1 or (partial and kcopies)), ctx
                assert p["variant"] < 10 or K % 128 == 0, ("a pipelined shape needs K % 128 == 0", ctx)
                begin += g["tile_blocks"] * g["ksb"]
        assert begin == p["total"], ctx
        if p["kind"] == "smallk":
            assert c["T"] <= 64 and not c["commit"], ctx
            assert p["grid"] == (p["total"] + 3) // 4, ctx
        else:
            assert p["grid"] == p["total"] + (c["commit"] if p["kind"] == "decode" else 0), ctx
    assert kinds == {"decode", "smallk", "tile"}


def test_the_sweep_reaches_the_planner_branches_it_is_for(planned):
    """What tests/test_gpu_dims.py then proves from the engine's own launch log, here from the plans: the branches exist in the sweep."""
    tile_lo_fp32 = tile_lo_fp16 = tail_split = smallk_ok = False
    for c, p in planned:
        Ks = [q[1] for q in c["probs"]]
        if p["kind"] == "tile" and p["variant"] < 10 and any(K % 128 for K in Ks):
            tile_lo_fp32 |= c["fp32"]
            tile_lo_fp16 |= not c["fp32"]
        if p["kind"] == "decode" and p["ksplit"] > 1 and any(g["Kb"] % 256 for g in p["probs"]):
            tail_split = True
        if p["kind"] == "smallk":
            smallk_ok = True
            assert max(Ks) <= D.SK_KMAX
        if c["name"] == "lora2" and max(Ks) > D.SK_KMAX:
            assert p["kind"] != "smallk"
    assert tile_lo_fp32 and tile_lo_fp16 and tail_split and smallk_ok

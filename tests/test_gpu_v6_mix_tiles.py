"""GPU (-m gpu): the token-tile decode form of v6_mix_kernel (gemm_plan.h v6_mix_plan): steps of 17 .. 32 rows run the V6 token-shift LoRA as two
16-token tiles of the NT = 1 kernel, strip groups sized for one block per CU.

Model: two-layer V6, C = 512 (the smallest width v6_mix_supported accepts: 32 strips in 25 groups of 1 or 2 — uneven groups, waves without a
strip in every block), LoRA width Dm = 32 and, through synth_checkpoint's lora_dims, Dm = 64 (R.model_info confirms the width that was built).
fp16 and Int8 weights; Precision.Fp16 (plain operands into the mix launch, hi + lo out of it for the promoted class) and Precision.Fp32 (hi + lo
throughout).  Dense decode steps at 17, 20, 31 and 32 active slots (a ragged second token tile: the row clamp and the store predicate) and at
16 (one tile, groups of 8 strips: the dispatch boundary).

Asserted: logits and the state read back within 1e-3 * max(1, |ref|inf) of R.RwkvRefBatch, arg-max ids by the tie rule of
tests/test_gpu_knobs.py, and the same bits from a second engine (the ownership of (token tile, strip) pairs is a fixed function of the block index).

NOT asserted: the bits of a 17 .. 32-slot step against the same slots run as two steps of <= 16.  Inside the mix launch the identity holds by
construction — per token the K split over the 8 waves, the order of the LDS reduce, the tanh, the (hi, lo) rounding of m_c and the epilogue do not
depend on which block owns the token — and tests/test_gpu_mix_exact.py holds that launch to an exact reference at T = 17 .. 32 bit for bit.  A whole
engine step is more than that launch: the GEMMs after it pick their variant (token tiles per block, K split over waves and blocks) by the step's row
count, so a 32-row step and two 16-row steps sum the same products in different orders.  The logits of the two schedules are therefore held to the
oracle tolerance only (each is, separately)."""
import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R

pytestmark = pytest.mark.gpu
FP16_TOL = 1e-3
B = 32
STEPS = (32, 17, 20, 31, 16, 32)


def tol(want):
    return FP16_TOL * max(1.0, float(np.abs(want).max()))


@pytest.fixture(scope="module")
def models():
    out = {}
    for Dm in (32, 64):
        tens = R.synth_checkpoint(6, 2, 512, 1792, 1024, seed=210 + Dm, lora_dims=(Dm, 64))
        assert tens["blocks.0.att.time_mix_w1"].shape == (5 * Dm, 512) and tens["blocks.0.att.time_mix_w2"].shape == (5, 512, Dm)
        out[Dm] = (tens, R.st_serialize(tens))
    return out


@pytest.fixture(scope="module")
def reference(models):
    """{(Dm, quant): (first tokens, per step logits, final states)} — computed once, read by every case."""
    out = {}
    for Dm, (tens, _) in models.items():
        for quant in (0, 1):
            rb = R.RwkvRefBatch(tens, 2 if quant else 0, quant)
            states = rb.init_states(B)
            ps = [[t % 1024 for t in R.synth_prompt(300 + b, 2)] for b in range(B)]
            lg0 = rb.prefill(ps, states)
            cur = [int(np.argmax(lg0[b])) for b in range(B)]
            first, steps = list(cur), []
            for nact in STEPS:
                sub = states[:nact].copy()
                lg = rb.step(cur[:nact], sub)
                states[:nact] = sub
                steps.append(lg)
                for b in range(nact):
                    cur[b] = int(np.argmax(lg[b]))
            for a in (lg0, states, *steps):
                a.setflags(write=False)
            out[(Dm, quant)] = (ps, lg0, first, steps, states)
    return out


def run_engine(st, quant, prec, ref):
    ps, lg0, first, steps, states = ref
    eng = rt.ModelBuilder(st).quant(2 if quant else 0, rt.Quant(quant)).build(max_batch=B, token_chunk_size=512, precision=prec)
    inp = rt.RnnInput([rt.RnnInputBatch(list(p), rt.RnnOption.Last) for p in ps])
    while inp.num_token() > 0:
        inp, _ = eng.infer(inp)
    cur, got = list(first), []
    for nact, want in zip(STEPS, steps):
        _, outs = eng.infer(rt.RnnInput([rt.RnnInputBatch([cur[b]] if b < nact else [], rt.RnnOption.Last) for b in range(B)]))
        lg = np.stack([outs[b][-1] for b in range(nact)])
        worst = 0.0
        for b in range(nact):
            err = float(np.abs(lg[b] - want[b]).max())
            worst = max(worst, err / tol(want[b]))
            gi, wi = int(np.argmax(lg[b])), int(np.argmax(want[b]))
            assert gi == wi or float(want[b][wi] - want[b][gi]) <= 2.0 * err, (nact, b, gi, wi)
            cur[b] = wi
        print(f"step of {nact} slots: max |err| / tol = {worst:.3f}")
        assert worst <= 1.0, (nact, worst)
        got.append(lg)
    back = np.stack([eng.state.back(b) for b in range(B)])
    eng.close()
    serr = max(float(np.abs(back[b] - states[b]).max()) / tol(states[b]) for b in range(B))
    print(f"state: max |err| / tol = {serr:.3f}")
    assert serr <= 1.0, serr
    return got, back


@pytest.mark.parametrize("prec", [rt.Precision.Fp16, rt.Precision.Fp32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("quant", [0, 1], ids=["f16w", "int8w"])
@pytest.mark.parametrize("Dm", [32, 64])
def test_token_tile_steps_give_the_oracles_answers_and_the_same_bits_twice(models, reference, Dm, quant, prec):
    tens, st = models[Dm]
    assert R.model_info(tens).num_emb == 512
    a, sa = run_engine(st, quant, prec, reference[(Dm, quant)])
    b, sb = run_engine(st, quant, prec, reference[(Dm, quant)])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(sa, sb)

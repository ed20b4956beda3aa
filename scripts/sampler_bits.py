"""Dump of what the on-device samplers return, bit for bit: one line per draw — case, u, token id, out_prob as the hex of its float32 bits.

    python scripts/sampler_bits.py OUT.txt
    RWKV_HIP_LIB=$PWD/ai00_server_amd/librwkv_hip_NAME.so python scripts/sampler_bits.py OTHER.txt && cmp OUT.txt OTHER.txt

The check of a change to nucleus_kernel / sample_wide_kernel that must not move a result: two libraries must write identical files.
Every draw goes through rwkv_infer_sample on the prompt's row from the initial state.  The models are the tests' (the smallest that reach
each branch; tests/test_gpu_sample_wide.py, tests/test_gpu_parity.py):
  x8 x4 x1  synth_checkpoint(6, 1, 128, 448, 65536, seed=5), head x 8 / x 4 / x 1: the FULL instantiations; a peaked, a two-window, a flat row
  ties      the same with head.weight[1000:9000] := the arg-max row: an 8001-way tie, more than the narrow buffer holds and more than a
            wide window's k admits, so the id-bound search runs under both conditions
  m20000    synth_checkpoint(6, 1, 128, 448, 20000): the bounded instantiation, a partial last window
  v512      synth_named("v6-tiny"): V below one window
Every setting that fits the vocabulary (top_k <= V) runs on every model with the uniforms 0.0, 0.999999 (find_or_first) and four seeded
draws; the last case of a model is a four-row call that mixes narrow and wide rows.  Prints the number of lines written: the grid fixes
it, so it is the same for every library."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 4


def models():
    from oracle import rwkv_ref as R

    def m65536(scale):
        t = R.synth_checkpoint(6, 1, 128, 448, 65536, seed=5)
        t["head.weight"] = t["head.weight"] * np.asarray(scale, t["head.weight"].dtype)
        return t

    def ties():
        t = m65536(1)
        p = [int(x) for x in R.synth_prompt(90, 5)]
        ref = R.RwkvRef(t)
        t["head.weight"][1000:9000] = t["head.weight"][int(np.argmax(ref.forward(p, ref.init_state())[-1]))]
        return t

    yield "x8", m65536(8)
    yield "x4", m65536(4)
    yield "x1", m65536(1)
    yield "ties", ties()
    yield "m20000", R.synth_checkpoint(6, 1, 128, 448, 20000)
    yield "v512", R.synth_named("v6-tiny")


def settings(V):
    """(name, sampler factory) of every setting a vocabulary of V reaches"""
    from ai00_server_amd import harness as H

    def nucleus(k, p, t):
        return lambda: H.NucleusSampler(top_p=p, top_k=k, temperature=t, presence_penalty=0.0, frequency_penalty=0.0)

    def typical(k, tau):
        return lambda: H.TypicalSampler(tau=tau, top_k=k, temperature=1.0, presence_penalty=0.0, frequency_penalty=0.0)

    def mirostat(ms):
        def mk():
            s = H.MirostatSampler()
            s.max_surprise = np.float32(ms)
            return s
        return mk

    out = [(f"nucleus k{k} p{p} t{t}", nucleus(k, p, t)) for k in (0, 1, 40, 256) for p in (0.3, 0.9, 1.0) for t in (0.7, 1.0, 1.5)]
    out += [(f"typical k{k} tau{tau}", typical(k, tau)) for k in (40, 256) for tau in (0.5, 0.95)]
    out += [(f"mirostat s{ms}", mirostat(ms)) for ms in (6.0, 12.5)]
    out += [(f"nucleus k{k} p0.9 t1.0", nucleus(k, 0.9, 1.0)) for k in (257, 1000, 5000, 20000) if k <= V]
    out += [("nucleus kV p2.0 t1.0", nucleus(V, 2.0, 1.0))]       # every window, both passes
    out += [(f"typical k{k} tau0.9", typical(k, 0.9)) for k in (1024,) if k <= V]
    out += [("typical kV tau2.0", typical(V, 2.0))]
    out += [(f"mirostat s{ms}", mirostat(ms)) for ms in (13.0, 16.0, 17.5)]
    mixed = [nucleus(40, 0.9, 1.0), nucleus(257, 0.9, 1.0), mirostat(12.5), mirostat(16.0)]   # narrow, wide, narrow, wide
    return out, mixed


def main(path):
    from ai00_server_amd import runtime as rt
    from oracle import rwkv_ref as R
    lines = []
    for name, tens in models():
        V = int(tens["head.weight"].shape[0])
        prompt = [int(t) % V for t in R.synth_prompt(90, 5)]
        eng = rt.ModelBuilder(R.st_serialize(tens)).build(max_batch=B, token_chunk_size=32, precision=rt.Precision.Fp32)
        del tens

        def call(smps, us):
            for b in range(B):
                eng.state.load(eng.state.init(), b)
            inp = rt.RnnInput([rt.RnnInputBatch(list(prompt) if smps[b] is not None else []) for b in range(B)])
            return eng.infer_sample(inp, smps, us)[1]

        def line(case, u, got):
            lines.append(f"{name} {case} u={u!r} token={got[0]} prob={int(np.float32(got[1]).view(np.uint32)):08x}")

        single, mixed = settings(V)
        rng = np.random.default_rng(20260119)
        for case, mk in single:
            for u in [0.0, 0.999999] + [float(x) for x in rng.random(4)]:
                line(case, u, call([mk(), None, None, None], [u, 0.0, 0.0, 0.0])[0])
        for u in [0.0, 0.999999] + [float(x) for x in rng.random(4)]:
            got = call([mk() for mk in mixed], [u] * B)
            for b in range(B):
                line(f"mixed row{b}", u, got[b])
        eng.close()
        print(name, "V", V, "lines so far", len(lines), flush=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(len(lines))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

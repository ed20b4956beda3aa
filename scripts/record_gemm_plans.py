"""Record the GEMM launch parameters of one engine over the step sizes on both sides of every planning threshold (GPU).

    python scripts/record_gemm_plans.py --list                    # engine names, one per line
    python scripts/record_gemm_plans.py <engine> <out.jsonl>      # one engine, RWKV_LAUNCH_LOG GEMM lines appended to <out.jsonl>
    python scripts/record_gemm_plans.py --pack <dir> <fixture.json.xz>   # de-duplicate the per-engine files of <dir> into the fixture

An engine is `<width>/<quant>/<precision>[/<SWITCH>=<value>]`: a two-layer synthetic checkpoint of that width with the 65536-row
head.  Every step size runs three ways: one slot with T tokens (last row emitted), one slot with T tokens and every row emitted
(the head at T rows), and, up to 64 rows, T slots with one token each (the dense decode step).  RWKV_HIP_LIB selects the library,
so the same script records a build of another commit.  tests/golden/gemm_plans.json.xz is the --pack of one run of every engine;
tests/test_gemm_plan_cpp.py replays it through the planner without a GPU.
"""
import glob
import json
import lzma
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS = {   # name: (version, layers, C, F, V) — the BASELINE models' widths, two layers
    "v5-24h": (5, 2, 1536, 5376, 65536),
    "v6-1.6b": (6, 2, 2048, 7168, 65536),
    "v6-3b": (6, 2, 2560, 8960, 65536),
    "v6-7b": (6, 2, 4096, 14336, 65536),
    "v7-2.9b": (7, 2, 2560, 10240, 65536),
}
STEPS = [1, 16, 17, 32, 33, 64, 65, 192, 193, 256, 320, 321, 512, 548, 768, 769, 1024, 1280, 1281, 2048]
MAX_BATCH, CHUNK = 64, 2048


def engines():
    out = ["v5-24h/fp16/Fp16", "v5-24h/int8/Fp16",
           "v6-1.6b/fp16/Fp16", "v6-1.6b/nf4/Fp16",
           "v6-3b/int8/Fp16", "v6-3b/int8/Fp16Raw", "v6-3b/int8/Fp32", "v6-3b/fp16/Fp16", "v6-3b/nf4/Fp16",
           "v6-7b/fp16/Fp16", "v6-7b/fp16/Fp32", "v6-7b/int8/Fp16Raw",
           "v7-2.9b/nf4/Fp16", "v7-2.9b/nf4/Fp16Raw", "v7-2.9b/nf4/Fp32", "v7-2.9b/int8/Fp16", "v7-2.9b/fp16/Fp16"]
    out += [f"v6-3b/int8/Fp16/RWKV_TILE_SHAPE={s}" for s in range(13)]
    out += ["v6-3b/int8/Fp16/RWKV_NO_TILE=1", "v6-3b/int8/Fp16/RWKV_TILE_KSPLIT=0"]
    return out


def checkpoint(width):
    """The synthetic `.st` image of a width, cached in the temporary directory (every engine of a width is its own process)."""
    import numpy as np
    from oracle import rwkv_ref as R
    path = os.path.join(tempfile.gettempdir(), f"gemm_plans_{width}.st")
    if os.path.exists(path):
        return np.fromfile(path, np.uint8)
    R.CONFIGS[width] = WIDTHS[width]
    st, _ = R.synth_st(width)
    st.tofile(path + ".part")
    os.replace(path + ".part", path)
    return st


def record(engine, out_path):
    width, quant, precision, *switch = engine.split("/")
    for s in switch:
        k, v = s.split("=")
        os.environ[k] = v
    log = out_path + ".raw"
    if os.path.exists(log):
        os.remove(log)
    os.environ["RWKV_LAUNCH_LOG"] = log
    from ai00_server_amd import runtime as rt
    from oracle import rwkv_ref as R
    st = checkpoint(width)
    L = WIDTHS[width][1]
    q = {"fp16": rt.Quant.NONE, "int8": rt.Quant.Int8, "nf4": rt.Quant.NF4}[quant]
    eng = rt.ModelBuilder(st).quant(0 if quant == "fp16" else L, q).build(max_batch=MAX_BATCH, token_chunk_size=CHUNK,
                                                                         precision=rt.Precision[precision])
    steps = [t for t in STEPS if t >= 193] if switch and "RWKV_TILE_KSPLIT" not in switch[0] and "RWKV_NO_TILE" not in switch[0] else STEPS
    V = WIDTHS[width][4]

    def run(batches):
        inp = rt.RnnInput([rt.RnnInputBatch(list(b), o) for b, o in batches] +
                          [rt.RnnInputBatch([], rt.RnnOption.Last) for _ in range(MAX_BATCH - len(batches))])
        while inp.num_token() > 0:
            inp, _ = eng.infer(inp)

    for T in steps:
        toks = [t % V for t in R.synth_prompt(0, T)]
        run([(toks, rt.RnnOption.Last)])
        run([(toks, rt.RnnOption.Full)])
        if T <= MAX_BATCH:
            run([([toks[s]], rt.RnnOption.Last) for s in range(T)])
    eng.close()
    with open(log) as f, open(out_path, "a") as o:
        for ln in f:
            d = json.loads(ln)
            if d["kind"] == "row":
                continue
            d["engine"] = engine
            o.write(json.dumps(d) + "\n")
    os.remove(log)
    print(f"{engine}: recorded", flush=True)


def normalise(d, np_in=None):
    """What the fixture keeps of a GEMM line: no byte / flop counts, no layer number in the matrix names."""
    d = {k: v for k, v in d.items() if k not in ("bytes", "flops")}
    d["mats"] = re.sub(r"blocks\.\d+\.", "", d["mats"])
    if np_in is not None:
        d["np_in"] = np_in
    return d


def pack(src_dir, fixture):
    seen, lines = set(), []
    for path in sorted(glob.glob(os.path.join(src_dir, "*.jsonl"))):
        fv_ksplit = 0
        for ln in open(path):
            d = json.loads(ln)
            # single-token steps of V6: whether the time-mix launch carries the token-shift commit depends on how many partial slabs its
            # LayerNorm prologue sums — the K split the log shows for the previous layer's ffn.value launch (0 at layer 0).  Kept as `np_in`.
            np_in = None
            if d["T"] == 1 and re.match(r"blocks\.\d+\.att\.key\.weight", d["mats"]):
                np_in = 0 if d["mats"].startswith("blocks.0.") else fv_ksplit
            if "ffn.value.weight" in d["mats"]:
                fv_ksplit = d["ksplit"]
            s = json.dumps(normalise(d, np_in), sort_keys=True)
            if s not in seen:
                seen.add(s)
                lines.append(s)
    lines.sort()
    with open(fixture, "wb") as f:
        f.write(lzma.compress(("[\n" + ",\n".join(lines) + "\n]\n").encode(), preset=9 | lzma.PRESET_EXTREME))
    print(f"{fixture}: {len(lines)} GEMM launches, {os.path.getsize(fixture)} bytes")


if __name__ == "__main__":
    if sys.argv[1] == "--list":
        print("\n".join(engines()))
    elif sys.argv[1] == "--pack":
        pack(sys.argv[2], sys.argv[3])
    else:
        record(sys.argv[1], sys.argv[2])

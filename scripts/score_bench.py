"""Perplexity of one document through the two paths the library has, on one engine in one process:

    full_rows   harness.perplexity        rwkv_infer with RnnOption::Full: every [V] row crosses PCIe, the host exponentiates it (run.rs:699-755)
    scored      harness.perplexity_scored rwkv_infer_score: the realised token is scored on the device, 4 bytes per token come back

    python scripts/score_bench.py [--out profiles/r8_score_vs_full.json] [--tokens 1024] [--chunk 128] [--regions 5]

Workload: synthetic RWKV-V6-3B, Int8 on every layer, default precision, one slot, a `--tokens`-token document, token_chunk_size `--chunk`.
Each path is warmed with one untimed region (graphs captured, code objects loaded); the `--regions` timed regions of the two paths alternate, so
that drift of the machine hits both alike; a region is a host clock around a whole request, which ends in a device synchronise (both paths wait for
their last call's results); the median is reported with the spread.  `full_rows_infer_only` times the rwkv_infer calls of the first path without
the host's exp / sum over the rows (what the transport alone costs), for orientation.  Bytes are what crosses PCIe device-to-host per request."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ai00_server_amd import harness as H  # noqa: E402
from ai00_server_amd import runtime as rt  # noqa: E402
from oracle import rwkv_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--workload", default="v6-3b")
    ap.add_argument("--tokens", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    st, tensors = R.synth_st(a.workload, fast=True)
    info = R.model_info(tensors)
    del tensors
    eng = rt.ModelBuilder(st).quant(info.num_layer, rt.Quant.Int8).build(max_batch=1, token_chunk_size=a.chunk, precision=rt.Precision.Fp16)
    V = info.num_vocab
    doc = [t % V for t in R.synth_prompt(1200, a.tokens - 1)]       # tokens' = [0] + doc: `--tokens` rows
    loop = H.InferLoop(eng)
    zero = eng.state.init()

    def full_rows():
        eng.state.load(zero, 0)
        t = time.perf_counter()
        v = H.perplexity(loop, 0, doc)
        return time.perf_counter() - t, v

    def scored():
        eng.state.load(zero, 0)
        t = time.perf_counter()
        v = H.perplexity_scored(eng, 0, doc)
        return time.perf_counter() - t, v

    def full_rows_infer_only():
        eng.state.load(zero, 0)
        t = time.perf_counter()
        req = loop.submit(H.InferRequest(0, [0] + doc, rt.RnnOption.Full))
        loop.run_pending()
        return time.perf_counter() - t, float(len(req.outputs))

    paths = {"full_rows": full_rows, "scored": scored, "full_rows_infer_only": full_rows_infer_only}
    times = {k: [] for k in paths}
    values = {}
    for k, f in paths.items():                                      # warm-up, untimed
        f()
    for _ in range(a.regions):
        for k, f in paths.items():
            s, v = f()
            times[k].append(s)
            values[k] = v
    rows = a.tokens
    res = {"workload": a.workload, "quant": "int8", "tokens": rows, "chunk": a.chunk, "num_vocab": V, "regions": a.regions,
           "seconds_median": {k: statistics.median(v) for k, v in times.items()},
           "seconds_min_max": {k: [min(v), max(v)] for k, v in times.items()},
           "bytes_device_to_host": {"full_rows": rows * V * 4, "scored": rows * 4, "full_rows_infer_only": rows * V * 4},
           "bytes_host_to_device_targets": {"full_rows": 0, "scored": rows * 4},
           "perplexity": {"full_rows": values["full_rows"], "scored": values["scored"]},
           "note": "perplexity of the full_rows path is inf / nan when a synthetic logit passes ~88 (exp without max subtraction, as the reference)"}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()

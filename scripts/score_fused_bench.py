"""Per-step time of `rwkv_infer_score_fused` against `rwkv_infer_score`, one engine, one process:

    python scripts/score_fused_bench.py [--out profiles/r19_score_fused.json] [--chunks 2048,256] [--regions 5] [--reps 8]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python scripts/score_fused_bench.py --trace
    python scripts/score_fused_bench.py --kernels OUT/.../p_kernel_trace.csv --out profiles/r19_score_fused.json     (merges the trace into the file)

Workload: synthetic RWKV-V6-3B, Int8 on every layer, default precision, 32 slots; per token_chunk_size one 2048-token scored prompt and 32 prompts of
64 scored tokens.  A region is `--reps` whole requests from the initial state under a host clock; every call ends in a device synchronise.  Each path
is warmed with one untimed region (graphs captured), the timed regions of the two paths alternate, medians and spreads are reported, per step = per
call of the entry point.  `--trace` runs every step shape ONCE per path: a shape's first step is launched directly, so no graph is replayed under the
profiler; `--kernels` lists the head's launches of that trace: head_score_kernel + head_score_combine_kernel against the head GEMM (the kernel in
front of score_rows_kernel on the stream) + score_rows_kernel."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernels(path):
    """the scoring head's launches in a rocprofv3 kernel trace, in stream order, microseconds: every score_rows_kernel with the kernel in front of
    it (the head GEMM), every head_score_kernel with the kernel behind it (its combine)"""
    with open(path) as f:
        rows = sorted((r for r in csv.DictReader(f) if "copyBuffer" not in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))   # no copy kernels
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    blocks = lambda r: int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))
    out = []
    for i, r in enumerate(rows):
        if "score_rows_kernel" in r["Kernel_Name"]:
            g = rows[i - 1]
            out.append({"path": "plain", "rows": blocks(r), "head": g["Kernel_Name"].split("(")[0], "head_blocks": blocks(g), "head_us": us(g),
                        "score_rows_us": us(r), "total_us": us(g) + us(r)})
        elif "head_score_kernel" in r["Kernel_Name"]:
            c = rows[i + 1]
            out.append({"path": "fused", "rows": blocks(c) * 4, "head": r["Kernel_Name"].split("(")[0], "head_blocks": blocks(r), "head_us": us(r),
                        "combine_us": us(c), "total_us": us(r) + us(c)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chunks", default="2048,256")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernels", default=None)
    a = ap.parse_args()
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))
    if a.kernels:
        res["kernel_trace_us"] = kernels(a.kernels)
    else:
        from ai00_server_amd import runtime as rt
        from oracle import rwkv_ref as R
        st, tensors = R.synth_st("v6-3b", fast=True)
        info = R.model_info(tensors)
        del tensors
        V, B = info.num_vocab, 32
        one = [[t % V for t in R.synth_prompt(1900, 2048)]] + [[]] * (B - 1)
        many = [[t % V for t in R.synth_prompt(1900 + b, 64)] for b in range(B)]
        res.update({"workload": "v6-3b", "quant": "int8", "num_vocab": V, "regions": a.regions, "requests_per_region": a.reps, "steps": {}})
        for chunk in [int(c) for c in a.chunks.split(",")]:
            if a.trace:                                             # one step per request: the first `chunk` rows of either workload
                one, many = [one[0][:chunk]] + [[]] * (B - 1), many[:chunk // 64] + [[]] * (B - chunk // 64)
            eng = rt.ModelBuilder(st).quant(info.num_layer, rt.Quant.Int8).build(max_batch=B, token_chunk_size=chunk, precision=rt.Precision.Fp16)
            zero = eng.state.init()

            def request(prompts, entry):
                for b, p in enumerate(prompts):
                    if p:
                        eng.state.load(zero, b)
                inp = rt.RnnInput([rt.RnnInputBatch(list(p), rt.RnnOption.Full) for p in prompts])
                tg, calls, acc = [(p[1:] + [rt.SCORE_SKIP]) if p else None for p in prompts], 0, 0.0
                t = time.perf_counter()
                while inp.num_token() > 0:
                    inp, tg, scores = entry(inp, tg)
                    calls += 1
                    acc += sum(float(s[:-1].sum()) for s in scores if len(s))
                return time.perf_counter() - t, calls, acc

            for wname, prompts in (("one_2048", one), ("32x64", many)):
                paths = {"plain": eng.infer_score, "fused": eng.infer_score_fused}
                times, calls, sums = {k: [] for k in paths}, 0, {}
                for k, f in paths.items():                          # warm-up, untimed; under --trace the only run
                    _, calls, sums[k] = request(prompts, f)
                    if not a.trace:
                        request(prompts, f)
                for _ in range(0 if a.trace else a.regions):
                    for k, f in paths.items():
                        times[k].append(sum(request(prompts, f)[0] for _ in range(a.reps)) / (a.reps * calls))
                row = {"steps_per_request": calls, "rows_per_step": sum(len(p) for p in prompts) // calls, "sum_logp": sums}
                if not a.trace:
                    row["seconds_per_step_median"] = {k: statistics.median(v) for k, v in times.items()}
                    row["seconds_per_step_min_max"] = {k: [min(v), max(v)] for k, v in times.items()}
                    row["fused_over_plain"] = row["seconds_per_step_median"]["fused"] / row["seconds_per_step_median"]["plain"]
                res["steps"][f"chunk{chunk}/{wname}"] = row
                print(json.dumps({f"chunk{chunk}/{wname}": row}), flush=True)
            eng.close()
    if a.out and not a.trace:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Per-step time of `rwkv_infer_topn_fused` against `rwkv_infer_topn`, one engine, one process:

    python scripts/topn_fused_bench.py [--out profiles/r20_topn_fused.json] [--chunks 2048,256] [--ns 5,32] [--regions 5] [--reps 4]

Workload: synthetic RWKV-V6-3B, Int8 on every layer, default precision, 32 slots; per token_chunk_size one 2048-token prompt (2048- resp. 256-row
steps) and, at chunk 256, 32 prompts of 64 tokens; every row is listed (`Full`) and scored against the next token.  A region is `--reps` whole
requests from the initial state under a host clock; every call ends in a device synchronise.  Each path is warmed with two untimed requests (graphs
captured, the list workspace allocated), the timed regions of the two paths alternate, medians and spreads are reported, per step = per call of
the entry point.  The logits of this model have no structure: the monotone worst case of the selection is not part of this workload."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chunks", default="2048,256")
    ap.add_argument("--ns", default="5,32")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    a = ap.parse_args()
    from ai00_server_amd import runtime as rt
    from oracle import rwkv_ref as R
    st, tensors = R.synth_st("v6-3b", fast=True)
    info = R.model_info(tensors)
    del tensors
    V, B = info.num_vocab, 32
    one = [[t % V for t in R.synth_prompt(2000, 2048)]] + [[]] * (B - 1)
    many = [[t % V for t in R.synth_prompt(2000 + b, 64)] for b in range(B)]
    res = {"workload": "v6-3b", "quant": "int8", "num_vocab": V, "regions": a.regions, "requests_per_region": a.reps, "steps": {}}
    for chunk in [int(c) for c in a.chunks.split(",")]:
        eng = rt.ModelBuilder(st).quant(info.num_layer, rt.Quant.Int8).build(max_batch=B, token_chunk_size=chunk, precision=rt.Precision.Fp16)
        zero = eng.state.init()

        def request(prompts, entry, n):
            for b, p in enumerate(prompts):
                if p:
                    eng.state.load(zero, b)
            inp = rt.RnnInput([rt.RnnInputBatch(list(p), rt.RnnOption.Full) for p in prompts])
            tg, calls, acc = [(p[1:] + [rt.SCORE_SKIP]) if p else None for p in prompts], 0, 0
            t = time.perf_counter()
            while inp.num_token() > 0:
                inp, tg, lists = entry(inp, n, tg)
                calls += 1
                acc += sum(int(o[0][:, 0].astype("int64").sum()) for o in lists if o is not None)
            return time.perf_counter() - t, calls, acc

        for wname, prompts in (("one_2048", one),) + ((("32x64", many),) if chunk < 2048 else ()):
            for n in [int(x) for x in a.ns.split(",")]:
                paths = {"plain": eng.infer_topn, "fused": eng.infer_topn_fused}
                times, calls, sums = {k: [] for k in paths}, 0, {}
                for k, f in paths.items():
                    request(prompts, f, n)
                    _, calls, sums[k] = request(prompts, f, n)
                for _ in range(a.regions):
                    for k, f in paths.items():
                        times[k].append(sum(request(prompts, f, n)[0] for _ in range(a.reps)) / (a.reps * calls))
                med = {k: statistics.median(v) for k, v in times.items()}
                row = {"steps_per_request": calls, "rows_per_step": sum(len(p) for p in prompts) // calls, "sum_of_top1_ids": sums,
                       "seconds_per_step_median": med, "seconds_per_step_min_max": {k: [min(v), max(v)] for k, v in times.items()},
                       "fused_over_plain": med["fused"] / med["plain"]}
                res["steps"][f"chunk{chunk}/{wname}/n{n}"] = row
                print(json.dumps({f"chunk{chunk}/{wname}/n{n}": row}), flush=True)
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

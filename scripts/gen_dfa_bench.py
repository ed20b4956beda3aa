"""What a byte-automaton constraint costs and buys in resident generation (rwkv_gen_set_constraint).

    python scripts/gen_dfa_bench.py [--out profiles/gen_dfa.json] [--tokens 128] [--steps-per-run 32] [--regions 5] [--batches 32,1]

Workload: synthetic RWKV-V6-3B, Int8 on every layer, default precision, V = 65,536, the World vocabulary as the token table, Nucleus with
the reference defaults, and a JSON-object automaton that loops (one object per line), so that a slot never halts inside a region.  Three
loops on one engine, alternating, region 0 dropped, medians with the spread:
  resident          rwkv_gen_run with no constraint (the step as it was)
  resident_dfa      rwkv_gen_run with the constraint on every slot (gen_mask_kernel in every step)
  per_token_dfa     what such a request had to do before: rwkv_infer_sample per token with an `allow` mask per slot from rwkv_dfa_allow and
                    `harness.DfaFormatter.update` on the host (driven from Python: the interpreter's share is in it)
`--loops resident_dfa --tokens 32 --regions 1` is the shape to put under a kernel trace for gen_mask_kernel's own time."""
import argparse
import json
import lzma
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ai00_server_amd import harness as H  # noqa: E402
from ai00_server_amd import runtime as rt  # noqa: E402
from oracle import rwkv_ref as R  # noqa: E402

PATTERN = rb'(\{"name":"[A-Za-z ]{1,40}","age":\d{1,3},"ok":(true|false)\}\n)*'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--workload", default="v6-3b")
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--steps-per-run", type=int, default=32)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--loops", default="resident,resident_dfa,per_token_dfa")
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    B = max(batches)
    st, tensors = R.synth_st(a.workload, fast=True)
    info = R.model_info(tensors)
    del tensors
    eng = rt.ModelBuilder(st).quant(info.num_layer, rt.Quant.Int8).build(max_batch=B, token_chunk_size=max(128, B), precision=rt.Precision.Fp16)
    V = info.num_vocab
    raw = lzma.open(os.path.join(ROOT, "tests", "golden", "rwkv_vocab_v20230424.json.xz"), "rt", encoding="utf-8").read()
    vocab = {int(k): (v.encode("utf-8") if isinstance(v, str) else bytes(v)) for k, v in json.loads(raw).items()}
    tab = [vocab.get(i) for i in range(max(vocab) + 1)]
    eng.gen_set_token_bytes(tab)
    dfa = rt.Dfa.compile(PATTERN)
    first = [t % V for t in R.synth_prompt(900, B)]
    n, spr = a.tokens, a.steps_per_run

    def resident(nb, constrained=False):
        for b in range(nb):
            eng.gen_arm(b, first[b], n, H.NucleusSampler(), seed=1)
            if constrained:
                eng.gen_set_constraint(b, dfa)
        emitted = 0
        t = time.perf_counter()
        for _ in range(-(-n // spr)):
            _, _, ne, _ = eng.gen_run(spr)
            emitted += int(ne.sum())
        dt = time.perf_counter() - t
        for b in range(nb):
            eng.gen_disarm(b)
        return dt, emitted

    def per_token_dfa(nb):
        smp = [H.NucleusSampler() if b < nb else None for b in range(B)]
        fms = [H.DfaFormatter(dfa, tab, V) for _ in range(nb)]
        cur = list(first)
        t = time.perf_counter()
        for s in range(n):
            for b in range(nb):
                smp[b].allow = fms[b].transform()
            inp = rt.RnnInput([rt.RnnInputBatch([cur[b]] if b < nb else []) for b in range(B)])
            us = rt.gen_uniform(1, 0, s * B, B)
            _, res = eng.infer_sample(inp, smp, [float(u) for u in us])
            for b in range(nb):
                cur[b] = res[b][0]
                smp[b].update(cur[b])
                fms[b].update(cur[b])
        return time.perf_counter() - t, nb * n

    loops = {"resident": resident, "resident_dfa": lambda nb: resident(nb, True), "per_token_dfa": per_token_dfa}
    loops = {k: f for k, f in loops.items() if k in a.loops.split(",")}
    out = {"workload": f"RWKV-{a.workload} int8, default precision, synthetic weights, V {V}", "pattern": PATTERN.decode(), "dfa_states": dfa.num_states,
           "token_table": "World vocabulary, %d entries" % len(tab), "tokens_per_slot_per_region": n, "steps_per_gen_run": spr, "regions": a.regions, "batches": {}}
    for nb in batches:
        times = {k: [] for k in loops}
        for rep in range(a.regions + 1):
            for k, f in loops.items():
                r = f(nb)
                if rep:
                    times[k].append(r)
        res = {}
        for k, v in times.items():
            rates = [tok / dt for dt, tok in v]
            res[k] = {"tokens_per_s": statistics.median(rates), "ms_per_step": statistics.median([dt / n * 1e3 for dt, _ in v]),
                      "tokens_per_s_min": min(rates), "tokens_per_s_max": max(rates), "spread_pct": 100.0 * (max(rates) - min(rates)) / statistics.median(rates),
                      "tokens_per_region": [tok for _, tok in v]}
        out["batches"][str(nb)] = res
    eng.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

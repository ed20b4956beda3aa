"""Cost of a wide sampler row (sample_wide_kernel): microseconds per launch on 32 rows of the bench model's logits, from a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python scripts/sample_wide_cost.py run
    python scripts/sample_wide_cost.py parse OUT [--json FILE]

`run` builds the bench model (synthetic RWKV-V6-3B, Int8 on every layer, default precision, 32 slots) and makes, in this order, 6 calls
of rwkv_infer_sample per case with 32 rows each, then 24 resident steps:
  narrow_miro  Mirostat max_surprise 12.5: nucleus_kernel<8192> (the same 8192-entry sort)
  a            Nucleus top_k 1000, top_p 0.5: ends in window 0
  b            Nucleus top_k num_vocab, top_p 1.0: every window, both passes
  c            Mirostat max_surprise 16
  d            rwkv_gen_run, one wide slot (Mirostat target 4.5) among 32 default Nucleus slots
`parse` reads the trace's *kernel_trace.csv, takes the sampler launches in time order and assigns them to the cases by that order (the
wide launches: 6 x a, 6 x b, 6 x c, the rest d).  The trace run collects no counters.  profiles/r8_sample_wide.json holds a result."""
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import numpy as np
    from ai00_server_amd import harness as H, runtime as rt
    from oracle import rwkv_ref as R
    B, REPS = 32, 6
    st, tensors = R.synth_st("v6-3b", fast=True)
    info = R.model_info(tensors); del tensors
    eng = rt.ModelBuilder(st).quant(info.num_layer, rt.Quant.Int8).build(max_batch=B, token_chunk_size=128, precision=rt.Precision.Fp16)
    V = info.num_vocab
    first = [t % V for t in R.synth_prompt(900, B)]
    def miro(ms):
        s = H.MirostatSampler(); s.max_surprise = np.float32(ms); return s
    def nuc(k, p):
        return H.NucleusSampler(top_p=p, top_k=k, presence_penalty=0.0, frequency_penalty=0.0)
    phases = [("narrow_miro", lambda: miro(12.5)), ("a", lambda: nuc(1000, 0.5)), ("b", lambda: nuc(V, 1.0)), ("c", lambda: miro(16.0))]
    out = {}
    for name, mk in phases:
        smp = [mk() for _ in range(B)]
        t = []
        for r in range(REPS):
            us = [float(u) for u in rt.gen_uniform(7, r, 0, B)]
            inp = rt.RnnInput([rt.RnnInputBatch([first[b]]) for b in range(B)])
            t0 = time.perf_counter(); eng.infer_sample(inp, smp, us); t.append(time.perf_counter() - t0)
        out[name] = {"launches": REPS, "host_ms_per_call_median": 1e3 * float(np.median(t))}
        print("PHASE", name, REPS, flush=True)
    for b in range(B):
        eng.gen_arm(b, first[b], 64, H.MirostatSampler(tau=4.5) if b == 0 else H.NucleusSampler(), seed=1)
    t0 = time.perf_counter(); _, _, ne, _ = eng.gen_run(24); dt = time.perf_counter() - t0
    out["d"] = {"launches": 24, "host_ms_per_step": 1e3 * dt / 24, "emitted": int(ne.sum())}
    print("PHASE d 24", flush=True)
    eng.close()
    print(json.dumps(out))



def parse(out_dir, json_path=None):
    f = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    samp = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows
            if "nucleus_kernel" in r["Kernel_Name"] or "sample_wide_kernel" in r["Kernel_Name"]]
    wide = [t for k, t in samp if "sample_wide" in k]
    nm = [t for k, t in samp if "nucleus_kernel" in k and "8192" in k]
    nt = [t for k, t in samp if "nucleus_kernel" in k and "8192" not in k]
    med = lambda v: statistics.median(v) if v else None
    res = {"n_wide": len(wide), "n_narrow_miro": len(nm), "n_narrow_nt": len(nt),
           "narrow_miro_us": med(nm[0:6]), "a_us": med(wide[0:6]), "b_us": med(wide[6:12]), "c_us": med(wide[12:18]), "d_wide_us": med(wide[18:]),
           "narrow_miro_all": nm[0:6], "a_all": wide[0:6], "b_all": wide[6:12], "c_all": wide[12:18], "d_all": wide[18:],
           "resident_narrow_nt_us": med(nt[-24:]) if len(nt) >= 24 else None}
    print(json.dumps(res))
    if json_path:
        with open(json_path, "w") as o:
            json.dump(res, o, indent=1)
            o.write("\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "parse":
        parse(sys.argv[2], sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None)
    elif len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    else:
        sys.exit(__doc__)

"""Three decode loops on one engine in one process: device-resident greedy (rwkv_decode_greedy), the per-token sampled loop
(rwkv_infer_sample, one call per token) and device-resident sampled generation (rwkv_gen_arm / rwkv_gen_run).

    python scripts/gen_resident_bench.py [--out profiles/r7_gen_resident.json] [--tokens 256] [--steps-per-run 32] [--regions 5]

Workload: synthetic RWKV-V6-3B, Int8 on every layer, default precision, 32 slots and 1 slot, Nucleus with the reference defaults
(sampler/nucleus.rs:13-26), `--tokens` tokens per slot per timed region.  Every loop is warmed with one untimed region (graphs
captured, code objects loaded); the `--regions` timed regions of the loops alternate, so that drift of the machine hits all of them
alike; each region is a host clock around work that ends in a device synchronise; the median is reported with the spread.

The per-token loop is timed twice: `sample_bare` is Runtime.serve_loop_sample — no penalty map at all, every per-step Python object
hoisted out: the LEAST the per-token path can cost and the yardstick the resident loop is held to — and `sample_host_samplers` is
the same call driven by harness.NucleusSampler objects (penalty maps on the host, adjustment lists per token), which includes the
Python interpreter's share and is reported for orientation only.  The resident loop always carries the penalty state machine.
Token 0 stops a resident slot (run.rs:855), so its rate counts the tokens really emitted.

`--loops resident` times the resident loop alone (the decode-only regression guard: run it on two builds, alternating, with
RWKV_HIP_LIB-less checkouts side by side).  `--admission` adds the admission scenario: 24 slots generate, every 16 steps one of the
other 8 slots receives a 256-token prompt and then generates; (a) `leave_and_prefill` is the sequence of ABI 8 (leave the run,
rwkv_infer_sample prefill, host sampler update, rwkv_gen_arm, re-enter), (b) `arm_prompt` is rwkv_gen_arm_prompt (ABI 9).  Reported for
both, by the host clock: tokens/s over the region; the time from the admission to the joiner's first token being in the host's hands;
and the longest gap between two tokens of a running slot: for (a) the time between the two runs around an admission plus one step, for
(b) the longest single-step run while a prompt is being consumed (rwkv_gen_run(1) per step during an admission, so that every step
is timed on its own).

`--stops N,LEN` gives every slot of the resident loop N stop strings of LEN bytes that never match, over a synthetic token table (ids map
to 1-4 letters): the price of matching stop strings on the device (rwkv_gen_set_stops).  `--loops resident_1` is what a caller with stop
strings had to do before: rwkv_gen_run(1) per token and `harness.StopMatcher` over every slot's token on the host.

`--watch` adds the loop `resident_watch`: the resident loop with a watch open (rwkv_gen_watch_open; every step publishes its record into
host memory and loads the slots' cancel words) and a reader thread that drains it while the run goes on.  Its regions alternate with
`resident`'s in the same process; the result also carries `resident_watch_vs_resident` and the records the reader got and lost.

`--capture` adds the loop `resident_capture`: the resident loop with RWKV_GEN_CAPTURE_FINISH set on every slot (rwkv_gen_set_capture; one
more launch per step that copies each running slot's raw row aside).  Its regions alternate with `resident`'s in the same process; the
result also carries `resident_capture_vs_resident`."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ai00_server_amd import harness as H  # noqa: E402
from ai00_server_amd import runtime as rt  # noqa: E402
from oracle import rwkv_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--workload", default="v6-3b")
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--steps-per-run", type=int, default=32)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--loops", default="greedy,sample_bare,sample_host_samplers,resident")
    ap.add_argument("--admission", action="store_true")
    ap.add_argument("--stops", default=None, help="N,LEN: every resident slot carries N never-matching stop strings of LEN bytes")
    ap.add_argument("--top", type=int, default=0, help="N: adds the loop resident_top, the resident loop with every slot listing its N most likely tokens")
    ap.add_argument("--watch", action="store_true", help="adds the loop resident_watch: the resident loop with a watch open and a reader thread draining it")
    ap.add_argument("--capture", action="store_true", help="adds the loop resident_capture: the resident loop with every slot capturing its FINISH item")
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    B = max(batches)
    st, tensors = R.synth_st(a.workload, fast=True)
    info = R.model_info(tensors)
    del tensors
    t0 = time.time()
    eng = rt.ModelBuilder(st).quant(info.num_layer, rt.Quant.Int8).build(max_batch=B, token_chunk_size=max(128, B), precision=rt.Precision.Fp16)
    load_s = time.time() - t0
    V = info.num_vocab
    first = [t % V for t in R.synth_prompt(900, B)]
    n, spr = a.tokens, a.steps_per_run
    n_stops, stop_len = (int(x) for x in a.stops.split(",")) if a.stops else (0, 0)
    stops = [bytes([122]) * (stop_len - 1) + bytes([48 + i]) for i in range(n_stops)]      # "zzz…0": the table below has no z
    trng = np.random.default_rng(3)
    tab = [bytes(trng.integers(97, 103, int(trng.integers(1, 5))).tolist()) for _ in range(V)]
    if n_stops or "resident_1" in a.loops.split(","):
        eng.gen_set_token_bytes(tab)

    def greedy(nb):
        t = time.perf_counter()
        eng.decode_greedy(first[:nb], n)
        return time.perf_counter() - t, nb * n

    def sample_bare(nb):
        return eng.serve_loop_sample(first[:nb], n), nb * n

    def sample_host(nb):
        smp = [H.NucleusSampler() if b < nb else None for b in range(B)]
        cur = list(first)
        t = time.perf_counter()
        for s in range(n):
            inp = rt.RnnInput([rt.RnnInputBatch([cur[b]] if b < nb else []) for b in range(B)])
            us = rt.gen_uniform(1, 0, s * B, B)
            _, res = eng.infer_sample(inp, smp, [float(u) for u in us])
            for b in range(nb):
                cur[b] = res[b][0]
                smp[b].update(cur[b])
        return time.perf_counter() - t, nb * n

    arm_s = {}

    watch_stats = {}

    def resident(nb, top=0, watch=False, capture=False):
        w = stop = reader = None
        if watch:                                                    # opened and closed outside the timed region, like the arming
            w, stop, got = eng.gen_watch_open(4096), threading.Event(), watch_stats.setdefault(nb, {"records": 0, "lost": 0})

            def drain():
                while True:
                    done = stop.is_set()
                    t_, _, _, lost = w.read(256)
                    got["records"] += len(t_)
                    got["lost"] += lost
                    if not len(t_):
                        if done:
                            return
                        time.sleep(0.0002)

            reader = threading.Thread(target=drain, daemon=True)
            reader.start()
        t = time.perf_counter()
        for b in range(nb):
            eng.gen_arm(b, first[b], n, H.NucleusSampler(), seed=1)
        if not top:
            arm_s.setdefault(nb, []).append(time.perf_counter() - t)
        for b in range(nb if top else 0):
            eng.gen_set_topn(b, top)                                # re-arming resets it: the plain loop's slots list nothing
        for b in range(nb if n_stops else 0):
            eng.gen_set_stops(b, stops)
        for b in range(nb if capture else 0):
            eng.gen_set_capture(b, rt.GenCapture.Finish)            # re-arming resets it, and drops the item the region before left untaken
        emitted = 0
        t = time.perf_counter()
        for _ in range(-(-n // spr)):
            ne = eng.gen_run(spr, top=top)[2]
            emitted += int(ne.sum())
        dt = time.perf_counter() - t
        if watch:
            stop.set()
            reader.join()
            w.close()
        for b in range(nb if n_stops else 0):
            eng.gen_disarm(b)                                       # the next loop's slots carry no strings
        return dt, emitted

    def resident_1(nb):
        """the only exact form without device stop strings: one rwkv_gen_run(1) per token, the host matcher over every slot's token"""
        hs = stops or [b"zzzzzzzzzzzzzzz0"]
        for b in range(nb):
            eng.gen_arm(b, first[b], n, H.NucleusSampler(), seed=1)
        ms = [H.StopMatcher(hs) for _ in range(nb)]
        emitted = 0
        t = time.perf_counter()
        for _ in range(n):
            toks, _, ne, fin = eng.gen_run(1)
            emitted += int(ne.sum())
            for b in range(nb):
                if toks[0, b] != 0xFFFFFFFF:
                    ms[b].push(tab[int(toks[0, b])])
        return time.perf_counter() - t, emitted

    loops = {"greedy": greedy, "sample_bare": sample_bare, "sample_host_samplers": sample_host, "resident": resident, "resident_1": resident_1}
    loops = {k: f for k, f in loops.items() if k in a.loops.split(",")}
    if a.top and "resident" in loops:
        loops["resident_top"] = lambda nb: resident(nb, a.top)
    if a.watch and "resident" in loops:
        loops["resident_watch"] = lambda nb: resident(nb, watch=True)
    if a.capture and "resident" in loops:
        loops["resident_capture"] = lambda nb: resident(nb, capture=True)

    def admission(mode, running=24, joiners=8, every=16, plen=256, tail=4):
        """One region.  Both modes call gen_run(every) while nobody is being admitted.  `leave_and_prefill` admits between two runs with
        existing calls; the running slots' gap there is the host time between the two runs plus one step.  `arm_prompt` arms the prompt
        and then calls gen_run(1) until the joiner's first token is out, each call timed: a running slot emits one token per call, so
        the longest such call IS its longest gap (it includes the per-call read-back a longer run would not pay).
        Returns (seconds, tokens emitted, [first-token latency per joiner], longest running-slot gap, mixed steps per admission)."""
        for b in range(running):
            eng.gen_arm(b, first[b], 1 << 20, H.NucleusSampler(), seed=1)
        prompts = [[t % V for t in R.synth_prompt(950 + j, plen)] for j in range(joiners)]
        emitted, lat, plain, gaps, mixed = 0, [], [], [], []
        t_region = time.perf_counter()
        for r in range(joiners + tail):
            t0 = time.perf_counter()
            _, _, ne, _ = eng.gen_run(every)
            t1 = time.perf_counter()
            emitted += int(ne.sum())
            plain.append((t1 - t0) / every)
            if r >= joiners:
                continue
            slot, q = running + r, prompts[r]
            smp = H.NucleusSampler()
            smp.init(q)
            ta = time.perf_counter()
            if mode == "arm_prompt":
                eng.gen_arm_prompt(slot, q, 1 << 20, smp, seed=1)
                n = 0
                while True:
                    tg = time.perf_counter()
                    toks, _, ne, _ = eng.gen_run(1)
                    te = time.perf_counter()
                    emitted += int(ne.sum())
                    gaps.append(te - tg)
                    n += 1
                    if toks[0, slot] != 0xFFFFFFFF:
                        break
                lat.append(te - ta)
                mixed.append(n)
            else:
                inp = rt.RnnInput([rt.RnnInputBatch(list(q) if b == slot else []) for b in range(B)])
                sm = [smp if b == slot else None for b in range(B)]
                us = [rt.gen_uniform(1, slot, 0) if b == slot else 0.0 for b in range(B)]
                res, n = None, 0
                while inp.num_token() > 0:
                    inp, out_ = eng.infer_sample(inp, sm, us)
                    res = out_[slot] or res
                    n += 1
                lat.append(time.perf_counter() - ta)
                emitted += 1
                smp.update(res[0])
                eng.gen_arm(slot, res[0], 1 << 20, smp, seed=1)
                gaps.append(time.perf_counter() - t1 + statistics.median(plain))
                mixed.append(n)
        dt = time.perf_counter() - t_region
        for b in range(B):
            eng.gen_disarm(b)
        return dt, emitted, lat, max(gaps), max(mixed)

    out = {"workload": f"RWKV-{a.workload} int8, default precision, synthetic weights", "tokens_per_slot_per_region": n, "steps_per_gen_run": spr,
           "regions": a.regions, "load_s": load_s, "stop_strings_per_slot": n_stops, "stop_string_bytes": stop_len, "sampler": "Nucleus top_p 0.5 top_k 128 temperature 1.0 penalties 0.3 / 0.3 / 0.99654026",
           "batches": {}}
    for nb in batches:
        times = {k: [] for k in loops}
        for rep in range(a.regions + 1):                       # region 0 warms every loop and is dropped
            for k, f in loops.items():
                dt, tokens = f(nb)
                if rep:
                    times[k].append((dt, tokens))
        res = {}
        for k, v in times.items():
            rates = [tok / dt for dt, tok in v]
            steps = [dt / n * 1e3 for dt, _ in v]
            res[k] = {"tokens_per_s": statistics.median(rates), "ms_per_step": statistics.median(steps),
                      "tokens_per_s_min": min(rates), "tokens_per_s_max": max(rates),
                      "spread_pct": 100.0 * (max(rates) - min(rates)) / statistics.median(rates), "tokens_per_region": [tok for _, tok in v]}
        if "resident" in res:
            res["resident"]["arm_ms_per_slot"] = 1e3 * statistics.median(arm_s[nb]) / nb
            for other in ("sample_bare", "greedy"):
                if other in res:
                    res["resident_vs_" + other] = res["resident"]["tokens_per_s"] / res[other]["tokens_per_s"]
        if "resident_watch" in res and "resident" in res:
            res["resident_watch_vs_resident"] = res["resident_watch"]["tokens_per_s"] / res["resident"]["tokens_per_s"]
            res["resident_watch"].update(watch_stats.get(nb, {}))   # over all regions, the warm-up included
        if "resident_capture" in res and "resident" in res:
            res["resident_capture_vs_resident"] = res["resident_capture"]["tokens_per_s"] / res["resident"]["tokens_per_s"]
        out["batches"][str(nb)] = res
    if a.admission:
        adm = {}
        modes = ("leave_and_prefill", "arm_prompt")
        runs = {m: [] for m in modes}
        for rep_ in range(a.regions + 1):                          # region 0 warms both and is dropped; the two alternate
            for m in modes:
                r = admission(m)
                if rep_:
                    runs[m].append(r)
        for m in modes:
            rates = [tok / dt for dt, tok, _, _, _ in runs[m]]
            lats = [statistics.median(l) * 1e3 for _, _, l, _, _ in runs[m]]
            gaps = [g * 1e3 for _, _, _, g, _ in runs[m]]
            sp = lambda v: 100.0 * (max(v) - min(v)) / statistics.median(v)
            adm[m] = {"tokens_per_s": statistics.median(rates), "tokens_per_s_spread_pct": sp(rates),
                      "first_token_ms": statistics.median(lats), "first_token_ms_spread_pct": sp(lats),
                      "longest_running_gap_ms": statistics.median(gaps), "longest_running_gap_ms_spread_pct": sp(gaps),
                      "steps_per_admission": runs[m][0][4]}
        adm["scenario"] = ("24 slots generating, every 16 steps one of 8 more slots gets a 256-token prompt; gen_run(16) per call, "
                           "gen_run(1) per step while arm_prompt consumes a prompt; token_chunk_size %d" % eng.token_chunk_size)
        out["admission"] = adm
    eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

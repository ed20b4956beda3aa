"""Dev tool (GPU box): NF4 against SF4 on the same isolated GEMM launches (rwkv_bench_gemm, fmt 2 against fmt 3), alternating within one
process, on the matrix shapes of V7-2.9B (C = 2560, F = 10240) at 1, 32 and 2048 rows.  One JSON line per (shape, rows) with every repeat's
microseconds per launch for both formats, their medians, the ratio of the medians and the spread between repeats of the SAME format — a
difference inside that spread is none.

    python scripts/sf4_ab.py [--repeats 5] [--out profiles/<name>.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ai00_server_amd import runtime as rt  # noqa: E402

C, F = 2560, 10240
SHAPES = [("att r/k/v/o", C, C), ("ffn.key", F, C), ("ffn.value", C, F)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name, rows, K in SHAPES:
        for T in (1, 32, 2048):
            iters = 200 if T <= 32 else 50
            us = {2: [], 3: []}
            rt.bench_gemm(rows, K, 2, T, iters=10)                    # code objects loaded, clocks up
            for _ in range(a.repeats):
                for fmt in (2, 3):
                    us[fmt].append(rt.bench_gemm(rows, K, fmt, T, iters=iters)[0])
            med = {f: statistics.median(v) for f, v in us.items()}
            spread = {f: (max(v) - min(v)) / med[f] for f, v in us.items()}
            d = {"matrix": name, "rows": rows, "K": K, "T": T, "iters": iters, "nf4_us": [round(x, 3) for x in us[2]], "sf4_us": [round(x, 3) for x in us[3]],
                 "nf4_median_us": round(med[2], 3), "sf4_median_us": round(med[3], 3), "sf4_over_nf4": round(med[3] / med[2], 4),
                 "nf4_spread": round(spread[2], 4), "sf4_spread": round(spread[3], 4)}
            print(json.dumps(d), flush=True)
            lines.append(d)
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

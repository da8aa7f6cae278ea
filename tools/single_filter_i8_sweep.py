#!/usr/bin/env python3
"""The single-query int8 filter on one GPU: launch shapes of k_scan_i8_qarg, and the int8 / bf16 crossover in index size.

  --what shapes     every k_scan_i8_qarg shape listed for the row stride (VL_SCAN8_SHAPE "G,VPL,U") x workgroups per CU
                    (VL_SCAN8_BPC), scan time per launch from HIP events, interleaved rounds in ONE process; the bf16
                    filter of the same index alongside.
  --what crossover  ONE index grown through --sizes: at each size, back-to-back single searches with the int8 filter
                    first ("i8") and with the bf16 filter first ("bf16"), interleaved rounds; per-search wall time.

One JSON object per line on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from single_filter_sweep import grow, queries, timed_launches  # noqa: E402

# int8 row stride / 16 -> the listed shapes (VL_I8_SCAN_SHAPES in mfma_scan.hip)
SHAPES = {8: ["4,2,1", "8,1,1"], 16: ["4,4,1", "8,2,1"], 24: ["4,6,1", "8,3,1", "8,3,2", "4,6,2", "2,12,1"],
          32: ["4,8,1", "8,4,1"], 48: ["8,6,1", "4,12,1", "16,3,1", "8,6,2"]}


def ldb_of(dim):
    return next(s for s in (128, 256, 384, 512, 768) if dim <= s)


def shapes(a, V, torch, dev):
    idx = V.FlatIndex(a.dim)
    idx.reserve(a.rows)
    grow(idx, torch, dev, a.dim, 0, a.rows)
    Q = queries(a.dim, 64)
    ldb = ldb_of(a.dim)
    i8_bytes = a.rows * (ldb + 8 + (4 if a.metric == 3 else 0))
    cands = [(s, b) for s in SHAPES[ldb // 16] for b in a.bpc.split(",")]
    res = {c: [] for c in cands}
    res_bf16 = []
    idx.set_single_filter("i8")
    idx.search_arrays(Q[0], 10, a.metric)  # builds the int8 copy
    idx.set_single_filter("bf16")
    idx.search_arrays(Q[0], 10, a.metric)
    for r in range(a.rounds):
        for s, b in cands:
            os.environ["VL_SCAN8_SHAPE"], os.environ["VL_SCAN8_BPC"] = s, b
            idx.set_single_filter("i8")
            timed_launches(idx, Q, a.metric, 3)
            ms, nl, ns = timed_launches(idx, Q, a.metric, a.per_round)
            res[(s, b)].append((ms, nl, ns, idx.last_scan()))
        idx.set_single_filter("bf16")
        timed_launches(idx, Q, a.metric, 3)
        res_bf16.append(timed_launches(idx, Q, a.metric, a.per_round)[0])
    os.environ.pop("VL_SCAN8_SHAPE")
    os.environ.pop("VL_SCAN8_BPC")
    for (s, b), v in res.items():
        med = statistics.median(x[0] for x in v)
        print(json.dumps({"what": "shape", "rows": a.rows, "dim": a.dim, "metric": a.metric, "shape_g_vpl_u": s, "bpc": int(b),
                          "variant": v[-1][3], "ms_per_launch_median": round(med, 4),
                          "ms_per_launch_rounds": [round(x[0], 4) for x in v],
                          "launches_per_search": round(sum(x[1] for x in v) / sum(x[2] for x in v), 3),
                          "GBps_on_i8_bytes": round(i8_bytes / (med * 1e-3) / 1e9, 1)}), flush=True)
    med = statistics.median(res_bf16)
    print(json.dumps({"what": "bf16_filter", "rows": a.rows, "dim": a.dim, "metric": a.metric, "variant": idx.last_scan(),
                      "ms_per_launch_median": round(med, 4), "ms_per_launch_rounds": [round(x, 4) for x in res_bf16],
                      "GBps": round(a.rows * ldb * 2 / (med * 1e-3) / 1e9, 1)}), flush=True)


def crossover(a, V, torch, dev):
    sizes = [int(x) for x in a.sizes.split(",")]
    idx = V.FlatIndex(a.dim)
    idx.reserve(sizes[-1])
    Q = queries(a.dim, 256)
    have = 0
    for n in sizes:
        grow(idx, torch, dev, a.dim, have, n)
        have = n
        wall = {"i8": [], "bf16": []}
        for mode in ("i8", "bf16"):  # warm: the copies' new rows, both code paths
            idx.set_single_filter(mode)
            for i in range(20):
                idx.search_arrays(Q[i], 10, a.metric)
        for r in range(a.rounds):
            for mode in ("bf16", "i8") if r % 2 == 0 else ("i8", "bf16"):
                idx.set_single_filter(mode)
                t = time.perf_counter()
                for i in range(a.per_round):
                    idx.search_arrays(Q[i % len(Q)], 10, a.metric)
                wall[mode].append((time.perf_counter() - t) / a.per_round * 1e3)
        i8, b = statistics.median(wall["i8"]), statistics.median(wall["bf16"])
        print(json.dumps({"what": "crossover_i8", "rows": n, "dim": a.dim, "metric": a.metric,
                          "f32_slab_MiB": round(n * ((a.dim + 3) // 4 * 4) * 4 / 2 ** 20, 1),
                          "ms_per_search_i8": round(i8, 4), "ms_per_search_bf16": round(b, 4), "i8_over_bf16": round(i8 / b, 3),
                          "rounds_i8": [round(x, 4) for x in wall["i8"]], "rounds_bf16": [round(x, 4) for x in wall["bf16"]]}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("shapes", "crossover"), required=True)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--metric", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--bpc", default="2,3,4")
    ap.add_argument("--sizes", default="100000,300000,700000,1000000,2000000,5000000,10000000")
    a = ap.parse_args()
    import torch
    import vectorlite_amd as V
    dev = torch.device("cuda", 0)
    {"shapes": shapes, "crossover": crossover}[a.what](a, V, torch, dev)


if __name__ == "__main__":
    main()

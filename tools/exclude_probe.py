"""Exclusion-filtered search on the headline index (10 M x 384 cosine unit rows by default): per exclusion set size (0, 100,
10 000, 1 M, 5 M random ids) the median per call of search(..., exclude=token), alternated query by query on ONE handle with
the unfiltered search and with the include filter of the complement; beside it the three masked kernels' times (each mode
forced in turn, HIP events around the scan), the token's creation (resolution) time, its re-resolution time after a
mutation, and the bytes it holds on the device (bitmap; position list once a list-route call asked for it).  One JSON line
per measurement on stdout and in profiles/exclude_<n>x<dim>.jsonl.

    python tools/exclude_probe.py [--rows 10000000] [--dim 384] [--queries 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ts):
    a = np.sort(np.asarray(ts) * 1e3)
    return {"median_ms": round(float(np.median(a)), 4), "p99_ms": round(float(a[min(len(a) - 1, int(0.99 * len(a)))]), 4),
            "mean_ms": round(float(a.mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--sets", default="0,100,10000,1000000,5000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim = args.rows, args.dim
    out_path = args.out or os.path.join(ROOT, "profiles", f"exclude_{n}x{dim}.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    fh = open(out_path, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        fh.write(line + "\n")
        fh.flush()

    os.environ.pop("VL_SINGLE_FILTER", None)
    idx = V.FlatIndex(dim)  # default ladder
    idx.reserve(n)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    step = 2_500_000
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        x = torch.randn((hi - lo, dim), dtype=torch.float64, device="cuda:0", generator=g)
        x /= torch.linalg.vector_norm(x, dim=1, keepdim=True)
        idx.add_rows(np.arange(lo, hi, dtype=np.uint64), x, validate=False)
        del x
    torch.cuda.synchronize()
    idx.set_coalescing(0)
    rng = np.random.default_rng(2)
    Q = rng.standard_normal((args.queries, dim))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    all_ids = np.arange(n, dtype=np.uint64)

    for size in [int(x) for x in args.sets.split(",")]:
        size = min(size, n)
        excluded = rng.choice(n, size=size, replace=False).astype(np.uint64) if size else np.zeros(0, np.uint64)
        t0 = time.perf_counter()
        fe = idx.make_filter(excluded, exclude=True)
        t_create = time.perf_counter() - t0
        t0 = time.perf_counter()
        complement = np.setdiff1d(all_ids, excluded, assume_unique=True)
        fi = idx.make_filter(complement)
        t_complement = time.perf_counter() - t0
        calls = {"exclude": lambda q: idx.search_arrays(q, 10, 0, exclude=fe),
                 "unfiltered": lambda q: idx.search_arrays(q, 10, 0),
                 "complement_include": lambda q: idx.search_arrays(q, 10, 0, filter=fi)}
        ts = {name: [] for name in calls}
        for q in Q[:20]:
            for fn in calls.values():
                fn(q)
        for q in Q:  # alternated query by query on the one handle
            for name, fn in calls.items():
                t0 = time.perf_counter()
                fn(q)
                ts[name].append(time.perf_counter() - t0)
        idx.search_arrays(Q[0], 10, 0, exclude=fe)
        path, scan = V.last_path(), idx.last_scan()
        med = {name: stats(t) for name, t in ts.items()}
        rec = {"what": "exclude", "rows": n, "dim": dim, "excluded_ids": size, "qualifying": fe.rows(), "k": 10,
               "create_ms": round(t_create * 1e3, 3), "complement_create_ms": round(t_complement * 1e3, 3),
               "path": path, "scan_variant": scan["variant"], "scan_grid": scan["grid"],
               "exclude": med["exclude"], "unfiltered": med["unfiltered"], "complement_include": med["complement_include"],
               "ratio_to_unfiltered": round(med["exclude"]["median_ms"] / med["unfiltered"]["median_ms"], 3),
               "ratio_to_complement_include": round(med["exclude"]["median_ms"] / med["complement_include"]["median_ms"], 3),
               # what the token holds on the device before any list-route call, and what such a call adds
               "token_bytes": {"ids": 8 * size, "chunk_offsets": 4 * 1025, "bitmap": 8 * ((n + 63) // 64)},
               "list_bytes_on_demand": 4 * (n - size), "complement_token_bytes": 8 * (n - size) + 4 * 1025 + 4 * (n - size)}
        # the three masked kernels, each mode forced in turn: HIP events around the scan launches
        for mode in ("i8", "bf16", "f32"):
            idx.set_single_filter(mode)
            for q in Q[:10]:
                idx.search_arrays(q, 10, 0, exclude=fe)
            idx.profile_read()
            idx.profile_enable(True)
            for q in Q[:50]:
                idx.search_arrays(q, 10, 0, exclude=fe)
            idx.profile_enable(False)
            nl, ms, by = idx.profile_read()
            if nl:
                rec["masked_" + mode] = {"launches_per_call": round(nl / 50, 2), "scan_ms": round(ms / nl, 4), "scan_bytes": by // nl,
                                         "scan_tb_s": round(by / (ms * 1e-3) / 1e12, 3) if ms > 0 else None,
                                         "scan_variant": idx.last_scan()["variant"]}
        idx.set_single_filter("auto")
        # re-resolution: one mutation, then the next use resolves the token again
        idx.add_rows(np.array([n + 1], dtype=np.uint64), Q[:1], validate=False)
        t0 = time.perf_counter()
        fe.rows()
        rec["reresolve_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        idx.delete(n + 1)
        emit(rec)
        fe.close()
        fi.close()
    fh.close()


if __name__ == "__main__":
    main()

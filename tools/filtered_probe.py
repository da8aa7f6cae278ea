"""Id-filtered search on the headline index (10 M x 384 cosine unit rows by default): per subset size and shape (random
ids / one contiguous run), filter creation time, re-resolution time after a mutation, and median / p99 ms per filtered
search (k = 10) over --queries queries after warm-up; beside them the unfiltered search with the f32 scan only
(VL_SINGLE_FILTER=f32) and with the default ladder, alternated query by query.  One JSON line per measurement on stdout
and in profiles/filtered_<n>x<dim>.jsonl.

    python tools/filtered_probe.py [--rows 10000000] [--dim 384] [--queries 200]
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
    ap.add_argument("--fractions", default="0.0001,0.001,0.01,0.1,0.5,1.0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim = args.rows, args.dim
    out_path = args.out or os.path.join(ROOT, "profiles", f"filtered_{n}x{dim}.jsonl")
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

    def timed(fn):
        for q in Q[:20]:
            fn(q)
        ts = []
        for q in Q:
            t0 = time.perf_counter()
            fn(q)
            ts.append(time.perf_counter() - t0)
        return ts

    # the unfiltered baselines, alternated query by query
    f32_ts, auto_ts = [], []
    for q in Q[:20]:
        idx.set_single_filter("f32")
        idx.search_arrays(q, 10, 0)
        idx.set_single_filter("auto")
        idx.search_arrays(q, 10, 0)
    for q in Q:
        idx.set_single_filter("f32")
        t0 = time.perf_counter()
        idx.search_arrays(q, 10, 0)
        f32_ts.append(time.perf_counter() - t0)
        idx.set_single_filter("auto")
        t0 = time.perf_counter()
        idx.search_arrays(q, 10, 0)
        auto_ts.append(time.perf_counter() - t0)
    emit({"what": "unfiltered", "single_filter": "f32", "rows": n, "dim": dim, **stats(f32_ts)})
    emit({"what": "unfiltered", "single_filter": "auto", "rows": n, "dim": dim, **stats(auto_ts)})

    for frac in [float(x) for x in args.fractions.split(",")]:
        m = max(1, int(round(n * frac)))
        for shape in ("random", "contiguous"):
            if shape == "random":
                keep = rng.choice(n, size=m, replace=False).astype(np.uint64)
            else:
                lo = int(rng.integers(0, n - m + 1))
                keep = np.arange(lo, lo + m, dtype=np.uint64)
            t0 = time.perf_counter()
            f = idx.make_filter(keep)
            t_create = time.perf_counter() - t0
            ts = timed(lambda q: idx.search_arrays(q, 10, 0, filter=f))
            idx.search_arrays(Q[0], 10, 0, filter=f)
            path, scan = V.last_path(), idx.last_scan()
            idx.profile_read()
            idx.profile_enable(True)
            for q in Q[:50]:
                idx.search_arrays(q, 10, 0, filter=f)
            idx.profile_enable(False)
            nl, ms, by = idx.profile_read()
            # re-resolution: one mutation outside the subset, then the next search resolves the filter again
            idx.add_rows(np.array([n + 1], dtype=np.uint64), Q[:1], validate=False)
            t0 = time.perf_counter()
            rows = f.rows()
            t_resolve = time.perf_counter() - t0
            idx.delete(n + 1)
            f.rows()
            rec = {"what": "filtered", "rows": n, "dim": dim, "fraction": frac, "subset_rows": m, "shape": shape, "k": 10,
                   "create_ms": round(t_create * 1e3, 3), "reresolve_ms": round(t_resolve * 1e3, 3), "qualifying": rows,
                   "path": path, "scan_variant": scan["variant"], "scan_grid": scan["grid"], **stats(ts)}
            if nl:
                rec["scan_ms"] = round(ms / nl, 4)
                rec["scan_bytes"] = by // nl
                rec["scan_tb_s"] = round(by / (ms * 1e-3) / 1e12, 3) if ms > 0 else None
            emit(rec)
            f.close()
    fh.close()


if __name__ == "__main__":
    main()

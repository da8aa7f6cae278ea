"""Diversified (MMR) search on the headline index (10 M x 384 cosine unit rows by default): for (k, fetch_k) in
(4, 20), (10, 60), (10, 256), (64, 1024) the median ms per call of search_mmr_arrays, alternated call by call with the
yardstick -- search_arrays(q, fetch_k) on the same handle, the unchanged path -- and their difference, the cost of the MMR
tail; the same over 1 % and 10 % id filters; and the do-it-by-hand alternative a caller had before: search + fetch_k x
get_vector + the pairwise similarities and the greedy selection in numpy on the host.
One JSON line per measurement on stdout and in profiles/mmr_<n>x<dim>.jsonl.

    python tools/mmr_probe.py [--rows 10000000] [--dim 384] [--calls 100] [--trace-calls 0]

--trace-calls N: only N MMR calls per (k, fetch_k) and nothing else (the run to put under `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((4, 20), (10, 60), (10, 256), (64, 1024))
LAMBDA = 0.5


def med(ts):
    return round(float(np.median(np.asarray(ts) * 1e3)), 4)


def by_hand(idx, q, k, fetch_k):
    """what a caller did without the entry point (cosine): fetch, copy every row out, f64 similarities, greedy selection"""
    ids, rel = idx.search_arrays(q, fetch_k, 0)
    rows = np.array([idx.get_vector(int(i)).values for i in ids])
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    sim = unit @ unit.T
    sel, red = [0], np.full(ids.size, -np.inf)
    left = np.ones(ids.size, dtype=bool)
    left[0] = False
    while len(sel) < min(k, ids.size):
        red = np.maximum(red, sim[:, sel[-1]])
        v = np.where(left, LAMBDA * rel - (1.0 - LAMBDA) * red, -np.inf)
        best = int(np.argmax(v))
        sel.append(best)
        left[best] = False
    return ids[sel], rel[sel]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim = args.rows, args.dim
    fh = None
    if not args.trace_calls:
        out_path = args.out or os.path.join(ROOT, "profiles", f"mmr_{n}x{dim}.jsonl")
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        fh = open(out_path, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    idx = V.FlatIndex(dim)
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
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)

    if args.trace_calls:
        for k, fetch_k in SHAPES:
            for _ in range(args.trace_calls):
                idx.search_mmr_arrays(q, k, fetch_k, LAMBDA, 0)
        return

    def alternate(plain, mmr, calls, warm=10):
        pt, mt = [], []
        for i in range(warm + calls):
            t0 = time.perf_counter()
            plain()
            t1 = time.perf_counter()
            mmr()
            t2 = time.perf_counter()
            if i >= warm:
                pt.append(t1 - t0)
                mt.append(t2 - t1)
        return med(pt), med(mt)

    for k, fetch_k in SHAPES:
        calls = args.calls if fetch_k <= 60 else max(10, args.calls // 5)  # the exact routes take milliseconds per call
        p, m = alternate(lambda: idx.search_arrays(q, fetch_k, 0), lambda: idx.search_mmr_arrays(q, k, fetch_k, LAMBDA, 0), calls)
        path = V.last_path()
        emit({"what": "mmr", "rows": n, "dim": dim, "k": k, "fetch_k": fetch_k, "lambda": LAMBDA, "path": path,
              "search_median_ms": p, "mmr_median_ms": m, "tail_ms": round(m - p, 4), "calls": calls})
        ts = []
        for _ in range(max(3, calls // 10)):
            t0 = time.perf_counter()
            by_hand(idx, q, k, fetch_k)
            ts.append(time.perf_counter() - t0)
        emit({"what": "by_hand", "rows": n, "dim": dim, "k": k, "fetch_k": fetch_k, "median_ms": med(ts),
              "note": "search + fetch_k x get_vector + numpy similarities and selection"})

    for frac in (0.01, 0.1):
        msub = max(1, int(round(n * frac)))
        keep = rng.choice(n, size=msub, replace=False).astype(np.uint64)
        with idx.make_filter(keep) as f:
            for k, fetch_k in SHAPES:
                calls = args.calls if fetch_k <= 60 else max(10, args.calls // 5)
                p, m = alternate(lambda: idx.search_arrays(q, fetch_k, 0, filter=f),
                                 lambda: idx.search_mmr_arrays(q, k, fetch_k, LAMBDA, 0, filter=f), calls)
                emit({"what": "mmr_filtered", "rows": n, "dim": dim, "fraction": frac, "subset_rows": msub, "k": k,
                      "fetch_k": fetch_k, "lambda": LAMBDA, "path": V.last_path(), "search_median_ms": p, "mmr_median_ms": m,
                      "tail_ms": round(m - p, 4), "calls": calls})
    fh.close()


if __name__ == "__main__":
    main()

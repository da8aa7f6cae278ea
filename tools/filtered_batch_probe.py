"""Batches of filtered searches on the headline index (10 M x 384 cosine unit rows by default, built as
tools/filtered_probe.py builds it), k = 10, filters made before the timed region.

Cells with one filter per query (256 distinct filters of random ids, reused round-robin): nq in {16, 256, 4096} x filter
size in {0.001 %, 0.01 %, 0.1 %, 1 %}.  Cells with one shared filter: 0.1 %, 1 %, 10 %, 100 % at nq in {16, 256}.  In the
same process every cell alternates 3 + 3 timed runs of the batch call with the loop of search_arrays(..., filter=) over
the same pairs (what the batch entry point did before it shared launches); reported are the median ms per batch, QPS,
the loop's own spread (min .. max of its runs) and the routing of the batch call: launches, the last launch's gx, jobs
cut by it (a lone scan of their rows would use more workgroups), batched / single / exact jobs.  Separately: the first
batch call after one add() with all 256 filters stale.  One JSON line per cell on stdout and in
profiles/filtered_batch_<n>x<dim>.jsonl.

    python tools/filtered_batch_probe.py [--rows 10000000] [--dim 384] [--trace]

--trace runs a few batch calls of every per-query cell and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the kernel times.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOBS_VARIANT_BASE = 6_000_000


def need_of(m, variant):
    """Workgroups a lone subset scan of m rows would use before its cap, from the jobs variant that ran."""
    if variant >= JOBS_VARIANT_BASE:
        g, u = (variant - JOBS_VARIANT_BASE) // 10000, variant % 100
    else:
        g, u = -variant - JOBS_VARIANT_BASE, 1
    rps = 64 // g
    steps = -(-m // rps)
    return max(1, -(-steps // (4 * u)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim, k = args.rows, args.dim, 10
    out_path = args.out or os.path.join(ROOT, "profiles", f"filtered_batch_{n}x{dim}.jsonl")
    fh = None
    if not args.trace:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        fh = open(out_path, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    idx = V.FlatIndex(dim)
    idx.reserve(n + 16)
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
    Q = rng.standard_normal((4096, dim))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)

    def routing(ms_of_jobs):
        st = idx.last_filtered_batch()
        sc = idx.last_scan()
        if st["launches"]:
            st["last_gx"] = sc["grid"]
            st["cut_by_last_gx"] = int(sum(1 for m in ms_of_jobs if need_of(m, sc["variant"]) > sc["grid"]))
        return st

    def cell(kind, frac, nq, filters, rows_of):
        Qc = np.ascontiguousarray(Q[:nq])
        per_query = [filters[i % len(filters)] for i in range(nq)]

        def batch():
            if kind == "shared":
                return idx.search_batch(Qc, k, 0, filter=filters[0])
            return idx.search_batch(Qc, k, 0, filters=per_query)

        def loop():
            return [idx.search_arrays(Qc[i], k, 0, filter=per_query[i]) for i in range(nq)]

        b = batch()  # warm
        route = routing([rows_of[i % len(filters)] for i in range(nq)])  # (before a single search overwrites last_scan)
        lp = loop()  # warm, and the two must agree
        for i in range(nq):
            assert b[0][i, : lp[i][0].size].tolist() == lp[i][0].tolist()
        if args.trace:
            for _ in range(3):
                batch()
            return
        tb, tl = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            batch()
            tb.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            loop()
            tl.append(time.perf_counter() - t0)
        mb, ml = float(np.median(tb)) * 1e3, float(np.median(tl)) * 1e3
        emit({"cell": kind, "fraction": frac, "nq": nq, "rows_per_filter": int(np.median(rows_of)),
              "batch_ms": round(mb, 4), "batch_qps": round(nq / mb * 1e3, 1), "loop_ms": round(ml, 4),
              "loop_qps": round(nq / ml * 1e3, 1), "loop_ms_min": round(min(tl) * 1e3, 4), "loop_ms_max": round(max(tl) * 1e3, 4),
              "batch_ms_runs": [round(t * 1e3, 4) for t in tb], "speedup": round(ml / mb, 3), "routing": route})

    for frac in (0.00001, 0.0001, 0.001, 0.01):
        m = max(1, int(n * frac))
        filters = [idx.make_filter(rng.integers(0, n, size=m, dtype=np.uint64)) for _ in range(256)]  # (a repeat is ignored)
        rows_of = [f.rows() for f in filters]
        for nq in (16, 256, 4096):
            cell("per-query", frac, nq, filters, rows_of)
        if frac == 0.0001 and not args.trace:
            # every filter stale: the first batch call after one add() resolves all 256 of them
            idx.add(V.Vector(id=n + 7, values=list(Q[0])))
            per_query = [filters[i % 256] for i in range(256)]
            t0 = time.perf_counter()
            idx.search_batch(np.ascontiguousarray(Q[:256]), k, 0, filters=per_query)
            first = time.perf_counter() - t0
            t0 = time.perf_counter()
            idx.search_batch(np.ascontiguousarray(Q[:256]), k, 0, filters=per_query)
            again = time.perf_counter() - t0
            emit({"cell": "stale", "fraction": frac, "nq": 256, "stale_filters": 256, "first_call_ms": round(first * 1e3, 3),
                  "next_call_ms": round(again * 1e3, 3)})
        for f in filters:
            f.close()
    if not args.trace:
        for frac in (0.001, 0.01, 0.1, 1.0):
            m = max(1, int(n * frac))
            ids = np.arange(n, dtype=np.uint64) if frac == 1.0 else rng.integers(0, n, size=m, dtype=np.uint64)
            f = idx.make_filter(ids)
            for nq in (16, 256):
                cell("shared", frac, nq, [f], [f.rows()])
            f.close()
    if fh:
        fh.close()


if __name__ == "__main__":
    main()

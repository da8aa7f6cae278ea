"""Batched range search on the headline index (10 M x 384 cosine unit rows by default): for 256 / 2048 / 4096 queries and
thresholds that let about 10 and about 1 000 rows per query qualify, the median ms of
  (a) search_range_batch_arrays,
  (b) search_batch(k = 10) with the same queries -- the yardstick: the same pass-1 kernel behind a sampling pass and
      threshold stages,
  (c) (256 queries only) the loop of single search_range_arrays calls a caller wrote before (and, for the factor a batch is
      worth on the top-k side, the loop of single search_arrays(k = 10) calls),
alternated call by call on one handle, with the route counts of the batch call.  The spread of the (b) medians over the
alternated repeats is the noise figure the (a)/(b) ratio is read against.
One JSON line per measurement on stdout and in profiles/range_batch_<n>x<dim>.jsonl.

    python tools/range_batch_probe.py [--rows 10000000] [--dim 384] [--repeats 3] [--calls 5] [--trace-calls 0]

--trace-calls N: only N batch range calls per shape and nothing else (the run to put under `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--repeats", type=int, default=3, help="alternated repeats per shape (each gives one median)")
    ap.add_argument("--calls", type=int, default=5, help="calls per repeat")
    ap.add_argument("--batches", default="256,2048,4096")
    ap.add_argument("--loop-queries", type=int, default=256, help="the batch size that is also timed as a loop of single calls")
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim = args.rows, args.dim
    fh = None
    if not args.trace_calls:
        out_path = args.out or os.path.join(ROOT, "profiles", f"range_batch_{n}x{dim}.jsonl")
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
    rng = np.random.default_rng(2)
    batches = [int(b) for b in args.batches.split(",")]
    all_q = rng.standard_normal((max(batches), dim))
    all_q /= np.linalg.norm(all_q, axis=1, keepdims=True)

    # ~10 rows per query: each query's own 10th best score (one top-k batch, which also builds the bf16 slab);
    # ~1000 rows per query: one scalar for the batch, the 1000th best score of the first query
    _, top10, _ = idx.search_batch(all_q, 10, 0)
    thr10 = np.ascontiguousarray(top10[:, 9])
    w_big = min(1000, n)
    _, top_big = idx.search_arrays(all_q[0], w_big, 0)
    thr_big = float(top_big[w_big - 1])
    shapes = [("10", lambda nq: thr10[:nq], 16), ("1000", lambda nq: np.full(nq, thr_big), 2048)]

    def med(ts):
        return round(float(np.median(np.asarray(ts) * 1e3)), 4)

    for nq in batches:
        q = np.ascontiguousarray(all_q[:nq])
        for name, thr_of, limit in shapes:
            ms = thr_of(nq)
            run_a = lambda: idx.search_range_batch_arrays(q, ms, 0, limit=limit)  # noqa: E731
            run_b = lambda: idx.search_batch(q, 10, 0)  # noqa: E731
            if args.trace_calls:
                for _ in range(args.trace_calls):
                    run_a()
                continue
            _, _, totals = run_a()
            routes, launch = idx.last_range_batch(), idx.last_filter()
            run_b()
            a_meds, b_meds, c_meds, d_meds = [], [], [], []
            loop = nq == args.loop_queries
            for _ in range(args.repeats):
                ta, tb, tc, td = [], [], [], []
                for _ in range(args.calls):
                    t0 = time.perf_counter()
                    run_a()
                    t1 = time.perf_counter()
                    run_b()
                    t2 = time.perf_counter()
                    ta.append(t1 - t0)
                    tb.append(t2 - t1)
                if loop:  # the loop of single calls is seconds long: once per repeat
                    t0 = time.perf_counter()
                    for i in range(nq):
                        idx.search_range_arrays(q[i], float(ms[i]), 0, limit=limit)
                    tc.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    for i in range(nq):
                        idx.search_arrays(q[i], 10, 0)
                    td.append(time.perf_counter() - t0)
                a_meds.append(med(ta))
                b_meds.append(med(tb))
                if loop:
                    c_meds.append(med(tc))
                    d_meds.append(med(td))
            a, b = float(np.median(a_meds)), float(np.median(b_meds))
            rec = {"what": "range_batch", "rows": n, "dim": dim, "queries": nq, "qualifying_target": name,
                   "qualifying_mean": round(float(np.mean(totals)), 1), "qualifying_max": int(np.max(totals)), "limit": limit,
                   "routes": routes, "filter": launch,
                   "a_range_batch_ms": round(a, 4), "a_medians": a_meds,
                   "b_search_batch_k10_ms": round(b, 4), "b_medians": b_meds,
                   "b_spread": round((max(b_meds) - min(b_meds)) / b, 4), "a_over_b": round(a / b, 4)}
            if loop:
                c = float(np.median(c_meds))
                d = float(np.median(d_meds))
                rec.update({"c_single_range_loop_ms": round(c, 2), "c_medians": c_meds, "c_over_a": round(c / a, 1),
                            "d_single_search_loop_ms": round(d, 2), "d_over_b": round(d / b, 1)})
            emit(rec)
    if fh:
        fh.close()


if __name__ == "__main__":
    main()

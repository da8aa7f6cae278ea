"""The deep-k batch on a 10 M x 384 cosine index with 256 and 2048 queries at k = 100 and 1000: per
record three calls, alternated call by call in one process on one handle --
  (a) search_batch(k) with the deep-k batch on;
  (b) search_batch(k = 60), the existing batch route at its largest k;
  (c) the loop of search(k) over 16 of the queries, SCALED to the batch's query count (labelled as scaled).
Rows and queries are unit gaussian.  Median wall time per call (and min .. max of --reps) and last_deep_batch() (the route
does not report its largest candidate count).  One JSON line per record on stdout and in profiles/deep_batch_<n>x<dim>.jsonl.

    python tools/deep_batch_probe.py [--shape 10000000x384] [--queries 256,2048] [--k 100,1000] [--reps 5]
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
    ap.add_argument("--shape", default="10000000x384")
    ap.add_argument("--queries", default="256,2048")
    ap.add_argument("--k", default="100,1000")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import vectorlite_amd as V

    def spread(t):
        return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(min(t) * 1e3, 4), "max_ms": round(max(t) * 1e3, 4)}

    n, dim = (int(v) for v in args.shape.split("x"))
    out_path = os.path.join(ROOT, "profiles", f"deep_batch_{n}x{dim}.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    rng = np.random.default_rng(1)
    idx = V.FlatIndex(dim)
    idx.reserve(n)
    for lo in range(0, n, 100000):
        hi = min(n, lo + 100000)
        idx.add_rows(np.arange(lo, hi, dtype=np.uint64), rng.standard_normal((hi - lo, dim)), validate=False)
    idx.set_coalescing(0)
    idx.set_deep_batch("on")
    with open(out_path, "w") as fh:
        for nq in (int(v) for v in args.queries.split(",")):
            Q = rng.standard_normal((nq, dim))
            for k in (int(v) for v in args.k.split(",")):
                idx.search_batch(Q, k, 0)  # warm: the bf16 copy, the workspace
                rec = {"rows": n, "dim": dim, "queries": nq, "k": k, "metric": 0, "last_deep_batch": idx.last_deep_batch()}
                t = {"deep": [], "k60": [], "loop16": []}
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    idx.search_batch(Q, k, 0)
                    t1 = time.perf_counter()
                    idx.search_batch(Q, 60, 0)
                    t2 = time.perf_counter()
                    for q in Q[:16]:
                        idx.search_arrays(q, k, 0)
                    t3 = time.perf_counter()
                    t["deep"].append(t1 - t0)
                    t["k60"].append(t2 - t1)
                    t["loop16"].append((t3 - t2) * nq / 16)
                rec["deep_batch"] = spread(t["deep"])
                rec["search_batch_k60"] = spread(t["k60"])
                rec["single_loop_scaled_from_16_queries"] = spread(t["loop16"])
                line = json.dumps(rec)
                print(line, flush=True)
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""The k-nearest-neighbour graph on 100 k and 1 M x 384 rows at k = 10 and 32: per record three calls,
alternated call by call in one process on one handle --
  (a) knn_graph (the row-stationary MFMA pass with per-row top-k lists, its seeds and its keep pass);
  (b) the same call on the exact route (one positional search per row), only up to --exact-rows rows: the answers must be
      equal bit for bit;
  (c) the by-hand loop: export the rows, search_batch(k + 1) over them in slices of --slice queries (the figure to judge (a)
      against; its self match is not stripped and its answer is not compared).
Rows are gaussian directions with lengths over 0.25 .. 4.  Wall time per call (median of --reps) and last_knn().  One JSON
line per record on stdout and in profiles/knn_<n>x<dim>.jsonl.

    python tools/knn_probe.py [--shapes 100000x384,1000000x384] [--ks 10,32] [--reps 3]
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
    ap.add_argument("--shapes", default="100000x384,1000000x384")
    ap.add_argument("--ks", default="10,32")
    ap.add_argument("--exact-rows", type=int, default=100000)
    ap.add_argument("--slice", type=int, default=2048)
    ap.add_argument("--metrics", default="0,1,3")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    import vectorlite_amd as V

    for shape in args.shapes.split(","):
        n, dim = (int(v) for v in shape.split("x"))
        out_path = os.path.join(ROOT, "profiles", f"knn_{n}x{dim}.jsonl")
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        rng = np.random.default_rng(1)
        idx = V.FlatIndex(dim)
        idx.reserve(n)
        for lo in range(0, n, 100000):
            hi = min(n, lo + 100000)
            x = rng.standard_normal((hi - lo, dim))
            x *= rng.uniform(0.25, 4.0, (hi - lo, 1)) / np.linalg.norm(x, axis=1, keepdims=True)
            idx.add_rows(np.arange(lo, hi, dtype=np.uint64), x, validate=False)
        idx.set_coalescing(0)
        with open(out_path, "w") as fh:
            for k in (int(v) for v in args.ks.split(",")):
                for metric in (int(v) for v in args.metrics.split(",")):
                    _, nbr, sc = idx.knn_graph(k, metric)  # warm: the bf16 copy, the workspace
                    rec = {"rows": n, "dim": dim, "k": k, "metric": metric, "report": idx.last_knn()}
                    t_new, t_exact, t_loop = [], [], []
                    for _ in range(args.reps):  # alternated call by call
                        if n <= args.exact_rows:
                            idx.set_knn_route("exact")
                            t0 = time.perf_counter()
                            _, enbr, esc = idx.knn_graph(k, metric)
                            t_exact.append(time.perf_counter() - t0)
                            idx.set_knn_route("auto")
                            rec["same_as_exact_route"] = bool(enbr.tolist() == nbr.tolist() and
                                                              esc.view(np.uint64).tolist() == sc.view(np.uint64).tolist())
                        t0 = time.perf_counter()
                        idx.knn_graph(k, metric)
                        t1 = time.perf_counter()
                        _, rows = idx.export()
                        for lo in range(0, n, args.slice):
                            idx.search_batch(rows[lo:lo + args.slice], k + 1, metric)
                        t2 = time.perf_counter()
                        t_new.append(t1 - t0)
                        t_loop.append(t2 - t1)
                    rec["knn_graph_ms"] = round(float(np.median(t_new)) * 1e3, 4)
                    rec["search_batch_loop_ms"] = round(float(np.median(t_loop)) * 1e3, 4)
                    if t_exact:
                        rec["exact_route_ms"] = round(float(np.median(t_exact)) * 1e3, 4)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    fh.write(line + "\n")
        del idx


if __name__ == "__main__":
    main()

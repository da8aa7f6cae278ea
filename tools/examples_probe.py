"""Search by examples on 10 M x 384 and 1 M x 768 rows with (a, b) = (1, 0), (8, 0), (8, 4), (64, 32)
positives and negatives: per record three calls, alternated call by call in one process on one handle --
  (a) search_examples (the MFMA pass that leaves two floats per row, its seeds and its survivors);
  (b) the same call with the exact route forced (one exact scan per example): the answers must be equal bit for bit;
  (c) search_batch of the a + b examples as independent queries (what a caller fusing lists by hand pays; not an answer).
Rows are gaussian directions with lengths over 0.5 .. 2, the examples noisy copies of rows with lengths over 0.3 .. 3.  Wall
time per call (median and min .. max of --reps) and last_examples().  One JSON line per record on stdout and in
profiles/examples_<n>x<dim>.jsonl.

    python tools/examples_probe.py [--shapes 10000000x384,1000000x768] [--k 10] [--metrics 0,1,3] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = [(1, 0), (8, 0), (8, 4), (64, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000000x384,1000000x768")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metrics", default="0,1,3")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    import vectorlite_amd as V

    def spread(t):
        return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(min(t) * 1e3, 4), "max_ms": round(max(t) * 1e3, 4)}

    for shape in args.shapes.split(","):
        n, dim = (int(v) for v in shape.split("x"))
        out_path = os.path.join(ROOT, "profiles", f"examples_{n}x{dim}.jsonl")
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        rng = np.random.default_rng(1)
        idx = V.FlatIndex(dim)
        idx.reserve(n)
        for lo in range(0, n, 100000):
            hi = min(n, lo + 100000)
            x = rng.standard_normal((hi - lo, dim))
            x *= rng.uniform(0.5, 2.0, (hi - lo, 1)) / np.linalg.norm(x, axis=1, keepdims=True)
            idx.add_rows(np.arange(lo, hi, dtype=np.uint64), x, validate=False)
        idx.set_coalescing(0)
        with open(out_path, "w") as fh:
            for a, b in SETS:
                src = x[rng.choice(len(x), a + b, replace=False)]  # rows of the last chunk added
                E = src / np.linalg.norm(src, axis=1, keepdims=True) + 0.1 * rng.standard_normal((a + b, dim)) / np.sqrt(dim)
                E *= np.geomspace(0.3, 3.0, a + b)[:, None]
                pos, neg = np.ascontiguousarray(E[:a]), (np.ascontiguousarray(E[a:]) if b else None)
                for metric in (int(v) for v in args.metrics.split(",")):
                    ids, sc = idx.search_examples_arrays(pos, neg, args.k, metric)  # warm: the bf16 copy, the workspace
                    rec = {"rows": n, "dim": dim, "a": a, "b": b, "k": args.k, "metric": metric, "report": idx.last_examples()}
                    t_new, t_exact, t_batch = [], [], []
                    for _ in range(args.reps):  # alternated call by call
                        t0 = time.perf_counter()
                        idx.search_examples_arrays(pos, neg, args.k, metric)
                        t1 = time.perf_counter()
                        idx.force_path(V.PATH_EXACT_SORT)
                        eids, esc = idx.search_examples_arrays(pos, neg, args.k, metric)
                        idx.force_path(V.PATH_NONE)
                        t2 = time.perf_counter()
                        idx.search_batch(E, args.k, metric)
                        t3 = time.perf_counter()
                        t_new.append(t1 - t0)
                        t_exact.append(t2 - t1)
                        t_batch.append(t3 - t2)
                        rec["same_as_exact_route"] = bool(eids.tolist() == ids.tolist() and
                                                          esc.view(np.uint64).tolist() == sc.view(np.uint64).tolist())
                    rec["search_examples"] = spread(t_new)
                    rec["exact_route"] = spread(t_exact)
                    rec["search_batch_of_examples"] = spread(t_batch)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    fh.write(line + "\n")
        del idx


if __name__ == "__main__":
    main()

"""Nearest-label assignment on 10 M x 384 and 1 M x 768 rows with 16 / 128 / 1024 / 4096 labels: per
record three calls, alternated call by call in one process on one handle --
  (a) assign (the row-stationary MFMA pass, its seed and its second pass);
  (b) the same call on the exact route (one exact scan per label), only up to --exact-labels labels: the answers must be
      equal bit for bit;
  (c) search_batch of the labels over the index at k = 10: k_mfma_rows' pass over the same multiply-adds, the yardstick for
      the pass itself (it answers another question: the best rows per label).
Rows are gaussian directions with lengths over 0.25 .. 4, labels noisy copies of rows.  Wall time per call (median of
--reps) and last_assign().  One JSON line per record on stdout and in profiles/assign_<n>x<dim>.jsonl.

    python tools/assign_probe.py [--shapes 10000000x384,1000000x768] [--labels 16,128,1024,4096] [--reps 3]
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
    ap.add_argument("--shapes", default="10000000x384,1000000x768")
    ap.add_argument("--labels", default="16,128,1024,4096")
    ap.add_argument("--exact-labels", type=int, default=16)
    ap.add_argument("--metrics", default="0,1,3")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    for shape in args.shapes.split(","):
        n, dim = (int(v) for v in shape.split("x"))
        out_path = os.path.join(ROOT, "profiles", f"assign_{n}x{dim}.jsonl")
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        idx = V.FlatIndex(dim)
        idx.reserve(n)
        g = torch.Generator(device="cuda:0")
        g.manual_seed(1)
        step = 1_000_000
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            x = torch.randn((hi - lo, dim), dtype=torch.float64, device="cuda:0", generator=g)
            x *= (0.25 + 3.75 * torch.rand((hi - lo, 1), dtype=torch.float64, device="cuda:0", generator=g)) / torch.linalg.vector_norm(x, dim=1, keepdim=True)
            idx.add_rows(np.arange(lo, hi, dtype=np.uint64), x, validate=False)
            del x
        torch.cuda.synchronize()
        idx.set_coalescing(0)
        rng = np.random.default_rng(2)
        with open(out_path, "w") as fh:
            for L in (int(v) for v in args.labels.split(",")):
                src = rng.integers(0, n, L)
                Y = np.array([idx.get_vector(int(i)).values for i in src]) + 0.3 * rng.standard_normal((L, dim)) / np.sqrt(dim)
                for metric in (int(v) for v in args.metrics.split(",")):
                    _, lab, sc = idx.assign(Y, metric)  # warm: the bf16 copy, the workspace
                    rec = {"rows": n, "dim": dim, "labels": L, "metric": metric, "report": idx.last_assign()}
                    t_new, t_exact, t_batch = [], [], []
                    for _ in range(args.reps):  # alternated call by call
                        if L <= args.exact_labels:
                            idx.set_assign_route("exact")
                            t0 = time.perf_counter()
                            _, elab, esc = idx.assign(Y, metric)
                            t_exact.append(time.perf_counter() - t0)
                            idx.set_assign_route("auto")
                            rec["same_as_exact_route"] = bool(elab.tolist() == lab.tolist() and
                                                              esc.view(np.uint64).tolist() == sc.view(np.uint64).tolist())
                        t0 = time.perf_counter()
                        idx.assign(Y, metric)
                        t1 = time.perf_counter()
                        idx.search_batch(Y, 10, metric)
                        t2 = time.perf_counter()
                        t_new.append(t1 - t0)
                        t_batch.append(t2 - t1)
                    rec["assign_ms"] = round(float(np.median(t_new)) * 1e3, 4)
                    rec["search_batch_ms"] = round(float(np.median(t_batch)) * 1e3, 4)
                    if t_exact:
                        rec["exact_route_ms"] = round(float(np.median(t_exact)) * 1e3, 4)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    fh.write(line + "\n")
        del idx


if __name__ == "__main__":
    main()

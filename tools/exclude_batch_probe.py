"""Batches of exclusion-filtered queries on the headline index (10 M x 384 cosine unit rows, k = 10 by default): per record
three calls on the SAME queries, alternated in one process on one handle --
  (a) search_batch unfiltered: the yardstick the masked MFMA pass should approach;
  (b) the exclusion batch with set_masked_batch("on"): the mask-aware pass;
  (c) the exclusion batch with set_masked_batch("off"): the jobs kernel over each token's position list;
and what "auto" (masked_batch_plan.hpp's cost rule) chose for the same call.  Records: 16 / 256 / 2048 queries under one
shared set of 0 / 100 / 10 000 / 1 M / 5 M excluded ids, 256 queries under 256 distinct sets of 100 ids, and a sweep of
kept fractions 50 % .. 0.1 % at 16 and 256 queries that brackets the point where (c) overtakes (b).  Wall time per call
(median of --reps), the scan kernels' time from HIP events and their accounted bytes (profile), the routes' reports.  One
JSON line per record on stdout and in profiles/exclude_batch_<n>x<dim>.jsonl.

    python tools/exclude_batch_probe.py [--rows 10000000] [--dim 384] [--reps 5] [--quick]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="256 queries only, no 2048-query records, a short sweep")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim, k = args.rows, args.dim, 10
    out_path = args.out or os.path.join(ROOT, "profiles", f"exclude_batch_{n}x{dim}.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    fh = open(out_path, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
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
    Q_all = rng.standard_normal((2048, dim))
    Q_all /= np.linalg.norm(Q_all, axis=1, keepdims=True)

    def timed(fn, reps):
        """median wall ms of fn(), then one profiled call: (kernel ms from HIP events, accounted bytes, launches)"""
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        idx.profile_read()
        idx.profile_enable(True)
        fn()
        idx.profile_enable(False)
        nl, ms, by = idx.profile_read()
        return {"wall_ms": round(float(np.median(ts)) * 1e3, 4), "kernel_ms": round(ms, 4), "bytes": int(by), "launches": int(nl)}

    def record(what, Q, filt_kw, excluded_desc, kept, reps):
        rec = {"what": what, "rows": n, "dim": dim, "k": k, "queries": int(Q.shape[0]), "excluded": excluded_desc, "kept": kept}
        rec["unfiltered"] = timed(lambda: idx.search_batch(Q, k, 0), reps)
        idx.set_masked_batch("on")
        rec["masked_on"] = timed(lambda: idx.search_batch(Q, k, 0, **filt_kw), reps)
        rec["masked_on"]["report"] = idx.last_masked_batch()
        got_on = idx.search_batch(Q, k, 0, **filt_kw)
        idx.set_masked_batch("off")
        rec["masked_off"] = timed(lambda: idx.search_batch(Q, k, 0, **filt_kw), reps)
        rec["masked_off"]["report"] = idx.last_filtered_batch()
        got_off = idx.search_batch(Q, k, 0, **filt_kw)
        rec["same_answers"] = bool((got_on[0] == got_off[0]).all() and (got_on[1].view(np.uint64) == got_off[1].view(np.uint64)).all())
        idx.set_masked_batch("auto")
        idx.search_batch(Q, k, 0, **filt_kw)
        rec["auto_routed"] = idx.last_masked_batch()["routed"]
        a, b, c = rec["unfiltered"]["wall_ms"], rec["masked_on"]["wall_ms"], rec["masked_off"]["wall_ms"]
        rec["on_over_unfiltered"] = round(b / a, 3)
        rec["off_over_on"] = round(c / b, 3)
        rec["auto_took_the_faster"] = bool((rec["auto_routed"] > 0) == (b < c))
        emit(rec)

    batch_sizes = (256,) if args.quick else (16, 256, 2048)
    for size in (0, 100, 10_000, 1_000_000, 5_000_000):
        size = min(size, n // 2)
        excluded = rng.choice(n, size=size, replace=False).astype(np.uint64) if size else np.zeros(0, np.uint64)
        with idx.make_filter(excluded, exclude=True) as f:
            for nq in batch_sizes:
                # the jobs route reads nq x kept x 1536 B: one repetition is enough where that is seconds
                record("shared set", Q_all[:nq], {"filter": f}, size, f.rows(), args.reps if nq * (n - size) < 3e9 else 1)
    filters = [idx.make_filter(rng.choice(n, size=100, replace=False).astype(np.uint64), exclude=True) for _ in range(256)]
    try:
        record("one set of 100 ids per query", Q_all[:256], {"filters": filters}, 100, n - 100, args.reps)
    finally:
        for f in filters:
            f.close()
    # where the jobs route overtakes the masked pass: kept fractions from 50 % down
    for frac in ((0.5, 0.05, 0.005) if args.quick else (0.5, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005, 0.002, 0.001)):
        kept = int(n * frac)
        excluded = rng.choice(n, size=n - kept, replace=False).astype(np.uint64)
        with idx.make_filter(excluded, exclude=True) as f:
            for nq in ((256,) if args.quick else (16, 256)):
                record("kept fraction sweep", Q_all[:nq], {"filter": f}, n - kept, f.rows(), args.reps)
    fh.close()


if __name__ == "__main__":
    main()

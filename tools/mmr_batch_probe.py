"""Batches of diversified (MMR) queries on the headline index (10 M x 384 cosine unit rows): per record three calls on the
SAME queries, alternated call by call in one process on one handle --
  (a) search_mmr_batch_arrays with set_mmr_batch("on"): the MFMA pass with the rank / similarity / selection stage;
  (b) the loop of search_mmr_arrays over the same queries (what a caller did before);
  (c) search_batch(k = fetch_k) unfiltered: the plain top-k batch the pass rides on;
and what "auto" (mmr_batch_plan.hpp's cost rule) chose for the same call.  (k, fetch_k) = (4, 20) and (10, 60), lambda 0.5,
16 / 256 / 2048 queries unfiltered; an include-1 % and an exclude-10 000 record at (4, 20), 256 queries.  The open numbers are
the hand-back rate (settled / handed_back of the report -- a property of these independent gaussian rows) and the speed-up
over the loop, both from the same run.  Wall time per call (median of --reps).  The loop over more than --loop-cap queries is
timed on that many (the record says how many) and scaled.  One JSON line per record on stdout and in
profiles/mmr_batch_<n>x<dim>.jsonl.

    python tools/mmr_batch_probe.py [--rows 10000000] [--dim 384] [--reps 3] [--quick]
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=256, help="queries of a batch the loop is timed on")
    ap.add_argument("--quick", action="store_true", help="no 2048-query records")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim, lam = args.rows, args.dim, 0.5
    out_path = args.out or os.path.join(ROOT, "profiles", f"mmr_batch_{n}x{dim}.jsonl")
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

    def med(ts):
        return round(float(np.median(ts)) * 1e3, 4)

    def record(what, Q, k, fetch_k, filt=None):
        nq = int(Q.shape[0])
        loop_q = Q[:min(nq, args.loop_cap)]
        rec = {"what": what, "rows": n, "dim": dim, "k": k, "fetch_k": fetch_k, "lambda": lam, "queries": nq,
               "filter_rows": filt.rows() if filt is not None else None, "loop_queries": int(loop_q.shape[0])}
        idx.set_mmr_batch("on")
        got = idx.search_mmr_batch_arrays(Q, k, fetch_k, lam, 0, filter=filt)  # warm: the bf16 copy, the bitmap, the scratch
        rec["report"] = idx.last_mmr_batch()
        same = True
        for i in range(min(nq, 8)):
            li, ls = idx.search_mmr_arrays(Q[i], k, fetch_k, lam, 0, filter=filt)
            m = int(got[2][i])
            same = same and m == li.size and got[0][i, :m].tolist() == li.tolist() \
                and got[1][i, :m].view(np.uint64).tolist() == ls.view(np.uint64).tolist()
        rec["same_answers_first_8"] = bool(same)
        idx.search_batch(Q, fetch_k, 0)
        t_batch, t_loop, t_plain = [], [], []
        for _ in range(args.reps):  # alternated call by call
            t0 = time.perf_counter()
            idx.search_mmr_batch_arrays(Q, k, fetch_k, lam, 0, filter=filt)
            t1 = time.perf_counter()
            for q in loop_q:
                idx.search_mmr_arrays(q, k, fetch_k, lam, 0, filter=filt)
            t2 = time.perf_counter()
            idx.search_batch(Q, fetch_k, 0)
            t3 = time.perf_counter()
            t_batch.append(t1 - t0)
            t_loop.append(t2 - t1)
            t_plain.append(t3 - t2)
        rec["batch_ms"] = med(t_batch)
        rec["loop_ms_timed"] = med(t_loop)
        rec["loop_ms"] = round(rec["loop_ms_timed"] * nq / loop_q.shape[0], 4)
        rec["plain_topk_batch_ms"] = med(t_plain)
        rec["loop_over_batch"] = round(rec["loop_ms"] / rec["batch_ms"], 2)
        rec["batch_over_plain"] = round(rec["batch_ms"] / rec["plain_topk_batch_ms"], 3)
        idx.set_mmr_batch("auto")
        idx.search_mmr_batch_arrays(Q, k, fetch_k, lam, 0, filter=filt)
        rec["auto_routed"] = idx.last_mmr_batch()["routed"]
        rec["auto_took_the_faster"] = bool((rec["auto_routed"] > 0) == (rec["batch_ms"] < rec["loop_ms"]))
        emit(rec)

    batch_sizes = (16, 256) if args.quick else (16, 256, 2048)
    for k, fetch_k in ((4, 20), (10, 60)):
        for nq in batch_sizes:
            record("unfiltered", Q_all[:nq], k, fetch_k)
    ids = np.arange(n, dtype=np.uint64)
    with idx.make_filter(rng.choice(ids, max(n // 100, 1), replace=False)) as f:
        for nq in (16, 256):
            record("include 1 %", Q_all[:nq], 4, 20, f)
    with idx.make_filter(rng.choice(ids, min(10_000, n // 2), replace=False), exclude=True) as f:
        record("exclude 10 000 ids", Q_all[:256], 4, 20, f)
    fh.close()


if __name__ == "__main__":
    main()

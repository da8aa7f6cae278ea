"""The similarity self-join on unit gaussian rows with planted duplicates (100 k and 1 M x 384 by default): on one handle,
alternated call by call, the median wall ms of
  (a) similarity_join_arrays on the mfma route,
  (b) the same call on the loop route (only up to --loop-max-rows rows: it is one range call per row),
  (c) search_range_batch_arrays answering the first --ref-queries stored rows as external queries over the same rows with
      the same threshold -- k_mfma_rows' launch; scaled by rows / ref-queries it is the yardstick for k_join_rows, which
      does half the multiply-adds and stages no queries,
with last_join's counts.  --metric cosine | euclidean | dot picks the metric of all three (Euclidean and dot reach the pass
only through the mfma route; on unit rows the planted pairs score ~0.76 and ~0.95 there, so --min-score defaults to 0.75
for Euclidean and 0.9 otherwise).  Median of --repeats alternated repeats of --calls calls; "spread" = (max - min) of the (a) repeat
medians over their median.  One JSON line per size on stdout and in profiles/join_<n>x<dim>.jsonl
(join_<metric>_<n>x<dim>.jsonl for Euclidean and dot).  Per-kernel times: run
`rocprofv3 --kernel-trace --stats -- python tools/join_probe.py --trace-calls 3` (no counters in that run).

    python tools/join_probe.py [--rows 100000,1000000] [--dim 384] [--metric cosine] [--min-score 0.9] [--repeats 3] [--calls 3]
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
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--metric", choices=["cosine", "euclidean", "dot"], default="cosine")
    ap.add_argument("--min-score", type=float, default=None)
    ap.add_argument("--planted", type=int, default=1000, help="near-duplicate pairs planted at cosine ~0.95")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--loop-max-rows", type=int, default=100_000)
    ap.add_argument("--ref-queries", type=int, default=2048)
    ap.add_argument("--trace-calls", type=int, default=0)
    args = ap.parse_args()

    import vectorlite_amd as V

    metric = {"cosine": 0, "euclidean": 1, "dot": 3}[args.metric]
    if args.min_score is None:
        args.min_score = 0.75 if args.metric == "euclidean" else 0.9
    dim = args.dim
    for n in [int(r) for r in args.rows.split(",")]:
        rng = np.random.default_rng(n)
        rows = rng.standard_normal((n, dim))
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        src = rng.choice(n, size=min(args.planted, n // 2), replace=False)
        dst = (src + n // 2) % n
        noise = rng.standard_normal((src.size, dim)) / np.sqrt(dim)
        rows[dst] = 0.95 * rows[src] + np.sqrt(1 - 0.95 ** 2) * noise
        idx = V.FlatIndex(dim)
        idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)

        def run(route):
            idx.set_join_route(route)
            t0 = time.perf_counter()
            out = idx.similarity_join_arrays(args.min_score, metric, limit=4096)
            return time.perf_counter() - t0, out[3], idx.last_join()

        nq = min(args.ref_queries, n)
        ref_q = np.ascontiguousarray(rows[:nq])

        def run_ref():
            t0 = time.perf_counter()
            idx.search_range_batch_arrays(ref_q, args.min_score, metric, limit=16)
            return time.perf_counter() - t0

        if args.trace_calls:
            for _ in range(args.trace_calls):
                run("mfma")
                run_ref()
            continue
        loop = n <= args.loop_max_rows
        _, total, lj = run("mfma")  # warm-up: builds the bf16 copy, sizes the buffers
        run_ref()
        loop_total = run("loop")[1] if loop else None
        a_meds, b_meds, c_meds = [], [], []
        for _ in range(args.repeats):
            ta, tb, tc = [], [], []
            for _ in range(args.calls):
                ta.append(run("mfma")[0])
                if loop:
                    tb.append(run("loop")[0])
                tc.append(run_ref())
            a_meds.append(float(np.median(ta)) * 1e3)
            c_meds.append(float(np.median(tc)) * 1e3)
            if loop:
                b_meds.append(float(np.median(tb)) * 1e3)
        a, c = float(np.median(a_meds)), float(np.median(c_meds))
        rec = {"what": "similarity_join", "metric": args.metric, "rows": n, "dim": dim, "min_score": args.min_score, "qualifying_pairs": total,
               "last_join": lj, "a_mfma_ms": round(a, 3), "a_medians": [round(x, 3) for x in a_meds],
               "a_spread": round((max(a_meds) - min(a_meds)) / a, 4), "ref_queries": nq, "c_range_batch_ms": round(c, 3),
               "c_scaled_to_n_queries_ms": round(c * n / nq, 3)}
        if loop:
            b = float(np.median(b_meds))
            rec.update({"b_loop_ms": round(b, 3), "b_medians": [round(x, 3) for x in b_meds], "b_over_a": round(b / a, 2),
                        "loop_total_matches": loop_total == total})
        line = json.dumps(rec)
        print(line, flush=True)
        name = f"join_{n}x{dim}.jsonl" if metric == 0 else f"join_{args.metric}_{n}x{dim}.jsonl"
        path = os.path.join(ROOT, "profiles", name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(line + "\n")
        del idx


if __name__ == "__main__":
    main()

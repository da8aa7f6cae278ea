"""Grouped search on the headline index (10 M x 384 cosine unit rows by default, the last 5 000 of them near-copies of the
query's direction), k = 10, for three group tables over the same rows:
    ten_per_group   key = id // 10: ~10 rows per group (the near-copies fall into 500 groups)
    one_per_group   key = id: the worst case for pass 1's atomics, every row raises a slot of its own
    near_duplicates key = id // 10, but the 5 000 near-copies form ONE group that holds the whole top of the ranking
Per table: median / p99 ms per call of search_grouped_arrays alternated call by call with the yardstick -- the single search
with the f32 scan only (VL_SINGLE_FILTER=f32), k = 10 -- and with search_range at the same L (the score of the 10th group);
the time of k_scan_group_best and of k_scan_range from the events around them (profile_enable) and their ratio; and once the
by-hand way, search(q, len) and a host loop.  One JSON line per measurement on stdout and in
profiles/grouped_<n>x<dim>.jsonl.

    python tools/grouped_probe.py [--rows 10000000] [--dim 384] [--calls 100] [--trace-calls 0]

--trace-calls N: only N grouped calls on --trace-table (default one_per_group), each followed by the range search at the same
L, and nothing else (the run to put under `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_TB_S = 8.0
K = 10
DUPLICATES = 5000


def stats(ts):
    a = np.sort(np.asarray(ts) * 1e3)
    return {"median_ms": round(float(np.median(a)), 4), "p99_ms": round(float(a[min(len(a) - 1, int(0.99 * len(a)))]), 4),
            "mean_ms": round(float(a.mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--trace-table", default="one_per_group")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim = args.rows, args.dim
    dup = min(DUPLICATES, n // 2)
    fh = None
    if not args.trace_calls:
        out_path = args.out or os.path.join(ROOT, "profiles", f"grouped_{n}x{dim}.jsonl")
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        fh = open(out_path, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    rng = np.random.default_rng(2)
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)

    idx = V.FlatIndex(dim)
    idx.reserve(n)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    step = 2_500_000
    for lo in range(0, n - dup, step):
        hi = min(n - dup, lo + step)
        x = torch.randn((hi - lo, dim), dtype=torch.float64, device="cuda:0", generator=g)
        x /= torch.linalg.vector_norm(x, dim=1, keepdim=True)
        idx.add_rows(np.arange(lo, hi, dtype=np.uint64), x, validate=False)
        del x
    x = torch.as_tensor(q, device="cuda:0")[None, :] + 0.01 * torch.randn((dup, dim), dtype=torch.float64, device="cuda:0", generator=g)
    x /= torch.linalg.vector_norm(x, dim=1, keepdim=True)
    idx.add_rows(np.arange(n - dup, n, dtype=np.uint64), x, validate=False)
    del x
    torch.cuda.synchronize()
    idx.set_coalescing(0)
    idx.set_single_filter("f32")

    ids = np.arange(n, dtype=np.uint64)
    ten = ids // np.uint64(10)
    one_group = ten.copy()
    one_group[n - dup:] = np.uint64(1 << 40)
    tables = {}
    for name, keys in (("ten_per_group", ten), ("one_per_group", ids), ("near_duplicates", one_group)):
        t0 = time.perf_counter()
        tables[name] = idx.make_groups(ids, keys)
        emit({"what": "make_groups", "table": name, "rows": n, "distinct": tables[name].distinct(),
              "seconds": round(time.perf_counter() - t0, 3)})

    if args.trace_calls:  # one table's grouped calls and the range search at the same L: both scans in one trace
        t = tables[args.trace_table]
        L = float(idx.search_grouped_arrays(q, K, 0, groups=t)[2][-1])
        for _ in range(args.trace_calls):
            idx.search_grouped_arrays(q, K, 0, groups=t)
            idx.search_range_arrays(q, L, 0, limit=K)
        return

    def scan_ms(fn, reps=30):
        """the time between the events around the call's first slab scan, per call"""
        idx.profile_read()
        idx.profile_enable(True)
        for _ in range(reps):
            fn()
        idx.profile_enable(False)
        nl, ms, by = idx.profile_read()
        if not nl or ms <= 0:
            return None, None
        return ms / nl, by / nl

    for name, t in tables.items():
        gk, gi, gs = idx.search_grouped_arrays(q, K, 0, groups=t)
        path, scan = V.last_path(), idx.last_scan()
        L = float(gs[-1])
        _, _, survivors = idx.search_range_arrays(q, L, 0, limit=0)
        grouped_ts, topk_ts, range_ts = [], [], []
        for i in range(20 + args.calls):
            t0 = time.perf_counter()
            idx.search_arrays(q, K, 0)
            t1 = time.perf_counter()
            idx.search_grouped_arrays(q, K, 0, groups=t)
            t2 = time.perf_counter()
            idx.search_range_arrays(q, L, 0, limit=K)
            t3 = time.perf_counter()
            if i >= 20:
                topk_ts.append(t1 - t0)
                grouped_ts.append(t2 - t1)
                range_ts.append(t3 - t2)
        emit({"what": "topk_f32_k10", "table": name, "rows": n, "dim": dim, "alternated_with": "grouped", **stats(topk_ts)})
        emit({"what": "range_at_L", "table": name, "rows": n, "dim": dim, "qualifying": survivors, "alternated_with": "grouped",
              **stats(range_ts)})
        best_ms, best_bytes = scan_ms(lambda: idx.search_grouped_arrays(q, K, 0, groups=t))
        range_ms, _ = scan_ms(lambda: idx.search_range_arrays(q, L, 0, limit=K))
        rec = {"what": "grouped", "table": name, "rows": n, "dim": dim, "k": K, "distinct": t.distinct(), "path": path,
               "scan_variant": scan["variant"], "scan_grid": scan["grid"], "rows_scoring_at_least_L": survivors, **stats(grouped_ts)}
        if best_ms and range_ms:
            rec.update({"k_scan_group_best_ms": round(best_ms, 4), "k_scan_range_ms": round(range_ms, 4),
                        "group_best_over_range": round(best_ms / range_ms, 3),
                        "group_best_tb_s": round(best_bytes / (best_ms * 1e-3) / 1e12, 3),
                        "group_best_frac_of_peak": round(best_bytes / (best_ms * 1e-3) / 1e12 / HBM_PEAK_TB_S, 3)})
        emit(rec)

    # the exact route at full size, three calls: a table of 5 groups asked for 10 (fewer groups than k), so every score is
    # computed, all rows are sorted, and the collapse's one workgroup walks the whole ranking without stopping early
    with idx.make_groups(ids, ids % np.uint64(5)) as few:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            gk, _, _ = idx.search_grouped_arrays(q, K, 0, groups=few)
            ts.append(time.perf_counter() - t0)
        emit({"what": "grouped_exact_route", "table": "five_groups", "rows": n, "dim": dim, "k": K, "returned": int(gk.size),
              "path": V.last_path(), "calls_ms": [round(x * 1e3, 2) for x in ts]})

    # the by-hand way, once: the exact sort of every row, 16 bytes per row copied back, then a host loop
    t = tables["near_duplicates"]
    keys = one_group
    t0 = time.perf_counter()
    all_ids, all_scores = idx.search_arrays(q, n, 0)
    t1 = time.perf_counter()
    seen, out = set(), []
    for i, s in zip(all_ids.tolist(), all_scores.tolist()):
        gkey = int(keys[i])
        if gkey not in seen:
            seen.add(gkey)
            out.append((gkey, i, s))
            if len(out) == K:
                break
    t2 = time.perf_counter()
    gk, gi, gs = idx.search_grouped_arrays(q, K, 0, groups=t)
    same = [o[0] for o in out] == gk.tolist() and [o[1] for o in out] == gi.tolist() and \
        np.asarray([o[2] for o in out]).view(np.uint64).tolist() == gs.view(np.uint64).tolist()
    emit({"what": "by_hand", "table": "near_duplicates", "rows": n, "dim": dim, "search_all_ms": round((t1 - t0) * 1e3, 2),
          "host_loop_ms": round((t2 - t1) * 1e3, 2), "same_answer_as_grouped": bool(same)})
    fh.close()


if __name__ == "__main__":
    main()

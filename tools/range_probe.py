"""Range search on the headline index (10 M x 384 cosine unit rows by default): median / p99 ms per call of
search_range_arrays at thresholds chosen from one top-k answer so that about 10, 1 000 and 100 000 rows qualify, and of
the filtered form over 1 % and 10 % subsets; the yardstick -- the single search with the f32 scan only
(VL_SINGLE_FILTER=f32), k = 10 -- runs on the same index in alternation, call by call, with the ~10-row range call.
The scan's own time (events around k_scan_range) gives its fraction of the HBM peak from the f32 slab bytes, as for k_scan.
One JSON line per measurement on stdout and in profiles/range_<n>x<dim>.jsonl.

    python tools/range_probe.py [--rows 10000000] [--dim 384] [--calls 200] [--trace-calls 0]

--trace-calls N: only N range calls per threshold and nothing else (the run to put under `rocprofv3 --kernel-trace --stats`).
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


def stats(ts):
    a = np.sort(np.asarray(ts) * 1e3)
    return {"median_ms": round(float(np.median(a)), 4), "p99_ms": round(float(a[min(len(a) - 1, int(0.99 * len(a)))]), 4),
            "mean_ms": round(float(a.mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim = args.rows, args.dim
    fh = None
    if not args.trace_calls:
        out_path = args.out or os.path.join(ROOT, "profiles", f"range_{n}x{dim}.jsonl")
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
    idx.set_coalescing(0)
    idx.set_single_filter("f32")
    rng = np.random.default_rng(2)
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)

    # thresholds from one top-k answer: the score of rank r lets r + 1 rows through
    wanted = [w for w in (10, 1000, 100_000) if w <= n]
    _, top = idx.search_arrays(q, max(wanted), 0)
    thr = {w: float(top[w - 1]) for w in wanted}

    def time_calls(fn, calls):
        for _ in range(min(20, calls)):
            fn()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    if args.trace_calls:
        for w in wanted:
            for _ in range(args.trace_calls):
                idx.search_range_arrays(q, thr[w], 0, limit=w + 8)
        return

    # the yardstick and the ~10-row range call in alternation
    w0 = wanted[0]
    topk_ts, range_ts = [], []
    for i in range(20 + args.calls):
        t0 = time.perf_counter()
        idx.search_arrays(q, 10, 0)
        t1 = time.perf_counter()
        idx.search_range_arrays(q, thr[w0], 0, limit=w0 + 8)
        t2 = time.perf_counter()
        if i >= 20:
            topk_ts.append(t1 - t0)
            range_ts.append(t2 - t1)
    emit({"what": "topk_f32_k10", "rows": n, "dim": dim, "alternated_with": f"range_{w0}", **stats(topk_ts)})
    emit({"what": "range", "rows": n, "dim": dim, "qualifying": w0, "alternated_with": "topk_f32_k10", **stats(range_ts)})

    def scan_profile(fn):
        idx.profile_read()
        idx.profile_enable(True)
        for _ in range(50):
            fn()
        idx.profile_enable(False)
        nl, ms, by = idx.profile_read()
        if not nl or ms <= 0:
            return {}
        tb = by / (ms * 1e-3) / 1e12
        return {"scan_ms": round(ms / nl, 4), "scan_bytes": by // nl, "scan_tb_s": round(tb, 3), "frac": round(tb / HBM_PEAK_TB_S, 3)}

    for w in wanted:
        fn = lambda w=w: idx.search_range_arrays(q, thr[w], 0, limit=w + 8)  # noqa: E731
        ts = time_calls(fn, args.calls)
        _, _, total = fn()
        scan = idx.last_scan()
        emit({"what": "range", "rows": n, "dim": dim, "qualifying": total, "path": V.last_path(), "scan_variant": scan["variant"],
              "scan_grid": scan["grid"], **stats(ts), **scan_profile(fn)})
        ts = time_calls(lambda w=w: idx.search_range_arrays(q, thr[w], 0, limit=0), args.calls)
        emit({"what": "range_count_only", "rows": n, "dim": dim, "qualifying": total, **stats(ts)})

    for frac in (0.01, 0.1):
        m = max(1, int(round(n * frac)))
        keep = rng.choice(n, size=m, replace=False).astype(np.uint64)
        with idx.make_filter(keep) as f:
            _, ftop = idx.search_arrays(q, 10, 0, filter=f)
            t = float(ftop[-1])
            fn = lambda: idx.search_range_arrays(q, t, 0, filter=f, limit=64)  # noqa: E731
            ts = time_calls(fn, args.calls)
            _, _, total = fn()
            scan = idx.last_scan()
            emit({"what": "range_filtered", "rows": n, "dim": dim, "fraction": frac, "subset_rows": m, "qualifying": total,
                  "path": V.last_path(), "scan_variant": scan["variant"], "scan_grid": scan["grid"], **stats(ts), **scan_profile(fn)})
    fh.close()


if __name__ == "__main__":
    main()

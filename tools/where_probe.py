"""Predicate filter tokens on the headline index (10 M x 384 cosine unit rows by default, k = 10), everything on ONE handle and
alternated call by call:

  a  per kept fraction: creation time of a predicate token over one int64 column (median of 5), its re-resolution after a
     mutation (the column's, then the predicate's alone), against make_filter over the same row set (the id route:
     profiles/filtered_<n>x<dim>.jsonl's creation times);
  b  per kept fraction, for the int8-first ladder (the default at this size) and the bf16-first one: the median single
     search under the predicate token with the route forced to "list", to "mask" and left on "auto", and (at the fractions of
     a) under the include token of the same rows -- closely spaced between 10 % and 60 % kept, to read the crossover that
     csrc/where_plan.hpp derives from byte counts;
  c  a 256-query batch under one predicate token against the same batch under the exclusion token of the complement.

One JSON line per measurement on stdout and in profiles/where_<n>x<dim>.jsonl.

    python tools/where_probe.py [--rows 10000000] [--dim 384] [--queries 60]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(ts):
    return round(float(np.median(np.asarray(ts)) * 1e3), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--queries", type=int, default=60)
    ap.add_argument("--create-fractions", default="0.0001,0.01,0.1,0.5,1.0")
    ap.add_argument("--search-fractions", default="0.0001,0.01,0.05,0.1,0.15,0.2,0.25,0.3,0.35,0.4,0.45,0.5,0.55,0.6,0.75,1.0")
    ap.add_argument("--batch-fractions", default="0.01,0.1,0.5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim = args.rows, args.dim
    out_path = args.out or os.path.join(ROOT, "profiles", f"where_{n}x{dim}.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    fh = open(out_path, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        fh.write(line + "\n")
        fh.flush()

    os.environ.pop("VL_SINGLE_FILTER", None)
    idx = V.FlatIndex(dim)  # default ladder
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
    Q = rng.standard_normal((max(args.queries, 256), dim))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    all_ids = np.arange(n, dtype=np.uint64)
    values = rng.permutation(n).astype(np.int64)  # value < f n keeps exactly the share f, at random positions

    t0 = time.perf_counter()
    col = idx.make_attribute(all_ids, values)
    emit({"what": "column_create", "rows": n, "pairs": n, "create_ms": round((time.perf_counter() - t0) * 1e3, 3),
          "device_bytes": {"pairs": 16 * n, "value_of_row": 8 * n, "has_bitmap": 8 * ((n + 63) // 64)}})
    bound = lambda f: max(int(round(f * n)), 1) - 1  # hi of the clause [0, hi]

    # ---- a: creation and re-resolution against the id route --------------------------------------------------------
    for f in [float(x) for x in args.create_fractions.split(",")]:
        hi = bound(f)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            w = idx.make_filter_where([(col, 0, hi)])
            ts.append(time.perf_counter() - t0)
            m = w.rows()
            w.close()
        w = idx.make_filter_where([(col, 0, hi)])
        kept_ids = all_ids[values <= hi]
        t0 = time.perf_counter()
        inc = idx.make_filter(kept_ids)
        t_inc = time.perf_counter() - t0
        assert inc.rows() == m == kept_ids.size
        idx.add_rows(np.array([n + 1], dtype=np.uint64), Q[:1], validate=False)  # one mutation: everything is stale
        t0 = time.perf_counter()
        col.rows()
        t_col = time.perf_counter() - t0
        t0 = time.perf_counter()
        w.rows()
        t_pred = time.perf_counter() - t0
        t0 = time.perf_counter()
        inc.rows()
        t_inc_re = time.perf_counter() - t0
        idx.delete(n + 1)
        t0 = time.perf_counter()
        idx.search_arrays(Q[0], 10, 0, filter=w)  # resolves column and predicate, then answers
        t_first = time.perf_counter() - t0
        emit({"what": "where_create", "rows": n, "dim": dim, "kept_fraction": f, "qualifying": m,
              "where_create_ms": median_ms(ts), "include_create_ms": round(t_inc * 1e3, 3),
              "column_reresolve_ms": round(t_col * 1e3, 3), "where_reresolve_ms": round(t_pred * 1e3, 3),
              "include_reresolve_ms": round(t_inc_re * 1e3, 3), "first_search_after_mutation_ms": round(t_first * 1e3, 3),
              "where_token_bytes": {"chunk_offsets": 4 * 1025, "bitmap": 8 * ((n + 63) // 64)}, "list_bytes_on_demand": 4 * m,
              "include_token_bytes": 8 * m + 4 * 1025 + 4 * m})
        w.close()
        inc.close()

    # ---- b: single searches, list against mask against auto -------------------------------------------------------
    create_set = {float(x) for x in args.create_fractions.split(",")}
    nq = args.queries
    for ladder in ("auto", "bf16"):  # auto at this size: the int8 copy first; "bf16": the bf16 copy first
        idx.set_single_filter(ladder)
        for f in [float(x) for x in args.search_fractions.split(",")]:
            hi = bound(f)
            w = idx.make_filter_where([(col, 0, hi)])
            m = w.rows()
            inc = idx.make_filter(all_ids[values <= hi]) if f in create_set else None

            def call(route):
                def fn(q):
                    idx.set_where_route(route)
                    return idx.search_arrays(q, 10, 0, filter=w)
                return fn

            calls = {"list": call("list"), "mask": call("mask"), "auto": call("auto")}
            if inc is not None:
                calls["include"] = lambda q: idx.search_arrays(q, 10, 0, filter=inc)
            ts = {name: [] for name in calls}
            info = {}
            for q in Q[:10]:
                for fn in calls.values():
                    fn(q)
            for q in Q[:nq]:  # alternated call by call on the one handle
                for name, fn in calls.items():
                    t0 = time.perf_counter()
                    fn(q)
                    ts[name].append(time.perf_counter() - t0)
            for name in ("list", "mask", "auto"):
                calls[name](Q[0])
                info[name] = {"route": idx.last_where()["route"], "scan_variant": idx.last_scan()["variant"], "path": V.last_path()}
            rec = {"what": "where_search", "rows": n, "dim": dim, "k": 10, "ladder": "i8_first" if ladder == "auto" else "bf16_first",
                   "kept_fraction": f, "qualifying": m, "queries": nq}
            for name in calls:
                rec[name + "_median_ms"] = median_ms(ts[name])
            rec["routes"] = info
            rec["auto_took"] = "mask" if info["auto"]["route"] else "list"
            rec["faster"] = "mask" if rec["mask_median_ms"] < rec["list_median_ms"] else "list"
            emit(rec)
            w.close()
            if inc is not None:
                inc.close()
    idx.set_single_filter("auto")
    idx.set_where_route("auto")

    # ---- c: a 256-query batch, predicate token against the exclusion token of the complement ----------------------
    QB = Q[:256]
    for f in [float(x) for x in args.batch_fractions.split(",")]:
        hi = bound(f)
        w = idx.make_filter_where([(col, 0, hi)])
        ex = idx.make_filter(all_ids[values > hi], exclude=True)
        assert w.rows() == ex.rows()
        calls = {"where": lambda: idx.search_batch(QB, 10, 0, filter=w), "exclude": lambda: idx.search_batch(QB, 10, 0, exclude=ex)}
        ts = {name: [] for name in calls}
        routed = {}
        for fn in calls.values():
            fn()
        for _ in range(3):
            for name, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                ts[name].append(time.perf_counter() - t0)
                routed[name] = idx.last_masked_batch()
        emit({"what": "where_batch", "rows": n, "dim": dim, "k": 10, "queries": 256, "kept_fraction": f, "qualifying": w.rows(),
              "where_median_ms": median_ms(ts["where"]), "exclude_median_ms": median_ms(ts["exclude"]),
              "where_masked_batch": routed["where"], "exclude_masked_batch": routed["exclude"]})
        w.close()
        ex.close()
    emit({"what": "where_counters", **idx.last_where()})
    col.close()
    fh.close()


if __name__ == "__main__":
    main()

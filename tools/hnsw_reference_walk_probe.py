#!/usr/bin/env python3
"""What reference navigation (HNSWIndex.set_navigation("reference"): k_hnsw_search_ref) costs and gives, beside the
default f32 walk (k_hnsw_search) and the CPU walker (oracle/vl_hnsw_cpu.c, one core) on the SAME graph.

Data: 1 M x 384 cosine rows, default build (M 16, M0 32, ef_construction 400), two distributions (latent16, clustered;
as tools/hnsw_efc_sweep.py).  Per (distribution, ef in 10 / 32 / 128) and walk: recall@10 against the exhaustive order of
the reference's u64 distances (ties at the 10th accepted), distance evaluations per query, QPS of a 1000-query batch,
the median latency of a lone query; for the reference walk also how many queries returned exactly the CPU walker's
nodes.  ef 10 is the trait's own search (ef = min(k, len)); 32 / 128 name the ef (vl_index_search_ef).

  python tools/hnsw_reference_walk_probe.py [--rows N] [--out profiles/hnsw_reference_walk_1m_d384.jsonl]
  python tools/hnsw_reference_walk_probe.py --kernels               # walks only: run under rocprofv3 --kernel-trace --stats
  python tools/hnsw_reference_walk_probe.py --kernel-stats DB --out F  # append the walk kernels' times from that run's database
"""
import argparse
import json
import os
import re
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
DEFAULT_OUT = os.path.join(ROOT, "profiles", "hnsw_reference_walk_1m_d384.jsonl")
EFS = (10, 32, 128)
K = 10


def build(torch, kind, rows, dim, with_flat):
    import vectorlite_amd as V
    from hnsw_efc_sweep import gen
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    state = {}
    flat = None
    if with_flat:
        flat = V.FlatIndex(dim)
        flat.reserve(rows)
    hn = V.HNSWIndex(dim, 0)
    t_build, done = 0.0, 0
    while done < rows:
        c = min(250_000, rows - done)
        x = gen(torch, dev, g, kind, c, dim, state)
        ids = np.arange(done, done + c, dtype=np.uint64)
        if flat is not None:
            flat.add_rows(ids, x, validate=False)
        t0 = time.perf_counter()
        hn.add_rows(ids, x)
        t_build += time.perf_counter() - t0
        done += c
        del x
    Q = gen(torch, dev, g, kind, 1000, dim, state).cpu().numpy()
    return hn, flat, Q, t_build


def measure(a):
    import torch
    from oracle import oracle as O
    O.build()
    out = open(a.out, "w")
    for kind in a.kinds.split(","):
        hn, flat, Q, t_build = build(torch, kind, a.rows, a.dim, True)
        nq, n_truth = len(Q), a.truth_queries
        allpos = np.arange(a.rows, dtype=np.uint64)
        D = [flat.hnsw_distances(Q[i], allpos, 0) for i in range(n_truth)]
        kth = [np.partition(d, K - 1)[K - 1] for d in D]
        del flat
        torch.cuda.empty_cache()

        def recall(rows_):
            return float(np.mean([sum(1 for x in rows_[i] if D[i][int(x)] <= kth[i]) / float(K) for i in range(n_truth)]))

        walker = O.HnswCpuWalker(hn.graph(with_rows=True), O.COSINE)
        for ef in EFS:
            cell = {"data": kind, "rows": a.rows, "dim": a.dim, "metric": "cosine", "build_s": round(t_build, 2), "ef": ef,
                    "k": K, "batch_queries": nq, "recall_queries": n_truth}
            e_arg = 0 if ef == K else ef
            for mode in ("f32", "reference"):
                hn.set_navigation(mode)
                hn.search_batch(Q[:8], K, 0, ef=e_arg)
                q0, e0 = hn.walk_stats()
                t0 = time.perf_counter()
                bi, _, bn = hn.search_batch(Q, K, 0, ef=e_arg)
                dt = time.perf_counter() - t0
                q1, e1 = hn.walk_stats()
                lat = []
                for i in range(31):
                    t1 = time.perf_counter()
                    hn.search_arrays(Q[i], K, 0, ef=e_arg)
                    lat.append(time.perf_counter() - t1)
                r = {"recall_at_10": round(recall([bi[i, :int(bn[i])] for i in range(n_truth)]), 4),
                     "distance_evals_per_query": round((e1 - e0) / max(q1 - q0, 1), 1),
                     "batch_queries_per_s": round(nq / dt, 0), "lone_query_ms_median": round(float(np.median(lat)) * 1e3, 4)}
                if mode == "reference":
                    w0 = walker.evals.value
                    t0 = time.perf_counter()
                    cw = [walker.search(Q[i], ef, K) for i in range(n_truth)]
                    t_cpu = (time.perf_counter() - t0) / n_truth
                    r["same_nodes_as_cpu_walker"] = int(sum(bi[i, :int(bn[i])].tolist() == cw[i][0].tolist() for i in range(n_truth)))
                    cell["cpu_walker"] = {
                        "cores": 1, "recall_at_10": round(recall([c[0] for c in cw]), 4),
                        "distance_evals_per_query": round((walker.evals.value - w0) / n_truth, 1),
                        "queries_per_s": round(1.0 / t_cpu, 1), "lone_query_ms": round(t_cpu * 1e3, 4)}
                cell[f"gpu_{mode}"] = r
            hn.set_navigation("f32")
            print(json.dumps(cell), flush=True)
            out.write(json.dumps(cell) + "\n")
        del walker, hn
        torch.cuda.empty_cache()
    out.close()


def kernels(a):
    """Walk batches only (one kind): ef 10 and 128, both navigations, five 1000-query batches each."""
    import torch
    hn, _, Q, _ = build(torch, a.kinds.split(",")[0], a.rows, a.dim, False)
    for ef in (10, 128):
        for mode in ("f32", "reference"):
            hn.set_navigation(mode)
            for _ in range(5):
                hn.search_batch(Q, K, 0, ef=0 if ef == K else ef)
    torch.cuda.synchronize()
    print("kernels done", flush=True)


def kernel_stats(a):
    """Per walk kernel instantiation: dispatches and time (the search kernels' slots template argument tells the ef:
    S = 1 for ef <= 64, 2 for ef <= 128)."""
    def key(name):
        m = re.search(r"(k_hnsw_search(?:_ref)?)\D*?\d\D+(\d)", name)  # <METRIC, S> demangled or ILi..ELi..E mangled
        return (m.group(1), int(m.group(2))) if m else None

    per = {}  # (kernel, slots) -> (dispatches, mean, min, max) in us
    if a.kernel_stats.endswith(".csv"):  # rocprofv3 --stats' kernel_stats.csv
        import csv
        for r in csv.DictReader(open(a.kernel_stats)):
            kk = key(r["Name"])
            if kk:
                per[kk] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3)
    else:                                # the rocpd database
        c = sqlite3.connect(a.kernel_stats)
        tables = [r[0] for r in c.execute("select name from sqlite_master where type in ('table', 'view')")]
        table = "kernels" if "kernels" in tables else next(t for t in tables if "kernel" in t.lower())
        ts = {}
        for name, s, e in c.execute(f"select name, start, end from {table}"):
            kk = key(name)
            if kk:
                ts.setdefault(kk, []).append((e - s) / 1e3)
        per = {kk: (len(v), float(np.mean(v)), float(np.min(v)), float(np.max(v))) for kk, v in ts.items()}
    with open(a.out, "a") as out:
        for (kern, slots), (n, mean, lo, hi) in sorted(per.items()):
            line = {"rocprofv3_kernel": kern, "slots": slots, "ef": 10 if slots == 1 else 128, "rows": a.rows,
                    "dim": a.dim, "batch_queries": 1000, "dispatches": n, "mean_us": round(mean, 1),
                    "min_us": round(lo, 1), "max_us": round(hi, 1)}
            print(json.dumps(line))
            out.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--kinds", default="latent16,clustered")
    ap.add_argument("--truth-queries", type=int, default=200)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-stats", default="")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a)
    elif a.kernels:
        kernels(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()

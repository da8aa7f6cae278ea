#!/usr/bin/env python3
"""The single-query bf16 filter on one GPU: launch shapes of k_scan_bf16, and the f32 / bf16 crossover in index size.

  --what shapes     every k_scan_bf16 shape listed for the row stride (VL_SCAN16_SHAPE "G,VPL,U") x workgroups per CU
                    (VL_SCAN16_BPC), scan time per launch from HIP events, interleaved rounds in ONE process; the f32
                    k_scan of the same index alongside.  Run it under `rocprofv3 --kernel-trace --stats` for kernel times.
  --what crossover  ONE index grown through --sizes: at each size, back-to-back single searches with the f32 scan
                    ("f32") and with the bf16 filter first ("bf16"), interleaved rounds; per-search wall time.
  --what clustered  rows in tight clusters (--clusters, --noise): the auto mode's fallback rate and per-search cost
                    against the f32-only mode where the bf16 bound rarely certifies.

One JSON object per line on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {48: ["8,6,1", "8,6,2"], 96: ["16,6,1", "16,6,2"],
          16: ["8,2,1", "8,2,2"], 32: ["8,4,1", "8,4,2"], 64: ["8,8,1", "8,8,2"]}


def grow(idx, torch, dev, dim, lo, hi, seed=1234, chunk=500_000):
    done = lo
    while done < hi:
        c = min(chunk, hi - done)
        g = torch.Generator(device=dev)
        g.manual_seed(seed + done)
        x = torch.randn((c, dim), dtype=torch.float64, device=dev, generator=g)
        x /= torch.linalg.vector_norm(x, dim=1, keepdim=True)
        idx.add_rows(np.arange(done, done + c, dtype=np.uint64), x, validate=False)
        done += c
    torch.cuda.synchronize()


def queries(dim, nq, seed=99):
    q = np.random.default_rng(seed).standard_normal((nq, dim))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def timed_launches(idx, Q, metric, reps):
    """(ms per scan launch from HIP events, launches, searches)."""
    idx.profile_read()
    idx.profile_enable(True)
    for i in range(reps):
        idx.search_arrays(Q[i % len(Q)], 10, metric)
    idx.profile_enable(False)
    nl, ms, _ = idx.profile_read()
    return ms / max(nl, 1), nl, reps


def shapes(a, V, torch, dev):
    idx = V.FlatIndex(a.dim)
    idx.reserve(a.rows)
    grow(idx, torch, dev, a.dim, 0, a.rows)
    Q = queries(a.dim, 64)
    ldb = next(s for s in (128, 256, 384, 512, 768) if a.dim <= s)
    bf16_bytes, f32_bytes = a.rows * ldb * 2, a.rows * ((a.dim + 3) // 4 * 4) * 4
    cands = [(s, b) for s in SHAPES[ldb // 8] for b in a.bpc.split(",")]
    res = {c: [] for c in cands}
    res_f32 = []
    idx.set_single_filter("bf16")
    idx.search_arrays(Q[0], 10, a.metric)  # builds the bf16 copy
    for r in range(a.rounds):
        for s, b in cands:
            os.environ["VL_SCAN16_SHAPE"], os.environ["VL_SCAN16_BPC"] = s, b
            idx.set_single_filter("bf16")
            timed_launches(idx, Q, a.metric, 3)
            ms, nl, ns = timed_launches(idx, Q, a.metric, a.per_round)
            res[(s, b)].append((ms, nl, ns, idx.last_scan()))
        idx.set_single_filter("f32")
        timed_launches(idx, Q, a.metric, 3)
        res_f32.append(timed_launches(idx, Q, a.metric, a.per_round)[0])
    os.environ.pop("VL_SCAN16_SHAPE")
    os.environ.pop("VL_SCAN16_BPC")
    for (s, b), v in res.items():
        med = statistics.median(x[0] for x in v)
        print(json.dumps({"what": "shape", "rows": a.rows, "dim": a.dim, "metric": a.metric, "shape_g_vpl_u": s, "bpc": int(b),
                          "variant": v[-1][3], "ms_per_launch_median": round(med, 4),
                          "ms_per_launch_rounds": [round(x[0], 4) for x in v],
                          "launches_per_search": round(sum(x[1] for x in v) / sum(x[2] for x in v), 3),
                          "GBps_on_bf16_bytes": round(bf16_bytes / (med * 1e-3) / 1e9, 1)}), flush=True)
    med = statistics.median(res_f32)
    print(json.dumps({"what": "f32_k_scan", "rows": a.rows, "dim": a.dim, "metric": a.metric, "variant": idx.last_scan(),
                      "ms_per_launch_median": round(med, 4), "ms_per_launch_rounds": [round(x, 4) for x in res_f32],
                      "GBps": round(f32_bytes / (med * 1e-3) / 1e9, 1)}), flush=True)


def crossover(a, V, torch, dev):
    sizes = [int(x) for x in a.sizes.split(",")]
    idx = V.FlatIndex(a.dim)
    idx.reserve(sizes[-1])
    Q = queries(a.dim, 256)
    have = 0
    for n in sizes:
        grow(idx, torch, dev, a.dim, have, n)
        have = n
        wall = {"f32": [], "bf16": []}
        for mode in ("bf16", "f32"):  # warm: the bf16 copy's new rows, both code paths
            idx.set_single_filter(mode)
            for i in range(20):
                idx.search_arrays(Q[i], 10, a.metric)
        for r in range(a.rounds):
            for mode in ("f32", "bf16") if r % 2 == 0 else ("bf16", "f32"):
                idx.set_single_filter(mode)
                t = time.perf_counter()
                for i in range(a.per_round):
                    idx.search_arrays(Q[i % len(Q)], 10, a.metric)
                wall[mode].append((time.perf_counter() - t) / a.per_round * 1e3)
        f, b = statistics.median(wall["f32"]), statistics.median(wall["bf16"])
        print(json.dumps({"what": "crossover", "rows": n, "dim": a.dim, "metric": a.metric,
                          "f32_slab_MiB": round(n * ((a.dim + 3) // 4 * 4) * 4 / 2 ** 20, 1),
                          "ms_per_search_f32": round(f, 4), "ms_per_search_bf16": round(b, 4), "bf16_over_f32": round(b / f, 3),
                          "rounds_f32": [round(x, 4) for x in wall["f32"]], "rounds_bf16": [round(x, 4) for x in wall["bf16"]]}),
              flush=True)


def clustered(a, V, torch, dev):
    """Rows in tight clusters (centres + noise of --noise per unit row): neighbourhoods denser than bf16 resolves.  Auto
    mode against the f32-only mode: per-search wall time, and how many searches took the bf16 pass / also the f32 one
    (profile bytes per search = a x n x ldb x 2 + b x n x ld x 4)."""
    n, dim = a.rows, a.dim
    ld, ldb = (dim + 3) // 4 * 4, next(s for s in (128, 256, 384, 512, 768) if dim <= s)
    idx = V.FlatIndex(dim)
    idx.reserve(n)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    C = torch.randn((a.clusters, dim), dtype=torch.float64, device=dev, generator=g)
    C /= torch.linalg.vector_norm(C, dim=1, keepdim=True)
    done = 0
    while done < n:
        c = min(500_000, n - done)
        x = C[torch.randint(0, a.clusters, (c,), device=dev, generator=g)]
        x = x + a.noise / dim ** 0.5 * torch.randn((c, dim), dtype=torch.float64, device=dev, generator=g)
        x /= torch.linalg.vector_norm(x, dim=1, keepdim=True)
        idx.add_rows(np.arange(done, done + c, dtype=np.uint64), x, validate=False)
        done += c
    torch.cuda.synchronize()
    Cq = C[:256].cpu().numpy()
    Q = Cq + a.noise / dim ** 0.5 * np.random.default_rng(5).standard_normal(Cq.shape)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    out = {}
    for mode in ("f32", "auto"):
        idx.set_single_filter(mode)
        for i in range(8):
            idx.search_arrays(Q[i], 10, a.metric)
        idx.set_single_filter(mode)  # a fresh window for the timed queries
        idx.profile_read()
        idx.profile_enable(True)
        t = time.perf_counter()
        res = [idx.search_arrays(Q[i % len(Q)], 10, a.metric) for i in range(a.per_round)]
        t = time.perf_counter() - t
        idx.profile_enable(False)
        nl, ms, by = idx.profile_read()
        f32_l = (by - nl * n * ldb * 2) // (n * ld * 4 - n * ldb * 2)  # launches = bf16 + f32, bytes as above
        out[mode] = {"ms_per_search": round(t / a.per_round * 1e3, 4), "launches": nl, "bf16_passes": nl - f32_l,
                     "f32_passes": f32_l, "answers": [(r[0].tolist(), r[1].tolist()) for r in res]}
    au = out["auto"]
    fails = au["bf16_passes"] + au["f32_passes"] - a.per_round  # searches that paid both passes
    print(json.dumps({"what": "clustered", "rows": n, "dim": dim, "metric": a.metric, "clusters": a.clusters, "noise": a.noise,
                      "searches": a.per_round, "ms_per_search_f32": out["f32"]["ms_per_search"],
                      "ms_per_search_auto": au["ms_per_search"], "auto_bf16_passes": au["bf16_passes"],
                      "auto_f32_passes": au["f32_passes"], "auto_bf16_not_certified": fails,
                      "auto_fallback_rate_of_bf16_tries": round(fails / max(au["bf16_passes"], 1), 3),
                      "same_answers": out["f32"]["answers"] == au["answers"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("shapes", "crossover", "clustered"), required=True)
    ap.add_argument("--clusters", type=int, default=2000)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--metric", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--bpc", default="2,3,4")
    ap.add_argument("--sizes", default="100000,200000,350000,500000,750000,1000000,2000000")
    a = ap.parse_args()
    import torch
    import vectorlite_amd as V
    dev = torch.device("cuda", 0)
    {"shapes": shapes, "crossover": crossover, "clustered": clustered}[a.what](a, V, torch, dev)


if __name__ == "__main__":
    main()

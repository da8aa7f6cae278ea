#!/usr/bin/env python3
"""HNSW graph import against the rebuild it replaces, on the same box in the same run: build (add_rows), export, import
(host validation, row ingest, uploads, edge-key kernel, in-degree kernel), snapshot save / load and the file's size.
Rows are latent-16 like tools/hnsw_eval.py --latent 16.  Appends one JSON line to profiles/hnsw_import_<rows>_d<dim>.jsonl."""
import argparse, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def label(rows):
    return f"{rows // 1_000_000}m" if rows % 1_000_000 == 0 else (f"{rows // 1000}k" if rows % 1000 == 0 else str(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--metric", type=int, default=0)
    ap.add_argument("--efc", type=int, default=400)
    ap.add_argument("--latent", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", f"hnsw_import_{label(a.rows)}_d{a.dim}.jsonl")
    import torch
    import vectorlite_amd as V
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(1234)
    A = torch.randn((a.latent, a.dim), dtype=torch.float64, device=dev, generator=g)
    hn = V.HNSWIndex(a.dim, a.metric, ef_construction=a.efc)
    t_build, done = 0.0, 0
    while done < a.rows:
        c = min(250_000, a.rows - done)
        x = torch.randn((c, a.latent), dtype=torch.float64, device=dev, generator=g) @ A
        x += 0.05 * torch.randn((c, a.dim), dtype=torch.float64, device=dev, generator=g)
        x /= torch.linalg.vector_norm(x, dim=1, keepdim=True)
        ids = np.arange(done, done + c, dtype=np.uint64)
        t0 = time.perf_counter(); hn.add_rows(ids, x); t_build += time.perf_counter() - t0
        done += c
    del x
    rec = {"rows": a.rows, "dim": a.dim, "metric": a.metric, "ef_construction": a.efc, "latent": a.latent, "build_s": round(t_build, 3)}
    t0 = time.perf_counter(); gr = hn.graph(with_rows=True); rec["export_s"] = round(time.perf_counter() - t0, 3)
    rec["n_upper"] = int(gr["cntU"].size)
    rec["edges"] = int(gr["cnt0"].sum() + gr["cntU"].sum())
    p = hn.params()
    t0 = time.perf_counter(); imp = V.HNSWIndex.from_graph(gr, a.dim, a.metric, **p); rec["import_s"] = round(time.perf_counter() - t0, 3)
    rec.update({k: round(v, 3) for k, v in imp.import_times().items()})
    # what from_graph spends outside the library: creating the handle and the level-law check in numpy
    rec["import_python_ms"] = round(rec["import_s"] * 1e3 - sum(imp.import_times().values()), 3)
    rng = np.random.default_rng(4321)
    Q = rng.standard_normal((64, a.latent)) @ A.cpu().numpy() + 0.05 * rng.standard_normal((64, a.dim))
    same = all(x.tobytes() == y.tobytes() for x, y in zip(hn.search_batch(Q, 10, a.metric, ef=64), imp.search_batch(Q, 10, a.metric, ef=64)))
    rec["same_answers_64_queries_ef64"] = bool(same)
    del imp, gr
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "snapshot.npz")
        t0 = time.perf_counter(); hn.save_snapshot(path); rec["snapshot_save_s"] = round(time.perf_counter() - t0, 3)
        rec["snapshot_bytes"] = os.path.getsize(path)
        t0 = time.perf_counter(); back = V.HNSWIndex.load_snapshot(path); rec["snapshot_load_s"] = round(time.perf_counter() - t0, 3)
        rec["snapshot_len"] = back.len()
    rec["import_vs_build"] = round(rec["build_s"] / rec["import_s"], 1)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

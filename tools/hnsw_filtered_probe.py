#!/usr/bin/env python3
"""Id-filtered HNSW walks on latent-16 cosine rows like tools/hnsw_eval.py --latent 16: per beam
width and pass fraction -- 1, 0.5, 0.1, just above and just below the route boundary ef * n = 256 * n_pass, 0.001 --
recall@10 against the exact order of the passing rows, evaluations per query, the route, the list capacity and the walks it
cut, QPS in 1000-query batches and the latency of a lone query; beside them over-fetch-and-discard on the unfiltered walk
at the same beam.  The cell just below the boundary IS the exact route's baseline.  Appends JSON lines to
profiles/hnsw_filtered_<rows>_d<dim>.jsonl.

--unfiltered-only measures nothing but unfiltered 1000-query batches at ef 10 and 128 and prints one line: run it
alternately with --package-root pointing at a build of the parent commit and at this tree to compare the two."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def label(rows):
    return f"{rows // 1_000_000}m" if rows % 1_000_000 == 0 else (f"{rows // 1000}k" if rows % 1000 == 0 else str(rows))


def timed_batches(fn, repeat):
    fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--efc", type=int, default=400)
    ap.add_argument("--latent", type=int, default=16)
    ap.add_argument("--efs", default="10,32,128")
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--recall-queries", type=int, default=100)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--unfiltered-only", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    out = a.out or os.path.join(ROOT, "profiles", f"hnsw_filtered_{label(a.rows)}_d{a.dim}.jsonl")
    import torch
    import vectorlite_amd as V
    metric, k, n = 0, 10, a.rows
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(1234)
    A = torch.randn((a.latent, a.dim), dtype=torch.float64, device=dev, generator=g)
    hn = V.HNSWIndex(a.dim, metric, ef_construction=a.efc)
    chunks, done, t_build = [], 0, 0.0
    while done < n:
        c = min(250_000, n - done)
        x = torch.randn((c, a.latent), dtype=torch.float64, device=dev, generator=g) @ A
        x += 0.05 * torch.randn((c, a.dim), dtype=torch.float64, device=dev, generator=g)
        x /= torch.linalg.vector_norm(x, dim=1, keepdim=True)
        t0 = time.perf_counter(); hn.add_rows(np.arange(done, done + c, dtype=np.uint64), x); t_build += time.perf_counter() - t0
        chunks.append(x.to(torch.float32))
        done += c
    X32 = torch.cat(chunks); del chunks, x
    rng = np.random.default_rng(4321)
    Q = rng.standard_normal((a.batch, a.latent)) @ A.cpu().numpy() + 0.05 * rng.standard_normal((a.batch, a.dim))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    lines = []

    def emit(rec):
        rec = dict({"rows": n, "dim": a.dim, "ef_construction": a.efc, "latent": a.latent, "tag": a.tag}, **rec)
        line = json.dumps(rec); print(line, flush=True); lines.append(line)

    efs = [int(e) for e in a.efs.split(",")]
    if a.unfiltered_only:
        rec = {"kind": "unfiltered", "build_s": round(t_build, 2)}  # --tag says which build this was
        for ef in (10, 128):
            s = timed_batches(lambda: hn.search_batch(Q, k, metric, ef=ef), 7)
            rec[f"qps_ef{ef}"] = round(a.batch / s)
        emit(rec)
    else:
        nr = a.recall_queries
        sims = torch.from_numpy(Q[:nr]).to(dev, torch.float32) @ X32.T          # [nr, n]; f32 is enough to rank the truth
        for ef in efs:
            edge = -(-ef * n // 256)                                                # smallest n_pass that still walks
            counts = [("1", n), ("0.5", n // 2), ("0.1", n // 10), ("above_boundary", edge + edge // 50),
                      ("below_boundary", edge - max(edge // 50, 1)), ("0.001", n // 1000)]
            for name, n_pass in counts:
                n_pass = min(n_pass, n)
                ids = np.sort(rng.choice(n, n_pass, replace=False)).astype(np.uint64)
                t0 = time.perf_counter(); wf = hn.make_walk_filter(ids); t_make = time.perf_counter() - t0
                mask = torch.zeros(n, dtype=torch.bool, device=dev); mask[torch.from_numpy(ids.astype(np.int64)).to(dev)] = True
                truth = torch.topk(sims.masked_fill(~mask[None, :], -2.0), k, dim=1).indices.cpu().numpy()
                e0 = hn.walk_stats()[1]
                got, _, cnt = hn.search_batch(Q[:nr], k, metric, ef=ef, filter=wf)
                evals = (hn.walk_stats()[1] - e0) / nr
                last = hn.last_filtered()
                recall = float(np.mean([len(set(truth[i].tolist()) & set(got[i, :int(cnt[i])].tolist())) / k for i in range(nr)]))
                s_batch = timed_batches(lambda: hn.search_batch(Q, k, metric, ef=ef, filter=wf), 5)
                cut_batch = hn.last_filtered()["cap_cut_walks"]
                lone = [0.0] * 30
                for j in range(30):
                    t0 = time.perf_counter(); hn.search_arrays(Q[j], k, metric, ef=ef, filter=wf); lone[j] = time.perf_counter() - t0
                # over-fetch and discard on the unfiltered walk: ask for enough neighbours to expect k passing ones
                fetch = int(min(512, max(k, -(-k * n // n_pass))))
                passing = np.zeros(n, bool); passing[ids.astype(np.int64)] = True

                def overfetch(qs):
                    i2, _, c2 = hn.search_batch(qs, fetch, metric, ef=max(ef, fetch))
                    return [[v for v in i2[r, :int(c2[r])].tolist() if passing[v]][:k] for r in range(len(qs))]
                of = overfetch(Q[:nr])
                recall_of = float(np.mean([len(set(truth[i].tolist()) & set(of[i])) / k for i in range(nr)]))
                s_of = timed_batches(lambda: overfetch(Q), 3)
                emit({"kind": "filtered", "ef": ef, "fraction": name, "n_pass": int(n_pass), "route": last["route"], "cap": last["cap"],
                      "recall_at_10": round(recall, 4), "evals_per_query": round(evals, 1), "cut_walks_of_batch": int(cut_batch),
                      "qps_batch": round(a.batch / s_batch), "lone_query_ms": round(float(np.median(lone)) * 1e3, 4),
                      "filter_create_ms": round(t_make * 1e3, 2), "overfetch_k": fetch, "overfetch_recall_at_10": round(recall_of, 4),
                      "overfetch_qps_batch": round(a.batch / s_of)})
                wf.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Late-interaction (MaxSim) search on 10 M x 128 unit rows, ~100 consecutive rows per group, 32 query tokens, k = 10: per
record three calls, alternated call by call in one process on one handle --
  (a) search_maxsim_arrays (the MFMA candidate pass and its certification);
  (b) the same call on the forced exact route (one exact scan per token): the answers must be equal bit for bit;
  (c) the loop a caller ran before: one search_grouped_arrays per token with k = 1024, the most a call returns, summed on
      the host.  With 100 000 groups that loop only knows a group's score when the group made every token's best 1024
      (`loop_complete_groups`, usually none): it is timed as the by-hand alternative, it is not an answer.
The tokens are noisy copies of rows of three groups.  Wall time per call (median of --reps), the route and the survivor
counts of last_maxsim().  One JSON line per record on stdout and in profiles/maxsim_<n>x<dim>.jsonl.

    python tools/maxsim_probe.py [--rows 10000000] [--dim 128] [--tokens 32] [--reps 3]
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
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--per-group", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vectorlite_amd as V

    n, dim, k, T = args.rows, args.dim, 10, args.tokens
    out_path = args.out or os.path.join(ROOT, "profiles", f"maxsim_{n}x{dim}.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)

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
    ids = np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(2)

    with open(out_path, "w") as fh, idx.make_groups(ids, ids // np.uint64(args.per_group)) as table:
        for metric in (0, 1, 3):
            src = np.concatenate([rng.integers(t * args.per_group, (t + 1) * args.per_group, size=T // 3 + 1) for t in (7, 1234, n // args.per_group - 1)])[:T]
            Q = np.array([idx.get_vector(int(i)).values for i in src]) + 0.1 * rng.standard_normal((T, dim)) / np.sqrt(dim)
            keys, scores = idx.search_maxsim_arrays(Q, k, metric, groups=table)  # warm: the bf16 copy, the workspace
            rec = {"rows": n, "dim": dim, "tokens": T, "k": k, "metric": metric, "groups": table.distinct(), "report": idx.last_maxsim()}
            t_new, t_loop, t_exact = [], [], []
            for _ in range(args.reps):  # alternated call by call
                idx.force_path(V.PATH_EXACT_SORT)
                te = time.perf_counter()
                ekeys, escores = idx.search_maxsim_arrays(Q, k, metric, groups=table)
                t_exact.append(time.perf_counter() - te)
                rec["exact_route"] = idx.last_maxsim()["route"]
                idx.force_path(V.PATH_NONE)
                t0 = time.perf_counter()
                idx.search_maxsim_arrays(Q, k, metric, groups=table)
                t1 = time.perf_counter()
                total = {}
                for q in Q:
                    gk, _, gs = idx.search_grouped_arrays(q, V.VL_GROUPED_MAX_K, metric, groups=table)
                    for key, s in zip(gk.tolist(), gs.tolist()):
                        total.setdefault(key, []).append(s)
                t2 = time.perf_counter()
                t_new.append(t1 - t0)
                t_loop.append(t2 - t1)
            full = sorted(((sum(v), key) for key, v in total.items() if len(v) == T), key=lambda e: (-e[0], e[1]))[:k]
            # the loop only knows the groups that made every token's best 1024: its leading entries are compared
            rec["loop_complete_groups"] = len(full)
            rec["loop_agrees_on_those"] = bool([e[1] for e in full] == keys.tolist()[:len(full)] and
                                               [e[0] for e in full] == scores.tolist()[:len(full)])
            rec["same_as_exact_route"] = bool(ekeys.tolist() == keys.tolist() and
                                              escores.view(np.uint64).tolist() == scores.view(np.uint64).tolist())
            rec["exact_route_ms"] = round(float(np.median(t_exact)) * 1e3, 4)
            rec["maxsim_ms"] = round(float(np.median(t_new)) * 1e3, 4)
            rec["loop_ms"] = round(float(np.median(t_loop)) * 1e3, 4)
            rec["loop_over_maxsim"] = round(rec["loop_ms"] / rec["maxsim_ms"], 2)
            line = json.dumps(rec)
            print(line, flush=True)
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""In-place update (update_rows) against the only other route to new values, delete_many + add_rows, on
one N x 384 cosine index with all three lazy copies built.

`update_probe.py [N] [--out FILE] [--rounds R]` writes profiles/update_<N>x384.jsonl.  For m = 1, 1 000 and 100 000 random ids,
R alternated rounds of
  update_rows(ids, new values)                 -- then the first and the second single search, a batch of 64, and the time
                                                  until 256 filters made beforehand have answered filter.rows() again
  delete_many(ids) + add_rows(ids, new values) -- the same four figures
on ONE handle (the delete + add moves the rows to the end; the index holds N rows after either).  Per m the medians of the
rounds; for the update also vl_index_last_update's device time and the bytes it wrote (per row: f64 master, f32 slab, two bf16
rows, the int8 row and the per-row scalars) over that time.  Nothing here asserts a speed."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vectorlite_amd as V


def main():
    args = sys.argv[1:]
    out_path, rounds = None, 5
    for flag in ("--out", "--rounds"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                out_path = args[i + 1]
            else:
                rounds = int(args[i + 1])
            del args[i:i + 2]
    n, dim = int(args[0]) if args else 10_000_000, 384
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = out_path or os.path.join(root, "profiles", f"update_{n}x{dim}.jsonl")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2025)
    idx = V.FlatIndex(dim)
    idx.reserve(n + 200_000)
    for c0 in range(0, n, 500_000):
        c = min(500_000, n - c0)
        g = torch.Generator(device=dev)
        g.manual_seed(99 + c0)
        x = torch.randn((c, dim), dtype=torch.float64, device=dev, generator=g)
        x /= torch.linalg.norm(x, dim=1, keepdim=True)
        idx.add_rows(np.arange(c0, c0 + c, dtype=np.uint64), x, validate=False)
        del x
    torch.cuda.synchronize()
    q = rng.standard_normal(dim)
    Q = rng.standard_normal((64, dim))

    def build_copies():
        for mode in ("i8", "bf16", "f32", "auto"):
            idx.set_single_filter(mode)
            idx.search_arrays(q, 10, 0)
        idx.search_batch(Q, 10, 0)

    build_copies()
    filters = [idx.make_filter(rng.integers(n, size=1000).astype(np.uint64)) for _ in range(256)]
    for f in filters:
        f.rows()

    def ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def after():
        return {"first_search_ms": ms(lambda: idx.search_arrays(q, 10, 0)), "second_search_ms": ms(lambda: idx.search_arrays(q, 10, 0)),
                "batch64_ms": ms(lambda: idx.search_batch(Q, 10, 0)), "filters256_usable_ms": ms(lambda: [f.rows() for f in filters])}

    ldb = 384
    bytes_per_row = dim * 8 + dim * 4 + 2 * ldb * 2 + ldb + 4 + 1 + 8 + 8 + 4  # master, slab, bf16 x 2, int8, inv_norm, flag, norm16 + sqnorm, (s, r), |row|
    lines = []
    for m in (1, 1000, 100_000):
        if m > n // 4:
            continue
        runs = {"update_rows": [], "delete_many + add_rows": []}
        for r in range(rounds):
            ids = rng.choice(n, size=m, replace=False).astype(np.uint64)
            vals = rng.standard_normal((m, dim))
            vals /= np.linalg.norm(vals, axis=1, keepdims=True)
            rec = {"wall_ms": ms(lambda: idx.update_rows(ids, vals))}
            st = idx.last_update()
            assert st["updated"] == m and st["inserted"] == 0, st
            rec.update(device_ms=st["micros"] / 1e3, chunks=st["chunks"], int8_rows=st["int8_rows"], bf16_rows=st["bf16_rows"],
                       bf16_frag_rows=st["bf16_frag_rows"], written_GB_per_s=m * bytes_per_row / max(st["micros"], 1) / 1e3)
            rec.update(after())
            runs["update_rows"].append(rec)

            def delete_add():
                assert idx.delete_many(ids) == m
                idx.add_rows(ids, vals, validate=False)
            rec = {"wall_ms": ms(delete_add)}
            rec.update(after())
            runs["delete_many + add_rows"].append(rec)
            build_copies()  # both routes start from an index whose copies are complete
        for route, recs in runs.items():
            med = {k: round(float(np.median([r[k] for r in recs])), 3) for k in recs[0]}
            lines.append(json.dumps({"run": route, "ids": m, "rounds": rounds, "rows": n, "dim": dim, "bytes_per_updated_row": bytes_per_row, **med}))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()

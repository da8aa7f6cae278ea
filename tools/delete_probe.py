#!/usr/bin/env python3
"""Order-preserving delete on a big index (Vec::retain, src/index/flat.rs:94): gigabytes of rows slide through the bounce
buffer; afterwards every remaining row must still be where its id says, duplicates of a deleted id must all be gone, and
the fast path must still equal the exact one.

`delete_probe.py --bulk [N] [--out FILE]` measures the bulk delete (delete_many) against the single one
on one N x 384 index and writes profiles/delete_bulk_<N>x384.jsonl: at each of 16 uniformly random positions delete(id),
delete_many([id]) and delete(id) again on the row stored there (like for like; the two single deletes give the run-to-run
spread); then delete_many of 1, 1 000, 100 000 and 1 000 000 random ids and of a contiguous 10 % block at the front.  After every delete as many fresh rows are added again, so every run sees N rows.  Per run: wall
time, the device time and bytes written of vl_index_last_delete, the host's share (wall - device: the walk over the ids and
the compaction of the host arrays), and the first search afterwards (it re-converts the derived copies behind the first
hole) beside the second."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vectorlite_amd as V


def bulk_main():
    import json
    args = [a for a in sys.argv[1:] if a != "--bulk"]
    out_path = None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    n, dim = int(args[0]) if args else 10_000_000, 384
    out_path = out_path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", f"delete_bulk_{n}x{dim}.jsonl")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2024)
    idx = V.FlatIndex(dim)
    idx.reserve(n + 1_100_000)
    live = []        # ids in storage order, as chunks
    next_id = [0]

    def add(count, seed):
        for c0 in range(0, count, 500_000):
            c = min(500_000, count - c0)
            g = torch.Generator(device=dev)
            g.manual_seed(seed + c0)
            x = torch.randn((c, dim), dtype=torch.float64, device=dev, generator=g)
            x /= torch.linalg.norm(x, dim=1, keepdim=True)
            ids = np.arange(next_id[0], next_id[0] + c, dtype=np.uint64)
            next_id[0] += c
            idx.add_rows(ids, x, validate=False)
            live.append(ids)
            del x
        torch.cuda.synchronize()

    def stored():
        ids = np.concatenate(live)
        live[:] = [ids]
        return ids

    def forget(gone):
        ids = stored()
        live[:] = [ids[~np.isin(ids, gone)]]

    def timed_search(q):
        t0 = time.perf_counter()
        idx.search_arrays(q, 10, 0)
        return (time.perf_counter() - t0) * 1e3

    add(n, 99)
    q = rng.standard_normal(dim)
    for _ in range(3):
        timed_search(q)   # the derived copies exist before anything is deleted
    lines = []

    def emit(rec):
        rec.update(rows=n, dim=dim)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # ---- one id, like for like: at each of 16 uniformly random positions the row stored there goes three times (the index is
    # re-filled at its end after each, so the position and the rows behind it stay the same): delete(id), delete_many([id]),
    # delete(id) again.  The two single deletes give that position's run-to-run spread; the bulk call is judged against it.
    def one_delete(pos, bulk):
        victim = int(stored()[pos])
        t0 = time.perf_counter()
        if bulk:
            idx.delete_many([victim])
        else:
            idx.delete(victim)
        ms = (time.perf_counter() - t0) * 1e3
        rec = {"run": "delete_many([id])" if bulk else "delete(id)", "position": pos, "rows_moved": n - 1 - pos, "wall_ms": round(ms, 3)}
        if bulk:
            st = idx.last_delete()
            rec.update(device_ms=round(st["micros"] / 1e3, 3), bytes_written=st["bytes_written"], direct_launches=st["direct_launches"],
                       bounced_segments=st["bounced_segments"])
        rec.update(first_search_ms=round(timed_search(q), 3), second_search_ms=round(timed_search(q), 3))
        emit(rec)
        forget(np.array([victim], dtype=np.uint64))
        add(1, 5000 + len(lines))
        return ms

    single_ms, ratios, spreads = [], [], []
    for i in range(16):
        pos = int(rng.integers(n))
        d1 = one_delete(pos, False)
        b1 = one_delete(pos, True)
        d2 = one_delete(pos, False)
        single_ms += [d1, d2]
        ratios.append(b1 / ((d1 + d2) / 2))
        spreads.append(max(d1, d2) / ((d1 + d2) / 2))
    emit({"run": "one id, summary", "positions": 16,
          "delete_ms_per_id_mean": round(float(np.mean(single_ms)), 3), "delete_ms_per_id_min": round(min(single_ms), 3),
          "delete_ms_per_id_max": round(max(single_ms), 3),
          # per position: delete_many([id]) / mean of the two delete(id) there; and the slower delete(id) / that mean
          "delete_many_over_delete_median": round(float(np.median(ratios)), 3), "delete_many_over_delete_min": round(min(ratios), 3),
          "delete_many_over_delete_max": round(max(ratios), 3),
          "delete_run_to_run_median": round(float(np.median(spreads)), 3), "delete_run_to_run_max": round(max(spreads), 3),
          "delete_many_within_run_to_run_spread_of_delete": bool(np.median(ratios) <= np.median(spreads)),
          "positions_where_delete_many_within_both_deletes_spread": int(sum(r <= s for r, s in zip(ratios, spreads)))})

    # ---- many ids
    runs = [("random", m) for m in (1, 1000, 100_000, 1_000_000) if m <= n // 2] + [("front block", n // 10)]
    for kind, m in runs:
        ids = stored()
        gone = rng.permutation(ids[rng.choice(ids.size, size=m, replace=False)]) if kind == "random" else ids[:m].copy()
        t0 = time.perf_counter()
        removed = idx.delete_many(gone)
        wall = (time.perf_counter() - t0) * 1e3
        st = idx.last_delete()
        assert removed == m == st["removed"] and len(idx) == n - m
        dev_ms = st["micros"] / 1e3
        rec = {"run": f"delete_many, {kind}", "ids": m, "wall_ms": round(wall, 3), "device_ms": round(dev_ms, 3),
               "host_ms": round(wall - dev_ms, 3), "rows_moved": st["moved"], "bytes_written": st["bytes_written"],
               "written_TB_per_s": round(st["bytes_written"] / max(dev_ms, 1e-9) / 1e9, 3),
               "share_of_8_TB_per_s_peak": round(st["bytes_written"] / max(dev_ms, 1e-9) / 1e9 / 8.0, 3),
               "direct_launches": st["direct_launches"], "bounced_segments": st["bounced_segments"],
               "single_front_deletes_equivalent": round(wall / max(single_ms), 2)}
        rec.update(first_search_ms=round(timed_search(q), 3), second_search_ms=round(timed_search(q), 3))
        emit(rec)
        forget(gone)
        add(m, 7000 + m)
        timed_search(q)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if "--bulk" in sys.argv:
    bulk_main()
    sys.exit(0)

n, dim = int(sys.argv[1]) if len(sys.argv) > 1 else 3_000_000, 384
dev = torch.device("cuda", 0)
idx = V.FlatIndex(dim); idx.reserve(n)
keep = {}
for ci, c0 in enumerate(range(0, n, 500_000)):
    c = min(500_000, n - c0)
    g = torch.Generator(device=dev); g.manual_seed(99 + ci)
    x = torch.randn((c, dim), dtype=torch.float64, device=dev, generator=g)
    ids = np.arange(c0, c0 + c, dtype=np.uint64) * np.uint64(5) + np.uint64(2)
    if ci == 2:
        ids[1000:1004] = 777          # four MORE rows share the id of position 155 (5 * 155 + 2 = 777): FlatIndex::new keeps them
    idx.add_rows(ids, x, validate=False)
    for p in (0, 17, c - 1):
        keep[int(ids[p])] = x[p].cpu().numpy()
    del x
assert len(idx) == n
victims = [int(5 * 10 + 2), int(5 * (n // 2) + 2), 777, int(5 * (n - 2) + 2), 123456789]   # early, middle, the duplicated id, late, absent
t0 = time.perf_counter()
for v in victims:
    idx.delete(v)
dt = time.perf_counter() - t0
assert len(idx) == n - 3 - 5, len(idx)
assert idx.get_vector(777) is None
bad = 0
for id_, row in keep.items():
    if id_ in victims:
        continue
    got = idx.get_vector(id_)
    assert got is not None and np.array_equal(np.asarray(got.values), row), id_
    r = idx.search(row, 1, 0)
    assert r[0].id == id_, (id_, r[0].id)
rng = np.random.default_rng(1)
for m in range(4):
    q = rng.standard_normal(dim)
    fi, fs = idx.search_arrays(q, 10, m)
    idx.force_path(V.PATH_EXACT_SELECT)
    try:
        ei, es = idx.search_arrays(q, 10, m)
    finally:
        idx.force_path(0)
    assert fi.tolist() == ei.tolist() and fs.tolist() == es.tolist(), m
print(f"delete probe: {n} x {dim} rows, 5 deletes (one id held by five rows, one absent) in {dt * 1e3:.0f} ms; {len(keep)} kept rows found where their ids say; fast == exact; ok")

"""CPU restatement of the id-filtered HNSW walk in reference navigation, over an exported-graph
dict (vectorlite_amd.HNSWIndex.graph(with_rows=True), or a hand-made one with the same keys).  Checker only.

A node PASSES iff `passing[node]` (the caller folds `live` in).  Upper layers: the unfiltered greedy descent of
oracle/vl_hnsw_cpu.c (beam of 1, a tied candidate stays behind).  Layer 0: one sorted list B of [u64, seq, node, pass,
expanded] entries, starting as the single entry the descent landed on; expand the first unexpanded entry; every neighbour
not yet visited, in list order, is marked, evaluated (one evaluation, the next sequence number) and inserted at its sorted
(u64, seq) position; after EVERY insertion B is cut to its first `cap` entries and then to its window -- the shortest
prefix holding `ef` passing entries, all of B while it holds fewer.  No early reject: every candidate really is inserted.

`cut` reports whether the cap cut ever dropped an entry that was already in the list and that the window cut alone would
have kept (a candidate that ranks at or behind `cap` and so drops itself never was in it; an entry behind the ef-th
passing one goes either way)."""
from bisect import bisect_right

import numpy as np


def _distance(metric):
    from oracle import oracle as O
    O.build()
    return lambda a, b: O.hnsw_distance(metric, a, b)


def filtered_walk(graph, metric, q, ef, cap, passing, k=None):
    """-> dict(nodes, dist, evals, longest, cut, lost_efth): the passing entries of the final list in order (at most k),
    their u64 distances, the evaluations made, the longest list seen after the cuts of an insertion, whether cap cut,
    and whether an entry it dropped was the ef-th passing one."""
    assert ef >= 1 and cap >= ef
    dist = _distance(metric)
    rows = graph["rows"]
    q = np.ascontiguousarray(q, dtype=np.float64)
    n = graph["n"]
    if n == 0:
        return {"nodes": [], "dist": [], "evals": 0, "longest": 0, "cut": False, "lost_efth": False}
    entry = graph["entry"]
    evals, seq = 1, 1
    best = (dist(q, rows[entry]), 0, entry)
    # upper layers: greedy, beam of 1, unfiltered, a fresh visited set per layer
    for layer in range(graph["max_level"], 0, -1):
        visited = {best[2]}
        expanded = False
        while not expanded:
            expanded = True
            c = best[2]
            slot = int(graph["upper_off"][c]) + layer - 1
            for e in graph["nbrU"][slot][: int(graph["cntU"][slot])].tolist():
                if e in visited:
                    continue
                visited.add(e)
                d = dist(q, rows[e])
                evals += 1
                s, seq = seq, seq + 1
                if d < best[0]:  # a tie stays behind the entry already there
                    best = (d, s, e)
                    expanded = False  # the newcomer is unexpanded; the rest of this list is still offered
        # the survivor is the entry point of the next layer
    B = [[best[0], best[1], best[2], bool(passing[best[2]]), False]]
    keys = [(best[0], best[1])]  # the (u64, seq) keys of B, kept beside it for the binary search
    visited = {best[2]}
    longest, cut, lost_efth = 1, False, False
    while True:
        pick = next((x for x in B if not x[4]), None)
        if pick is None:
            break
        pick[4] = True
        c = pick[2]
        for e in graph["nbr0"][c][: int(graph["cnt0"][c])].tolist():
            if e in visited:
                continue
            visited.add(e)
            d = dist(q, rows[e])
            evals += 1
            s, seq = seq, seq + 1
            at = bisect_right(keys, (d, s))
            keys.insert(at, (d, s))
            B.insert(at, [d, s, e, bool(passing[e]), False])
            window, seen = len(B), 0
            for i, x in enumerate(B):
                seen += x[3]
                if seen == ef:
                    window = i + 1
                    break
            if window > cap and at < cap:
                cut = True  # the entry now behind cap was in the list, and the window would have kept it
                lost_efth = lost_efth or seen == ef  # ... and it closed the window: the ef-th passing entry
            del B[min(window, cap):]  # cap, then the window: the same prefix in either order
            del keys[len(B):]
            longest = max(longest, len(B))
    out = [x for x in B if x[3]]
    if k is not None:
        out = out[:k]
    return {"nodes": [x[2] for x in out], "dist": [x[0] for x in out], "evals": evals, "longest": longest, "cut": cut,
            "lost_efth": lost_efth}

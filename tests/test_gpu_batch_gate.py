"""VL_MFMA and VL_MFMA_MIN_BATCH, read per call by the one gate of the batched MFMA routes (csrc/batch_gate.hpp, DESIGN.md
section 19): switching the filter off, or asking for a larger batch than the call has, moves search_batch, the filtered, the
grouped, the MMR and the range batch off the pass and changes no id and no score bit; the last_*_batch counters tell which
route a call took.  (The plain search_batch has no such counter: the profile tells, the pass being the one route that
streams the bf16 slab exactly once for the whole batch.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS = 0
N, DIM, NQ, K = 9000, 128, 4, 10   # just above MFMA_MIN_ROWS, the size the batched tests use


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def test_env_switches_move_every_batched_mode_off_the_pass_and_change_no_bit(monkeypatch):
    import vectorlite_amd as V
    n_dev, _ = V.runtime_info()
    assert n_dev > 0, "GPU tests need a HIP device"
    rng = np.random.default_rng(1909)
    rows = rng.standard_normal((N, DIM))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    ids = np.arange(N, dtype=np.uint64) * np.uint64(3) + np.uint64(11)
    Q = rng.standard_normal((NQ, DIM))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    idx = V.FlatIndex(DIM, device=0)
    idx.add_rows(ids, rows, validate=False)
    excluded = idx.make_filter(ids[::7], exclude=True)
    table = idx.make_groups(ids, ids % np.uint64(50))
    idx.set_masked_batch("on")
    idx.set_grouped_batch("on")
    idx.set_mmr_batch("on")

    def run():
        out, routed = {}, {}
        idx.profile_read()
        idx.profile_enable(True)
        gi, gs, gn = idx.search_batch(Q, K, COS)
        idx.profile_enable(False)
        out["plain"] = (gi.tolist(), bits(gs), gn.tolist())
        # the pass is one launch sequence over the bf16 slab; off it, NQ single searches or the f32 rows (4 bytes a value)
        passes, _, nbytes = idx.profile_read()
        routed["plain"] = NQ if (passes, nbytes) == (1, N * DIM * 2) else 0
        gi, gs, gn = idx.search_batch(Q, K, COS, filter=excluded)
        out["filtered"] = (gi.tolist(), bits(gs), gn.tolist())
        routed["filtered"] = idx.last_masked_batch()["routed"]
        gk, gi, gs, gn = idx.search_grouped_batch_arrays(Q, K, COS, groups=table)
        out["grouped"] = (gk.tolist(), gi.tolist(), bits(gs), gn.tolist())
        routed["grouped"] = idx.last_grouped_batch()["routed"]
        gi, gs, gn = idx.search_mmr_batch_arrays(Q, K, 20, 0.5, COS)
        out["mmr"] = (gi.tolist(), bits(gs), gn.tolist())
        routed["mmr"] = idx.last_mmr_batch()["routed"]
        il, sl, totals = idx.search_range_batch_arrays(Q, 0.25, COS, limit=32)
        out["range"] = ([np.asarray(i).tolist() for i in il], [bits(s) for s in sl], [int(t) for t in totals])
        routed["range"] = idx.last_range_batch()["mfma_queries"]
        return out, routed

    monkeypatch.delenv("VL_MFMA", raising=False)
    monkeypatch.delenv("VL_MFMA_MIN_BATCH", raising=False)
    base, routed = run()                                  # (a) nothing set
    assert routed == dict.fromkeys(routed, NQ), routed
    assert all(n == K for n in base["plain"][2]) and sum(base["range"][2]) > 0
    monkeypatch.setenv("VL_MFMA", "0")                    # (b) the filter switched off
    got, routed = run()
    assert got == base and routed == dict.fromkeys(routed, 0), routed
    monkeypatch.delenv("VL_MFMA")
    monkeypatch.setenv("VL_MFMA_MIN_BATCH", str(NQ + 1))  # (c) one query short of the minimum batch
    got, routed = run()
    assert got == base and routed == dict.fromkeys(routed, 0), routed
    monkeypatch.setenv("VL_MFMA_MIN_BATCH", str(NQ))      # (d) exactly the minimum batch
    got, routed = run()
    assert got == base and routed == dict.fromkeys(routed, NQ), routed

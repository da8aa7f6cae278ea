"""The host model of tests/_finalize_cases.py against FlatOracle, and the construction of its list-count cases.

tests/test_gpu_finalize_audit.py judges the merge / finalize / selection launchers with this model; here the model is
shown right first, without a GPU: fed with lists that hold every row of a small index under their f32 scan keys it must
answer like FlatOracle.search, and the planted winners of every list-count case must cover what the audit is there for.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _finalize_cases as F  # noqa: E402
from oracle import oracle  # noqa: E402


def scan_keys(metric, rows, q):
    """The f32 scan key of every row (larger = better), from the f32-rounded inputs."""
    x, y = rows.astype(np.float32).astype(np.float64), q.astype(np.float32).astype(np.float64)
    if metric == F.COS:
        nrm = np.linalg.norm(rows, axis=1)
        return ((x @ y) * np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)).astype(np.float32)
    if metric == F.DOT:
        return (x @ y).astype(np.float32)
    d = x - y[None, :]
    return (-(d * d).sum(axis=1) if metric == F.EUC else -np.abs(d).sum(axis=1)).astype(np.float32)


def index_rows(rng, n, dim):
    rows = F.mixed_rows(rng, n, dim)
    rows[n // 3] = rows[n // 2]          # equal rows: the lower position ranks first
    rows[n - 1] = rows[0]
    return rows


def as_lists(rng, keys, n_lists):
    """Every row in one of n_lists sorted lists (at most 64 each)."""
    n = len(keys)
    li = np.sort(rng.permutation(np.arange(n) % n_lists))
    li = li[rng.permutation(n)] if n <= n_lists * F.KP else li
    pos = np.arange(n, dtype=np.uint32)
    order = np.lexsort((pos, -keys.astype(np.float64), li))
    return np.bincount(li, minlength=n_lists).astype(np.uint32), keys[order], pos[order]


@pytest.mark.parametrize("metric", F.ALL4, ids=[F.METRIC_NAME[m] for m in F.ALL4])
@pytest.mark.parametrize("n,n_lists", [(40, 3), (64, 5), (64, 1), (200, 7)])
def test_list_model_answers_like_flat_oracle(metric, n, n_lists):
    rng = np.random.default_rng([1, metric, n])
    dim = 6
    rows = index_rows(rng, n, dim)
    ids = np.arange(n, dtype=np.uint64) * 7 + 3
    orc = oracle.FlatOracle(dim, ids, rows)
    R = float(np.linalg.norm(rows, axis=1).max())
    for k in (1, 10, 64):
        if n > F.KP and k == 64:
            continue  # rows outside the list: its 64th entry cannot certify itself
        q = rng.standard_normal(dim)
        lens, keys, pos = as_lists(rng, scan_keys(metric, rows, q), n_lists)
        case = F.ListCase(F.FINALIZE, metric, rows, q[None, :], lens, keys, pos, n_lists, n, k, R)
        assert F.lists_sorted(case)
        merged = F.merge_groups(case)
        assert merged[0].n_cand == min(n, F.KP)
        ans = F.model_answers(case, oracle.calculate, merged)
        F.set_flags(case, merged, ans, [F.py_bound(metric, merged[0].key64, 8, R, case.qn[0], 0.0)])
        want_ids, want_scores = orc.search(q, k, metric)
        a = ans[0]
        m = min(a.k_eff, a.n_cand)
        assert a.k_eff == len(want_ids) == min(k, n)
        assert (ids[a.pos[:m]] == want_ids).all(), (k, a.pos[:m], want_ids)
        assert (a.score[:m] == F.bits(want_scores)).all()
        assert a.flags == 0, (k, a.flags)
        blk = F.expected_blocks(case, ans, 1)
        assert int(blk["n_out"][0]) == len(want_ids) and (blk["pos"][0][m:] == F.FILL32).all()


def test_flag_logic_edges():
    # rank_check_emit: certifies iff s_cut > B, strictly
    assert F.flags_single(False, 64, 100, 10, 0.5, 0.5) == F.NEEDS_EXACT
    assert F.flags_single(False, 64, 100, 10, 0.5, np.nextafter(0.5, 0.0)) == 0
    assert F.flags_single(False, 64, 100, 10, 0.5, float("inf")) == F.NEEDS_EXACT
    assert F.flags_single(False, 63, 100, 10, 0.5, -1.0) == F.NEEDS_EXACT
    assert F.flags_single(False, 40, 40, 10, 0.5, 9.0) == 0
    assert F.flags_single(False, 39, 40, 10, 0.5, -9.0) == F.NEEDS_EXACT
    assert F.flags_single(True, 40, 40, 10, 0.5, -9.0) == F.NEEDS_EXACT | F.HAS_NAN
    assert F.flags_single(False, 64, 100, 0, 0.0, -9.0) == F.NEEDS_EXACT
    # k_merge_finalize_multi: the largest bound over the FULL partitions decides
    assert F.flags_multi(False, [64, 64], 500, 100, 0.5, [0.4, 0.5]) == F.NEEDS_EXACT
    assert F.flags_multi(False, [64, 64], 500, 100, 0.5, [0.4, 0.49]) == 0
    assert F.flags_multi(False, [64, 20], 500, 70, 0.5, [0.4, 0.9]) == 0          # a short list excludes no row
    assert F.flags_multi(False, [30, 20], 500, 40, 0.5, [0.0, 0.0]) == F.NEEDS_EXACT  # short lists that do not cover
    assert F.flags_multi(False, [30, 20], 50, 40, 0.5, [0.0, 0.0]) == 0
    assert F.flags_multi(False, [30, 20], 50, 50, 0.5, [0.0, 0.0]) == 0
    assert F.flags_multi(False, [64, 64], 500, 129, 0.5, [0.0, 0.0]) == F.NEEDS_EXACT  # total < k_eff
    # the f32 ordering used to step key64 by one ulp
    for v in (-1.5, -0.0, 0.0, 1e-45, 3.25):
        o = F.f32_to_ordered(v)
        assert F.ordered_to_f32(o).tobytes() == np.float32(v).tobytes()
        assert F.ordered_to_f32(o + 1) > np.float32(v) or (v == 0 and F.ordered_to_f32(o + 1) == 0)


def test_select_model_answers_like_flat_oracle():
    rng = np.random.default_rng(5)
    n, dim = 300, 3
    rows = rng.integers(-1, 2, size=(n, dim)).astype(np.float64)  # 27 distinct rows: long ties
    ids = np.arange(n, dtype=np.uint64) + 1000
    orc = oracle.FlatOracle(dim, ids, rows)
    for metric in F.ALL4:
        q = np.array([1.0, -2.0, 0.5])
        scores = np.array([oracle.calculate(metric, r, q) for r in rows])
        for krs in ((10,), (64,), (64, 64, 64, 36), (64,) * 5 + (1,)):
            blk = F.select_model(scores, krs, 0)
            k = 64 * (len(krs) - 1) + krs[-1]
            want_ids, want_scores = orc.search(q, k, metric)
            got_pos = np.concatenate([blk["pos"][r][:min(kr, max(0, n - 64 * r))] for r, kr in enumerate(krs)])
            got_sc = np.concatenate([blk["score"][r][:min(kr, max(0, n - 64 * r))] for r, kr in enumerate(krs)])
            assert (ids[got_pos] == want_ids).all(), (metric, krs)
            assert (got_sc == F.bits(want_scores)).all()
            assert (blk["flags"] == 0).all() and int(blk["n_out"][-1]) == krs[-1]
    # rows run out inside a full round: sentinels, and a later round is empty
    blk = F.select_model(np.array([1.0, -0.0, 0.0, 2.0]), (64, 64), 1)
    assert blk["pos"][0][:5].tolist() == [3, 0, 1, 2, F.POS_SENTINEL] and (blk["pos"][1] == F.POS_SENTINEL).all()
    assert blk["n_out"].tolist() == [4, 4] and (blk["flags"] == F.HAS_NAN).all()


@pytest.mark.parametrize("n_lists", F.LIST_COUNTS)
def test_list_count_cases_plant_their_winners(n_lists):
    cases = F.list_count_cases(n_lists)
    assert all(F.lists_sorted(c) for c in cases)
    assert {c.metric for c in cases} >= {F.COS}
    F.check_list_count_coverage(n_lists, cases, [F.merge_groups(c) for c in cases])


def test_all_four_metrics_among_the_list_count_cases():
    assert {F.ALL4[1 + F.LIST_COUNTS.index(n) % 3] for n in F.LIST_COUNTS if n <= 129} == {F.EUC, F.MAN, F.DOT}


def test_generated_cases_are_well_formed():
    for mode in (F.FINALIZE, F.BATCH):
        for c in F.branch_cases(mode) + F.width_cases(mode, 49):
            assert F.lists_sorted(c), c.name
    for p in F.MULTI_PARTS:
        for L in (1, 5, 65):
            for c in F.multi_cases(p, L):
                assert F.lists_sorted(c), c.name
                assert c.k <= F.KMULTI_MAX
    chains = {(len(c.krs), c.krs[-1]) for n in F.SELECT_N for c in F.select_cases(n)}
    assert chains >= {(r, k) for r in F.SELECT_CHAINS for k in F.SELECT_LAST}
    assert any(c.flag_word for n in F.SELECT_N for c in F.select_cases(n) if n < 1000)

"""The 8-query f32 batch scan (k_scan_batch, "K3") through the library, where no other test sends it: Manhattan batches on
an index above the MFMA filter's 8192-row floor, the row strides 192 / 320 / 640 / 1024 / 1536, and launches cut down to
one or two workgroups (VL_BATCH_GRID, read at every launch) so that every wave loops over hundreds of rows and folds its
lazy insertion buffer into its lists many times -- with the rows stored in rising and in falling order of score.

Every row of every batch is the oracle's, ids and score bits.  What these tests cannot see: a query whose K3 list fails the
bound check is redone on the exact path by search_batch and then answers like the oracle all the same, without a trace in
vl_last_path or in the profile's pass count.  A list that lost rows can therefore pass here (it fails only if the loss
reaches the top k unnoticed by the bound check); the list-level audit (test_gpu_filter_audit.py, the `ordered` and
`lattice` cases) is the check for that.  The pass count asserted below catches the other detour: a query handed to the
single-query f32 scan adds a pass of its own.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
KMAX = 48
# one dim per row stride of the batch shapes (32 ... 1536 floats); 190, 637 and 1021 only pad to theirs
STRIDE_DIMS = (32, 64, 96, 128, 190, 256, 320, 384, 512, 637, 768, 1021, 1536)


@pytest.fixture(scope="module")
def V():
    import vectorlite_amd as V
    n_dev, _ = V.runtime_info()
    assert n_dev > 0, "GPU tests need a HIP device"
    return V


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    O.build()
    return O


def permuted_ids(n):
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(2 ** 40)


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


class Pair:
    """One set of rows in the library and in the oracle; the oracle's top KMAX of a query is computed once (a smaller k is
    its prefix: the oracle ranks by a stable sort and cuts)."""

    def __init__(self, V, O, rows):
        n, dim = rows.shape
        ids = permuted_ids(n)
        self.gpu = V.FlatIndex(dim)
        self.gpu.add_rows(ids, rows, validate=False)
        self.ref = O.FlatOracle(dim, ids, rows)
        self.want = {}

    def check_batch(self, Q, nq, k, metric, ctx, passes=None):
        """search_batch(Q[:nq]) against the oracle, every query; `passes`: the slab passes the profile must count."""
        if passes is not None:
            self.gpu.profile_read()
            self.gpu.profile_enable(True)
        bi, bs, bn = self.gpu.search_batch(Q[:nq], k, metric)
        if passes is not None:
            self.gpu.profile_enable(False)
            assert self.gpu.profile_read()[0] == passes, (ctx, nq, k, "slab passes")
        assert bn.tolist() == [k] * nq, (ctx, nq, k)
        for i in range(nq):
            if (metric, i) not in self.want:
                self.want[metric, i] = self.ref.search(Q[i], KMAX, metric)
            ri, rs = self.want[metric, i]
            assert bi[i].tolist() == ri[:k].tolist(), (ctx, nq, k, i, "ids")
            assert bs[i].tolist() == rs[:k].tolist(), (ctx, nq, k, i, "scores")


@pytest.mark.parametrize("dim", STRIDE_DIMS)
def test_manhattan_batches_above_the_mfma_floor(V, O, dim):
    """Manhattan has no MFMA filter: on 9000 rows (MFMA_MIN_ROWS = 8192) its batches still run 8 per f32 slab pass, at
    every stride.  Random rows, no ties: ceil(nq / 8) passes and nothing else."""
    rng = np.random.default_rng(3000 + dim)
    p = Pair(V, O, rng.standard_normal((9000, dim)))
    Q = rng.standard_normal((23, dim))
    for nq in (2, 8, 9, 23):
        for k in (1, 10, KMAX):
            p.check_batch(Q, nq, k, MAN, ("manhattan", dim), passes=(nq + 7) // 8)


@pytest.mark.parametrize("dim", [192, 320, 637, 1024, 1536])
def test_wide_strides_below_the_mfma_floor(V, O, dim):
    """2500 rows: every metric's batch takes K3.  One exact duplicate row, a query equal to it (a tie the list cannot
    break: that query is redone exactly) and a query equal to an ordinary row."""
    rng = np.random.default_rng(4000 + dim)
    rows = rng.standard_normal((2500, dim))
    rows[1700] = rows[11]
    p = Pair(V, O, rows)
    Q = rng.standard_normal((9, dim))
    Q[4] = rows[11]
    Q[6] = rows[300]
    for metric in (COS, EUC, MAN, DOT):
        for k in (1, 10, KMAX):
            p.check_batch(Q, 9, k, metric, ("wide", dim, metric))


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("dim", [64, 192, 640])
def test_looping_waves_with_rows_in_score_order(V, O, monkeypatch, dim, grid):
    """VL_BATCH_GRID = 1 / 2: four or eight waves stream all 2500 rows (8 queries; 11 queries are two groups, one workgroup
    each).  Rows stored in rising order of score to Q[0]: every row Q[0] meets beats its list, the buffer fills and is
    folded in as often as it can be; in falling order nothing gets in after the first 64.  The other queries see the rows in
    no order, so the 8 buffers of a wave fill out of step.  4, 8 and 16 lanes per row."""
    monkeypatch.setenv("VL_BATCH_GRID", str(grid))
    rng = np.random.default_rng(5000 + dim)
    rows = unit_rows(rng, 2500, dim)
    Q = unit_rows(rng, 11, dim)
    # unit rows and a unit query: cosine, dot and Euclidean rank alike; Manhattan has its own order
    orders = (((COS, EUC, DOT), np.argsort(rows @ Q[0], kind="stable")),
              ((MAN,), np.argsort(-np.abs(rows - Q[0][None, :]).sum(axis=1), kind="stable")))
    for metrics, rising in orders:
        for name, order in (("rising", rising), ("falling", rising[::-1])):
            p = Pair(V, O, rows[order])
            for metric in metrics:
                for nq in (8, 11):
                    for k in (10, KMAX):
                        p.check_batch(Q, nq, k, metric, ("looping", dim, grid, name, metric), passes=(nq + 7) // 8)

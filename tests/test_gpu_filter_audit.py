"""Audit of every candidate filter against the exactness bound it is certified with.

tests/native/filter_audit.hip runs the library's own stages on one case -- ingest, the bf16 row copies, ONE filter, the
shipped bound_for_key on the device, the exact f64 scan of every row -- and writes the filter's 64-entry list per query.
Here, for every query, with u = 2^-24 and n = the padded row length:
  (a) key fidelity: every listed key equals the key host numpy computes in f64 from the same rounded inputs, within the
      undoubled u-part of the bound ((n + 4) u times the sum of the absolute terms);
  (b) completeness: no row outside the list has a host key above the list's 64th key t64 (plus the same allowance);
  (c) certificate: every row outside the list has reference score <= B(t64), every listed row <= B(its key);
  (d) ordering: (key desc, pos asc), no duplicate positions, none >= n.
  (e) lattice cases only: the list IS the host's top 64 by (key desc, pos asc), positions and key bits, at zero tolerance.
End-to-end answers would only notice a wrong key or a dropped row if it landed in the final top k; these checks look at
the filter output itself.  For the 8-query f32 batch scan (k_scan_batch) nothing else can: a query whose list fails the
bound check is redone on the exact path and still answers like the oracle, so a list that lost rows in a mid-stream flush
of the lazy insertion buffer is invisible from outside.  The `ordered` and `lattice` cases run that kernel under
VL_BATCH_GRID, so that one workgroup streams the whole index and every wave flushes its buffers many times.
"""
import os
import struct
import subprocess
import sys
from dataclasses import dataclass, field

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _filter_host_model import (U, TINY, KP, POS_SENTINEL, MAGIC, COS, EUC, MAN, DOT, F32_QARG, F32_Q64, F32_BATCH,  # noqa: E402,F401
                                BF16_SINGLE, MFMA_BATCH, dev_sumsq, bf16_rne, f32, HostRows, host_keys, family)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FILTER_NAME = {F32_QARG: "f32-qarg", F32_Q64: "f32-q64", F32_BATCH: "f32-batch", BF16_SINGLE: "bf16-single",
               MFMA_BATCH: "mfma"}
METRIC_NAME = {COS: "cosine", EUC: "euclidean", MAN: "manhattan", DOT: "dot"}
ALL4 = (COS, EUC, MAN, DOT)
BF16_METRICS = (COS, EUC, DOT)


@dataclass
class Case:
    filt: int
    fam: str
    dim: int
    n: int
    nq: int
    metrics: tuple
    env: dict = field(default_factory=dict)
    tag: str = ""
    grid: int = 0        # f32 batch: the grid the launcher must arrive at under the case's VL_BATCH_GRID (0: not checked)
    loops: bool = False  # f32 batch: every wave must stream at least LOOP_ROWS rows

    @property
    def id(self):
        return f"{FILTER_NAME[self.filt]}-{self.fam}-d{self.dim}-n{self.n}-q{self.nq}{'-' + self.tag if self.tag else ''}"


N1 = 8192 + 37    # not a multiple of 16 / 32 / 64: the last block is masked
NM = 8192 + 45
NW = 4133         # rows longer than 768 columns (the case file stays near 50 MB)
NG = 2048 + 37    # the 512-query cases: 64 reference scans per metric
# A wave of k_scan_batch parks the rows that beat its list's (stale) threshold in a 64-entry buffer and folds the buffer
# in once more than 64 - RPS entries wait.  On the rising query of an `ordered` case every row beats all rows before it,
# so a wave that streams 256 rows flushes in mid-stream at least three times however stale the threshold is.
LOOP_ROWS = 256


def k3_looping(fam, dim, nq, metrics, cap, tag=None, n=None, grid=1):
    """An f32 batch case under VL_BATCH_GRID = cap that leaves `grid` workgroups to stream the whole index."""
    n = n or (N1 if dim <= 768 else NW)
    return Case(F32_BATCH, fam, dim, n, nq, metrics, {"VL_BATCH_GRID": str(cap)}, tag or f"grid{cap}", grid,
                n // (4 * grid) >= LOOP_ROWS)


# one dim per stride of VL_BATCH_SHAPES; 190, 637 and 1021 only pad to theirs (192, 640, 1024)
K3_DIMS = (32, 64, 96, 128, 190, 256, 320, 384, 512, 637, 768, 1021, 1536)
K3_FAMILIES = (("ordered", (COS, EUC, DOT)), ("ordered-l1", (MAN,)), ("ordered-l1r", (MAN,)), ("lattice", ALL4))
K3_EDGE_FAMILIES = (K3_FAMILIES[0], K3_FAMILIES[3])
K3_CASES = (
    # every stride, all four metrics: 11 queries = two groups, which halve the cap of 2 -- one workgroup, four waves
    [k3_looping(f, d, 11, m, 2) for d in K3_DIMS for f, m in K3_FAMILIES]
    # grid boundaries, one group of 8 (the cap is not divided): 65 lists per query give the merge a second level whose
    # second block holds a single list
    + [k3_looping(f, 128, 8, m, g, grid=g) for g in (1, 64, 65) for f, m in K3_EDGE_FAMILIES]
    # group boundaries at four lanes per row: 8 and 9 queries, and 512 = SCAN_BATCH_MAX_QUERIES (64 groups as blockIdx.y:
    # a cap of 64 leaves each group one workgroup; the largest cap leaves 32, which fills the partial-list buffer)
    + [k3_looping(f, 64, 8, m, 2, grid=2) for f, m in K3_EDGE_FAMILIES]
    + [k3_looping(f, 64, 9, m, 2) for f, m in K3_EDGE_FAMILIES]
    + [k3_looping("ordered", 64, 512, (COS, EUC, DOT), 64, n=NG), k3_looping("lattice", 64, 512, ALL4, 64, n=NG),
       k3_looping("lattice", 64, 512, ALL4, 4096, n=NG, grid=32)]
    # the older families once each at a wide stride, looping
    + [k3_looping("gauss", 640, 11, ALL4, 2), k3_looping("cancel", 1024, 11, ALL4, 2), k3_looping("scales", 1021, 11, ALL4, 2)]
)
CASES = (
    # f32 single query: the query in the kernel arguments (k_scan), from device memory (k_scan_q64), k_scan_generic
    [Case(F32_QARG, "gauss", d, N1, 4, ALL4) for d in (128, 384, 512, 768)]
    + [Case(F32_Q64, "gauss", d, N1, 4, ALL4) for d in (100, 300, 384, 700, 1536)]
    + [Case(F32_Q64, "gauss", 3072, 4133, 3, ALL4)]
    + [Case(F32_QARG, "scales", 384, N1, 4, ALL4), Case(F32_Q64, "scales", 700, N1, 4, ALL4),
       Case(F32_QARG, "cancel", 768, N1, 4, ALL4), Case(F32_Q64, "cancel", 300, N1, 4, ALL4),
       Case(F32_QARG, "underflow", 512, N1, 4, ALL4), Case(F32_Q64, "underflow", 100, N1, 4, ALL4),
       Case(F32_QARG, "bf16edge", 256, N1, 4, ALL4), Case(F32_Q64, "gemm", 1536, 4133, 4, ALL4)]
    # f32 batch: 11 queries = two groups of 8; four lanes per row at 32 / 64
    + [Case(F32_BATCH, "gauss", d, N1, 11, ALL4) for d in (32, 64, 96, 384, 768)]
    + [Case(F32_BATCH, "scales", 256, N1, 11, ALL4), Case(F32_BATCH, "cancel", 128, N1, 11, ALL4),
       Case(F32_BATCH, "underflow", 512, N1, 11, ALL4)]
    # bf16 single query
    + [Case(BF16_SINGLE, "gauss", d, N1, 4, BF16_METRICS) for d in (100, 384, 768)]
    + [Case(BF16_SINGLE, f, d, N1, 4, BF16_METRICS) for f, d in
       (("bf16edge", 256), ("scales", 512), ("cancel", 384), ("underflow", 300), ("gemm", 128))]
    # MFMA batch: k_mfma_rows at every stride (128 / 256 / 384 / 512 / 768), k_mfma_scan, 2 query chunks, 2-4 pass-1 stages
    + [Case(MFMA_BATCH, "gauss", d, NM, 40, BF16_METRICS) for d in (100, 256, 300, 512, 768)]
    + [Case(MFMA_BATCH, "gauss", d, NM, 40, BF16_METRICS, {"VL_MFMA_KERNEL": "tile"}, "tile") for d in (384, 700)]
    + [Case(MFMA_BATCH, "gauss", 384, NM, 160, BF16_METRICS, {}, "2chunks"),
       Case(MFMA_BATCH, "gauss", 768, NM, 100, BF16_METRICS, {}, "2chunks"),
       Case(MFMA_BATCH, "gauss", 512, NM, 40, BF16_METRICS, {"VL_MFMA_STREAM_LOADS": "0"}, "plainloads")]
    + [Case(MFMA_BATCH, "gauss", 256, 41003, 24, BF16_METRICS,
            {"VL_MFMA_GRID": "1", "VL_MFMA_STAGES": str(st), "VL_MFMA_STREAM_LOADS": str(st % 2)}, f"stages{st}")
       for st in (2, 3, 4)]
    + [Case(MFMA_BATCH, f, d, NM, 40, BF16_METRICS) for f, d in
       (("bf16edge", 384), ("scales", 256), ("cancel", 512), ("underflow", 768), ("gemm", 384))]
    + K3_CASES
)


# ---------------------------------------------------------------------------------------------
# running one case
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    vbuild.build()  # the MFMA / bf16 launchers: mfma_scan.o of the library build
    d = tmp_path_factory.mktemp("filter_audit")
    exe, obj = d / "filter_audit", d / "filter_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "filter_audit.hip"), "-o", str(obj)],
                arch + [str(obj), os.path.join(vbuild.OBJ, "mfma_scan.o"), "-o", str(exe)]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


RATIOS = {}        # (filter, metric, ld) -> largest (a) ratio
SKIPPED = {}       # (filter, metric, ld) -> [MFMA lists skipped as overflowed (exact path), lists audited]
_STATE = {"failed_child": None}


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    if RATIOS:
        lines = ["largest |key_dev - key_host| / allowance per (filter, metric, stride):"]
        for (f, m, ld), r in sorted(RATIOS.items()):
            sk, au = SKIPPED.get((f, m, ld), (0, 0))
            lines.append(f"  {f:12s} {METRIC_NAME[m]:10s} ld {ld:5d}: {r:.3g}   ({au} lists audited, {sk} overflowed lists skipped)")
        print("\n" + "\n".join(lines))


def run_case(exe, case, tmp_path):
    if _STATE["failed_child"]:
        pytest.fail(f"not started: the audit child of {_STATE['failed_child']} failed")
    rng = np.random.default_rng([case.filt, case.dim, case.n, case.nq, sum(map(ord, case.fam + case.tag))])
    rows, queries = family(case.fam, rng, case.n, case.dim, case.nq)
    src = tmp_path / "case.bin"
    out = tmp_path / "out.bin"
    mets = list(case.metrics) + [0] * (4 - len(case.metrics))
    with open(src, "wb") as f:
        f.write(struct.pack("<10I", MAGIC, case.filt, len(case.metrics), *mets, case.n, case.dim, case.nq))
        f.write(np.ascontiguousarray(rows, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(queries, dtype="<f8").tobytes())
    env = dict(os.environ)
    env.update(case.env)
    # the flag is set BEFORE the child starts and cleared only when it exits cleanly: a hang (TimeoutExpired), a crash or
    # any other exception leaves it set, so no later case starts a process on a card that may be wedged
    _STATE["failed_child"] = case.id
    r = subprocess.run([exe, str(src), str(out)], capture_output=True, text=True, timeout=180, env=env)
    if r.returncode == 0 and "audit ok" in r.stdout:
        _STATE["failed_child"] = None
    else:
        pytest.fail(f"audit child exited {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return rows, queries, out.read_bytes()


def parse_blocks(buf, n_metrics):
    blocks, off = [], 0
    for _ in range(n_metrics):
        magic, metric, nq, n, ld, *info = struct.unpack_from("<9I", buf, off)
        assert magic == MAGIC
        off += 36
        R, in_extra = struct.unpack_from("<2d", buf, off)
        off += 16

        def take(dtype, count):
            nonlocal off
            a = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
            off += a.nbytes
            return a

        b = dict(metric=metric, nq=nq, n=n, ld=ld, info=info, R=R, in_extra=in_extra)
        b["Q"] = take("<f8", nq)
        b["key"] = take("<f4", nq * KP).reshape(nq, KP).astype(np.float64)
        b["pos"] = take("<u4", nq * KP).reshape(nq, KP)
        b["bt"] = take("<f8", nq)
        b["bk"] = take("<f8", nq * KP).reshape(nq, KP)
        b["exact"] = take("<f8", nq * n).reshape(nq, n)
        blocks.append(b)
    assert off == len(buf)
    return blocks


def documented_bound(metric, t, n, R, Q, in_extra):
    """DESIGN.md §3's bound with every u-term doubled, in plain f64: the shipped B must not fall below it."""
    if metric == COS:
        return t / Q + 2.0 * (n + 4) * U + in_extra
    if metric == DOT:
        return t + (2.0 * (n + 2) * U + in_extra) * R * Q
    if metric == EUC and in_extra > 0.0:
        err = 2.0 * in_extra * R * Q + 4.0 * (n + 4) * U * (R * Q + R * R)
        return 1.0 / (1.0 + np.sqrt(np.maximum(Q * Q - t - err, 0.0)))
    ts = np.maximum(-t, 0.0)
    if metric == EUC:
        d = np.sqrt(ts) * (1.0 - 2.0 * (n + 2) * U) - 4.0 * U * (R + Q)
    else:
        d = ts * (1.0 - 2.0 * (n + 2) * U) - 4.0 * U * np.sqrt(n) * (R + Q)
    return 1.0 / (1.0 + np.maximum(d, 0.0))


# in_extra of the bf16 filters, derived: a bf16 row is x/|x| rounded f64 -> f32 -> bf16 (relative 2^-8 + 2^-23 with the
# double rounding); the single-query filter's query is f32 (2^-24), the MFMA filter's is bf16 like the rows
UB = 2.0 ** -8 + 2.0 ** -23
IN_EXTRA_MIN = {BF16_SINGLE: UB * (1.0 + U) + U, MFMA_BATCH: (2.0 + UB) * UB}


def audit_block(case, h, queries, b):
    """(a)-(d) for every query of one metric; returns the number of lists audited."""
    filt, metric, n, ld = case.filt, b["metric"], b["n"], b["ld"]
    ctx = (case.id, METRIC_NAME[metric])
    audited = 0
    skipped = 0
    worst = 0.0
    assert b["in_extra"] >= IN_EXTRA_MIN.get(filt, 0.0), (ctx, "in_extra below its derivation", b["in_extra"])
    for qi in range(b["nq"]):
        pos, key = b["pos"][qi], b["key"][qi]
        live = pos != POS_SENTINEL
        m = int(live.sum())
        if filt == MFMA_BATCH and m == 0:
            skipped += 1  # an overflowed candidate buffer: the library answers that query on the exact path
            continue
        assert live[:m].all() and not live[m:].any(), (ctx, qi, "sentinels inside the list")
        assert m == min(KP, n), (ctx, qi, m, "short list")
        p, kd = pos[:m].astype(np.int64), key[:m]
        # (d) ordering, uniqueness, range
        assert (p < n).all(), (ctx, qi, "position past the last row", p[p >= n])
        assert len(np.unique(p)) == m, (ctx, qi, "duplicate positions")
        order_ok = (kd[:-1] > kd[1:]) | ((kd[:-1] == kd[1:]) & (p[:-1] < p[1:]))
        assert order_ok.all(), (ctx, qi, "list not sorted by (key desc, pos asc)", np.nonzero(~order_ok)[0][:5])
        # (a) key fidelity
        kh, tol = host_keys(h, queries[qi], filt, metric, ld)
        err = np.abs(kd - kh[p])
        ratio = err / tol[p]
        bad = ratio > 1.0
        assert not bad.any(), (ctx, qi, "key differs from the host key beyond the allowance",
                               [(int(p[i]), kd[i], kh[p[i]], tol[p[i]]) for i in np.nonzero(bad)[0][:4]])
        worst = max(worst, float(ratio.max()))
        # the shipped bound keeps the documented terms and their 2x safety factor
        doc = documented_bound(metric, kd, ld, b["R"], b["Q"][qi], b["in_extra"])
        low = b["bk"][qi][:m] < doc - 1e-9 * np.abs(doc)
        assert not low.any(), (ctx, qi, "B(key) below the documented bound", b["bk"][qi][:m][low][:3], doc[low][:3])
        # (b) completeness
        if m < n:
            t64 = kd[-1]
            outside = np.ones(n, dtype=bool)
            outside[p] = False
            above = outside & (kh > t64 + tol)
            assert not above.any(), (ctx, qi, "rows missing from the list", t64,
                                     [(int(i), kh[i], tol[i]) for i in np.nonzero(above)[0][:4]])
            # (c) certificate: every row left out scores <= B(t64), every listed row <= B(its key)
            ex = b["exact"][qi]
            over = outside & (ex > b["bt"][qi])
            assert not over.any(), (ctx, qi, "a row outside the list beats B(t64)", b["bt"][qi],
                                    [(int(i), ex[i], kh[i]) for i in np.nonzero(over)[0][:4]])
            over_l = ex[p] > b["bk"][qi][:m]
            assert not over_l.any(), (ctx, qi, "a listed row beats B(its key)",
                                      [(int(p[i]), ex[p[i]], b["bk"][qi][i]) for i in np.nonzero(over_l)[0][:4]])
        audited += 1
    k = (FILTER_NAME[filt], metric, ld)
    RATIOS[k] = max(RATIOS.get(k, 0.0), worst)
    sk = SKIPPED.setdefault(k, [0, 0])
    sk[0] += skipped
    sk[1] += audited
    return audited


def check_ordered_construction(case, h, queries, b):
    """The host keys of query 0 rise strictly with the storage position over the whole index (fall for `ordered-l1r`), those
    of query 1 of `ordered` fall: asserted before the device is judged."""
    kh, _ = host_keys(h, queries[0], case.filt, b["metric"], b["ld"])
    step = np.diff(kh)
    ctx = (case.id, METRIC_NAME[b["metric"]], "construction")
    assert (step < 0.0).all() if case.fam == "ordered-l1r" else (step > 0.0).all(), ctx
    if case.fam == "ordered":
        kh, _ = host_keys(h, queries[1], case.filt, b["metric"], b["ld"])
        assert (np.diff(kh) < 0.0).all(), ctx


def check_lattice_exact(case, h, queries, b):
    """(e): integer inputs make every f32 partial sum exact in any order (dim <= 1536: |dot| <= 24 576, squared distance
    <= 98 304, L1 <= 12 288, all below 2^24) and the cosine key one f32 product with the device's own 1/norm, so the host
    key is the device's bit for bit and the list has to be the host's top 64 by (key desc, pos asc)."""
    n, metric = b["n"], b["metric"]
    for qi in range(b["nq"]):
        kh, _ = host_keys(h, queries[qi], case.filt, metric, b["ld"])
        if metric != COS:
            assert (kh == np.round(kh)).all() and np.abs(kh).max() < 2.0 ** 24
        kh = f32(kh)
        want = np.lexsort((np.arange(n), -kh))[:KP]
        ctx = (case.id, METRIC_NAME[metric], qi)
        got = b["pos"][qi].astype(np.int64)
        assert got.tolist() == want.tolist(), (ctx, "(e) positions", np.nonzero(got != want)[0][:4], got[:4], want[:4])
        assert (b["key"][qi] == kh[want]).all(), (ctx, "(e) key bits")


def check_case(exe, case, tmp_path):
    rows, queries, buf = run_case(exe, case, tmp_path)
    blocks = parse_blocks(buf, len(case.metrics))
    h = HostRows(rows)
    R = float(np.sqrt(dev_sumsq(rows)).max())
    for b in blocks:
        assert b["R"] == R, (case.id, "IngestStats max norm", b["R"], R)
        if case.fam.startswith("ordered"):
            check_ordered_construction(case, h, queries, b)
        audited = audit_block(case, h, queries, b)
        # an MFMA list may be empty (overflow -> exact path), but the audit must not be vacuous
        assert audited >= (b["nq"] + 1) // 2, (case.id, METRIC_NAME[b["metric"]], audited, b["nq"])
        if case.filt == F32_BATCH:
            grid, lanes = b["info"][0], b["info"][1]
            assert audited == b["nq"], (case.id, "an f32 batch list was skipped", audited)
            assert lanes == (4 if b["ld"] <= 64 else 8 if b["ld"] <= 512 else 16), (case.id, "lanes per row", b["ld"], lanes)
            if case.grid:
                assert grid == case.grid, (case.id, "grid", grid)
            if case.loops:  # rows per wave: the case is there for the mid-stream flushes
                assert b["n"] // (4 * grid) >= LOOP_ROWS, (case.id, "waves do not loop", b["n"], grid)
            if case.fam == "lattice":
                check_lattice_exact(case, h, queries, b)
        if case.filt == MFMA_BATCH:
            assert b["info"][3] == (0 if case.env.get("VL_MFMA_KERNEL") == "tile" else 1), b["info"]
            if "chunks" in case.tag:
                assert b["info"][1] >= 2, b["info"]
            if "stages" in case.tag:
                assert b["info"][2] == int(case.env["VL_MFMA_STAGES"]), b["info"]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_filter_list_against_its_bound(audit_exe, case, tmp_path):
    check_case(audit_exe, case, tmp_path)

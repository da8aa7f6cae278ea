"""Audit of the int8 single-query filter against the exactness bound it is certified with.

tests/native/filter_audit_i8.hip runs the library's own stages; every check is made here.
  rows  (1 M x 384, 200 k x 768, 50 k x 100, each with adversarial rows in front): the residual bound r of every row is at
        least the true residual |x/|x| - s k| recomputed on the host in long double; bytes, scale, padding, zero rows and
        the f32 row norm are as the conversion promises.
  keys  per case and query, with u = 2^-24 and n = ldb (the length the kernel sums):
    (a) key fidelity: every listed key equals the key host numpy computes in f64 from the same rounded inputs (the copy's
        bytes and (s, r, |x|), the query's f16 values, 2^-e, Qd and D) within the undoubled u-part (n + 5) u (sum of the
        absolute terms), and that part stays inside IN_EXTRA_I8_SINGLE / 2 x Q (cosine) or x R Q (dot);
    (b) the key is an upper bound: every row's reference score is <= its host key (/ Q for cosine);
    (c) completeness: no row outside the list has a host key above the list's 64th key plus the allowance;
    (d) certificate: every row outside the list scores <= B(t64), every listed row <= B(its key), B as documented;
    (e) ordering: (key desc, pos asc), no duplicate positions, none >= n.
The largest key error is reported as a fraction of the undoubled term.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24
KP = 64
POS_SENTINEL = 0xFFFFFFFF
MAGIC = 0x38414C56
COS, DOT = 0, 3
METRIC_NAME = {COS: "cosine", DOT: "dot"}
IN_EXTRA_I8_SINGLE = 0.000113  # mfma_scan.hpp; the binary reports the value it was compiled with
WORST = {}  # (metric, ldb) -> largest |key_dev - key_host| / (IN_EXTRA_I8_SINGLE / 2 x Q or R Q)


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    vbuild.build()  # launch_rows_i8 / prepare_i8_query / launch_scan_i8: mfma_scan.o of the library build
    d = tmp_path_factory.mktemp("filter_audit_i8")
    exe, obj = d / "filter_audit_i8", d / "filter_audit_i8.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "filter_audit_i8.hip"), "-o", str(obj)],
                arch + [str(obj), os.path.join(vbuild.OBJ, "mfma_scan.o"), "-o", str(exe)]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


_STATE = {"failed_child": None}


def run_child(args, timeout):
    """One audit child; after a child that did not exit cleanly no further one is started."""
    if _STATE["failed_child"]:
        pytest.fail(f"not started: the audit child {_STATE['failed_child']} failed")
    _STATE["failed_child"] = " ".join(args[1:3])
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    if r.returncode == 0 and "audit ok" in r.stdout:
        _STATE["failed_child"] = None
    else:
        pytest.fail(f"audit child exited {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return r.stdout


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        print("\nlargest |key_dev - key_host| / (IN_EXTRA_I8_SINGLE / 2 x Q, or x R Q for dot):")
        for (m, ldb), v in sorted(WORST.items()):
            print(f"  {METRIC_NAME[m]:7s} ldb {ldb:4d}: {v:.3g}")


# ---------------------------------------------------------------------------------------------
# rows: r against the true residual
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,seed", [(1_000_000, 384, 1), (200_000, 768, 2), (50_000, 100, 3), (20_000, 256, 4)])
def test_row_residual_bound(audit_exe, n, dim, seed):
    out = run_child([audit_exe, "rows", str(n), str(dim), str(seed)], timeout=900)
    line = next(l for l in out.splitlines() if l.startswith("rows "))
    f = dict(kv.split("=") for kv in line.split()[1:])
    print("\n" + line)
    for k in ("bad_r", "bad_byte", "bad_scale", "bad_pad", "bad_zero", "bad_norm", "bad_tail"):
        assert int(f[k]) == 0, (k, line)
    # r - true residual > 0 on every row (the ratio true / r prints as 1 where only the additive slack separates them)
    assert float(f["min_margin"]) > 0.0 and float(f["worst_ratio"]) <= 1.0, line
    # the residual of a rounded row is at most sqrt(ldb) / 254: the bound behind IN_EXTRA_I8_SINGLE
    assert float(f["max_r"]) <= float(f["r_bound"]) * (1.0 + 1e-6), line


# ---------------------------------------------------------------------------------------------
# keys: the filter's lists against the bound
# ---------------------------------------------------------------------------------------------
def unit(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def i8_edge_rows(rng, n, dim):
    rows = unit(rng, n, dim)
    t = 2.0 ** -20
    k = n // 8
    rows[0] = 0.0                                   # zero row
    rows[1] = 0.0
    rows[1, 3] = 2.0 ** -39                          # one-hot rows
    rows[2] = 0.0
    rows[2, 0] = -(2.0 ** 39)
    rows[3] = 1.0                                   # k = 127 everywhere
    # x^ / s near k + 1/2 in every column
    half = (np.arange(dim) % 127 + 0.5) * t * np.where(np.arange(dim) & 2, -1.0, 1.0)
    half[0] = 127.0 * t
    rows[4:k] = half[None, :] * rng.choice([-1.0, 1.0], size=(k - 4, dim))
    # rows on the int8 grid exactly, and sparse rows of mixed magnitude
    rows[k:2 * k] = rng.integers(-127, 128, size=(k, dim)) * 2.0 ** -7
    rows[k:2 * k, 0] = 127 * 2.0 ** -7
    sp = np.zeros((k, dim))
    for i in range(k):
        j = rng.choice(dim, size=1 + i % 5, replace=False)
        sp[i, j] = rng.standard_normal(len(j)) * 2.0 ** rng.uniform(-20, 20, size=len(j))
    rows[2 * k:3 * k] = sp
    return rows


def query_family(name, rng, nq, dim, rows):
    q = unit(rng, nq, dim)
    if name == "scaled":
        q[0::2] *= 2.0 ** -39.5
        q[1::2] *= 2.0 ** 39.5
    elif name == "range":  # entries over 40 binades: the small ones flush to 0 in f16, D takes them
        q *= 2.0 ** rng.uniform(-40.0, 0.0, size=q.shape)
    elif name == "f16half":  # values halfway between f16 neighbours after the scaling
        m = rng.integers(1024, 2048, size=q.shape) + 0.5
        q = m * rng.choice([-1.0, 1.0], size=q.shape) * 2.0 ** -12
    q[-1] = rows[5] if name != "range" else q[-1]  # a query equal to a row: a clear winner
    return q


def row_family(name, rng, n, dim):
    if name == "unit":
        return unit(rng, n, dim)
    if name == "norms":
        return unit(rng, n, dim) * 2.0 ** rng.uniform(-3.0, 3.0, size=(n, 1))
    if name == "scales":
        rows = unit(rng, n, dim) * 2.0 ** rng.uniform(-39.0, 39.0, size=(n, 1))
        return rows
    if name == "cancel":
        base = unit(rng, 1, dim)[0]
        return base[None, :] + 1e-3 * rng.standard_normal((n, dim))
    if name == "i8edge":
        return i8_edge_rows(rng, n, dim)
    raise ValueError(name)


N = 8192 + 37
CASES = ([("unit", "unit", d) for d in (100, 384, 768)]
         + [("norms", "unit", 384), ("norms", "range", 512), ("scales", "scaled", 256), ("cancel", "unit", 768),
            ("i8edge", "unit", 384), ("i8edge", "f16half", 128), ("i8edge", "range", 768), ("unit", "f16half", 384),
            ("unit", "scaled", 100)])


def parse(buf, n, nq, n_metrics):
    off = 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a

    ldb = int(take("<u4", 1)[0])
    copy = dict(ldb=ldb, k=take("u1", n * ldb).reshape(n, ldb).astype(np.int64) - 128,
                sr=take("<f4", n * 2).reshape(n, 2).astype(np.float64), nrm=take("<f4", n).astype(np.float64))
    blocks = []
    for _ in range(n_metrics):
        magic, metric, bnq, bn, ld, grid = take("<u4", 6)
        assert magic == MAGIC and bnq == nq and bn == n
        R, in_extra = take("<f8", 2)
        b = dict(metric=int(metric), ld=int(ld), grid=int(grid), R=float(R), in_extra=float(in_extra), Q=take("<f8", nq))
        b["prep"] = []
        for _ in range(nq):
            inv_scale, qd, d = take("<f4", 3).astype(np.float64)
            h = take("<u2", ldb).copy().view(np.float16).astype(np.float64)
            b["prep"].append((inv_scale, qd, d, h))
        b["key"] = take("<f4", nq * KP).reshape(nq, KP).astype(np.float64)
        b["pos"] = take("<u4", nq * KP).reshape(nq, KP)
        b["bt"] = take("<f8", nq)
        b["bk"] = take("<f8", nq * KP).reshape(nq, KP)
        b["exact"] = take("<f8", nq * n).reshape(nq, n)
        blocks.append(b)
    assert off == len(buf)
    return copy, blocks


def host_keys(copy, prep, metric):
    """(key, allowance) of every row: the kernel's key in f64 from the same rounded inputs (products of integers and f16
    values, their sums exact in f64), and the undoubled u-part of its f32 evaluation."""
    inv_scale, qd, d, q16 = prep
    k = copy["k"]
    s, r = copy["sr"][:, 0], copy["sr"][:, 1]
    p = (k @ q16) * inv_scale
    a = (np.abs(k) @ np.abs(q16)) * inv_scale
    key = s * p + (r * qd + d)
    tol = (copy["ldb"] + 5) * U * (s * a + r * qd + d)
    if metric == DOT:
        nr = copy["nrm"]
        return key * nr, tol * nr + U * np.abs(key * nr)
    return key, tol


@pytest.mark.parametrize("rows_fam,q_fam,dim", CASES, ids=[f"{a}-{b}-d{c}" for a, b, c in CASES])
def test_i8_filter_list_against_its_bound(audit_exe, rows_fam, q_fam, dim, tmp_path):
    rng = np.random.default_rng([dim, sum(map(ord, rows_fam + q_fam))])
    rows = row_family(rows_fam, rng, N, dim)
    nq = 6
    queries = query_family(q_fam, rng, nq, dim, rows)
    metrics = (COS, DOT)
    src, out = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<7I", MAGIC, len(metrics), *metrics, N, dim, nq))
        f.write(np.ascontiguousarray(rows, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(queries, dtype="<f8").tobytes())
    run_child([audit_exe, "keys", str(src), str(out)], timeout=300)
    copy, blocks = parse(out.read_bytes(), N, nq, len(metrics))
    n, ldb = N, copy["ldb"]
    for b in blocks:
        metric, ld, R = b["metric"], b["ld"], b["R"]
        ctx = (rows_fam, q_fam, dim, METRIC_NAME[metric])
        assert b["in_extra"] == IN_EXTRA_I8_SINGLE, (ctx, b["in_extra"])
        for qi in range(nq):
            Q = b["Q"][qi]
            pos, key = b["pos"][qi], b["key"][qi]
            assert (pos != POS_SENTINEL).all(), (ctx, qi, "short list")
            p, kd = pos.astype(np.int64), key
            # (e) ordering, uniqueness, range
            assert (p < n).all() and len(np.unique(p)) == KP, (ctx, qi)
            assert ((kd[:-1] > kd[1:]) | ((kd[:-1] == kd[1:]) & (p[:-1] < p[1:]))).all(), (ctx, qi, "list order")
            kh, tol = host_keys(copy, b["prep"][qi], metric)
            # (a) key fidelity, and the per-row term inside the shipped constant's undoubled half
            undoubled = IN_EXTRA_I8_SINGLE / 2.0 * (Q if metric == COS else R * Q)
            assert (tol <= undoubled * (1.0 + 1e-9)).all(), (ctx, qi, "per-row evaluation term above the constant",
                                                             float(tol.max()), undoubled)
            err = np.abs(kd - kh[p])
            bad = err > tol[p]
            assert not bad.any(), (ctx, qi, "key differs from the host key beyond the allowance",
                                   [(int(p[i]), kd[i], kh[p[i]], tol[p[i]]) for i in np.nonzero(bad)[0][:4]])
            w = (metric, ldb)
            WORST[w] = max(WORST.get(w, 0.0), float(err.max() / undoubled))
            # (b) the key bounds the reference score from above (in real arithmetic, the same rounded inputs)
            ex = b["exact"][qi]
            if metric == COS:
                over = ex > kh / Q + 1e-12
            else:
                over = ex > kh + 2.0 * U * np.abs(kh) + 1e-12 * (1.0 + R * Q)
            assert not over.any(), (ctx, qi, "a row scores above its key", [(int(i), ex[i], kh[i]) for i in np.nonzero(over)[0][:4]])
            # (c) completeness
            t64 = kd[-1]
            outside = np.ones(n, dtype=bool)
            outside[p] = False
            above = outside & (kh > t64 + tol)
            assert not above.any(), (ctx, qi, "rows missing from the list", [(int(i), kh[i]) for i in np.nonzero(above)[0][:4]])
            # (d) certificate with the shipped constant, and B no lower than documented
            if metric == COS:
                doc = kd / Q + 2.0 * (ld + 4) * U + IN_EXTRA_I8_SINGLE
            else:
                doc = kd + (2.0 * (ld + 2) * U + IN_EXTRA_I8_SINGLE) * R * Q
            assert (b["bk"][qi] >= doc - 1e-9 * np.abs(doc)).all(), (ctx, qi, "B(key) below the documented bound")
            assert not (outside & (ex > b["bt"][qi])).any(), (ctx, qi, "a row outside the list beats B(t64)")
            assert not (ex[p] > b["bk"][qi]).any(), (ctx, qi, "a listed row beats B(its key)")

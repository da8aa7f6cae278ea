"""Audit of the lists k_scan_subset_jobs writes -- the scan of a filtered batch, many (query, position list) jobs in one
launch.

The end-to-end tests cannot see a list that lost a row: the bound check sends that job to the exact kernels and the answer
is still right (tests/test_gpu_filter_audit.py makes the same point about the 8-query batch scan).  So the lists
themselves are audited.  tests/native/subset_jobs_audit.hip ingests one case, runs ONE launch of the jobs scan with a given
number of workgroups per job (gx), merges each job's gx lists with the library's k_merge_lists and writes one 64-entry
list per job -- and, beside it, the list of k_scan_subset launched alone on the same position list and query.  Per job:
  (d) structure: (key desc, pos asc), no duplicates, every position a member of the job's list, min(64, m) live entries
      followed by sentinels;
  (s) the list equals the lone k_scan_subset's list bit for bit, positions and key bits (every family);
  (e) lattice rows (small integers: every f32 partial sum is exact, so the host key is the device's bit for bit): the list
      is exactly the host's top 64 of the job's rows by (key desc, position asc) -- the whole subset when m < 64;
  (b) ordered rows (keys rising with the position): no row of the job outside the list has a host key above the list's
      64th key plus the existing audit's allowance (n + 4) u sum|terms|.
Within one launch the jobs' sizes sit on the kernel's boundaries (1, one wave step -1/0/+1, one full iteration of the whole
job grid -1/0/+1, 63, 64, 65, every row), so some workgroups have no step, some exactly one, some loop with a partial last
step; the lists are contiguous, strided, at the very end of the slab (position n - 1 included) and shared between jobs.
"""
import os
import struct
import subprocess
from dataclasses import dataclass

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24
TINY = 2.0 ** -126
KP = 64
POS_SENTINEL = 0xFFFFFFFF
MAGIC = 0x4A534C56
COS, EUC, MAN, DOT = 0, 1, 2, 3
METRIC_NAME = {COS: "cosine", EUC: "euclidean", MAN: "manhattan", DOT: "dot"}
ALL4 = (COS, EUC, MAN, DOT)
JOBS_VARIANT_BASE = 6_000_000
N = 4133  # the last row sits in a partial step at every shape

# float4 per row -> (lanes per row G, row groups in flight U) of the stride's default shape (VL_SCAN_VARIANTS)
DEFAULT_SHAPES = {32: (8, 3), 64: (8, 2), 96: (8, 1), 128: (8, 1), 192: (16, 1), 256: (16, 1), 384: (16, 1)}


def shape_of(dim):
    ld4 = (dim + 3) // 4
    if ld4 in DEFAULT_SHAPES:
        return DEFAULT_SHAPES[ld4] + (True,)
    g = 1
    while g < 64 and g * 2 <= ld4:
        g *= 2
    return g, 1, False


# ---- host model of what the kernel reads (tests/test_gpu_filter_audit.py) -------------------------------------------
def dev_sumsq(x):
    """Sum of squares of every row in k_ingest's order: lane l adds columns l, l + 64, ..., then a butterfly."""
    n, d = x.shape
    w = -(-d // 64) * 64
    p = np.zeros((n, w))
    p[:, :d] = x
    p = p.reshape(n, w // 64, 64)
    s = np.zeros((n, 64))
    for j in range(w // 64):
        s = s + p[:, j, :] * p[:, j, :]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, 0]


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


class HostRows:
    def __init__(self, rows):
        nrm = np.sqrt(dev_sumsq(rows))
        self.x32 = f32(rows)
        with np.errstate(divide="ignore"):
            self.inv_norm = f32(np.where(nrm > 0.0, 1.0 / nrm, 0.0))  # k_ingest: (float)(1.0 / norm)


def host_keys(h, q, metric, n_acc):
    """(key, allowance) of every row: the kernel's key in f64 from the same rounded inputs, and (n + 4) u sum|terms|."""
    g = (n_acc + 4) * U
    q32 = f32(q)
    if metric in (COS, DOT):
        p = h.x32 @ q32
        a = np.abs(h.x32) @ np.abs(q32)
        if metric == COS:
            return p * h.inv_norm, (g * a + n_acc * TINY) * h.inv_norm
        return p, g * a + n_acc * TINY
    d = h.x32 - q32[None, :]
    s = np.sum(d * d, axis=1) if metric == EUC else np.sum(np.abs(d), axis=1)
    return -s, g * s + n_acc * TINY


def unit(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def family(name, rng, n, dim, nq):
    if name == "gauss":
        return rng.standard_normal((n, dim)), rng.standard_normal((nq, dim))
    if name == "ordered":  # cosine / dot / Euclidean keys of query 0 rise with the storage position, those of query 1 fall
        q0 = unit(rng, 1, dim)[0]
        x = unit(rng, n, dim)
        x = x[np.argsort(x @ q0, kind="stable")]
        across = x - (x @ q0)[:, None] * q0[None, :]
        across /= np.linalg.norm(across, axis=1, keepdims=True)
        t = np.linspace(-0.9, 0.9, n)
        rows = t[:, None] * q0[None, :] + np.sqrt(1.0 - t * t)[:, None] * across
        q = rng.standard_normal((nq, dim))
        q[0] = q0
        q[1] = -q0
        return rows, q
    if name == "lattice":  # small integers: every f32 partial sum is exact in any order, and the keys tie massively
        rows = rng.integers(-4, 5, size=(n, dim)).astype(np.float64)
        rows[~rows.any(axis=1), 0] = 1.0
        q = rng.integers(-4, 5, size=(nq, dim)).astype(np.float64)
        q[~q.any(axis=1), 0] = 1.0
        return rows, q
    raise ValueError(name)


# ---- cases ----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    fam: str
    dim: int
    n_jobs: int
    gx: int
    metrics: tuple = ALL4

    @property
    def id(self):
        return f"{self.fam}-d{self.dim}-j{self.n_jobs}-gx{self.gx}"


def boundary_sizes(dim, gx, n):
    g, u, _ = shape_of(dim)
    rps = 64 // g
    it = 4 * u * rps * gx  # rows one iteration of a job's whole grid scores
    sizes = [1, rps - 1, rps, rps + 1, it - 1, it, it + 1, 63, 64, 65, n]
    return [min(max(s, 1), n) for s in sizes]


def build_jobs(case, rng, n, nq):
    """(pool, jobs [n_jobs, 3] = (query, offset, m)): contiguous, strided and end-of-slab lists whose sizes cycle through
    the boundary sizes; every fifth job shares the list of the job before it (another query), and the same query meets
    different lists."""
    sizes = boundary_sizes(case.dim, case.gx, n)
    pool, jobs, off = [], [], 0
    for j in range(case.n_jobs):
        q = (j // 2) % nq  # consecutive jobs share a query, under different lists
        if j % 5 == 4 and jobs:  # the list of the job before it, under another query
            jobs.append(((q + 1) % nq, jobs[-1][1], jobs[-1][2]))
            continue
        m = sizes[(j + case.n_jobs) % len(sizes)] if case.n_jobs < len(sizes) else sizes[j % len(sizes)]
        kind = j % 3
        if kind == 0:    # at the very end of the slab: position n - 1 included
            pl = np.arange(n - m, n)
        elif kind == 1:  # strided over the whole slab
            pl = np.arange(m) * (n // m)
        else:            # contiguous, somewhere inside
            a = int(rng.integers(0, n - m + 1))
            pl = np.arange(a, a + m)
        pool.append(pl.astype(np.uint32))
        jobs.append((q, off, m))
        off += m
    return np.concatenate(pool), np.asarray(jobs, dtype=np.uint32)


# one dim per specialised stride (128 ... 1536 floats), two generic ones (3, and 900: longer than 768, served by no variant)
SPECIAL_DIMS = (128, 256, 384, 512, 768, 1024, 1536)
CASES = tuple(
    # every dim: 512 jobs through all the boundary sizes, and 9 jobs at the finalize kernel's 64 lists
    [Case("lattice", d, 512, 2) for d in SPECIAL_DIMS + (3, 900)]
    + [Case("lattice", d, 9, 64) for d in SPECIAL_DIMS + (3, 900)]
    + [Case("gauss", d, 9, 1) for d in SPECIAL_DIMS + (3, 900)]
    # one job and two, one workgroup and many; more than 64 lists per job (eight jobs or fewer: the merge levels)
    + [Case("lattice", 384, 1, 1), Case("lattice", 384, 1, 64), Case("lattice", 126, 2, 2), Case("gauss", 384, 2, 64),
       Case("lattice", 768, 2, 200), Case("gauss", 50, 8, 130), Case("lattice", 384, 512, 1), Case("gauss", 384, 512, 32)]
    + [Case("ordered", d, 9, g, (COS, EUC, DOT)) for d, g in ((384, 2), (768, 1), (1536, 64), (50, 2))]
)


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    d = tmp_path_factory.mktemp("subset_jobs_audit")
    exe = d / "subset_jobs_audit"
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "subset_jobs_audit.hip"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


_STATE = {"failed_child": None}


def run_case(exe, case, tmp_path):
    if _STATE["failed_child"]:
        pytest.fail(f"not started: the audit child of {_STATE['failed_child']} failed")
    rng = np.random.default_rng([case.dim, case.n_jobs, case.gx, sum(map(ord, case.fam))])
    nq = 6
    rows, queries = family(case.fam, rng, N, case.dim, nq)
    pool, jobs = build_jobs(case, rng, N, nq)
    src, out = tmp_path / "case.bin", tmp_path / "out.bin"
    mets = list(case.metrics) + [0] * (4 - len(case.metrics))
    with open(src, "wb") as f:
        f.write(struct.pack("<12I", MAGIC, len(case.metrics), *mets, N, case.dim, nq, case.n_jobs, case.gx, pool.size))
        f.write(np.ascontiguousarray(rows, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(queries, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(pool, dtype="<u4").tobytes())
        f.write(np.ascontiguousarray(jobs, dtype="<u4").tobytes())
    # the flag is set BEFORE the child starts and cleared only when it exits cleanly: a hang (TimeoutExpired), a crash or
    # any other exception leaves it set, so no later case starts a process on a card that may be wedged
    _STATE["failed_child"] = case.id
    r = subprocess.run([exe, str(src), str(out)], capture_output=True, text=True, timeout=120)
    if r.returncode == 0 and "audit ok" in r.stdout:
        _STATE["failed_child"] = None
    else:
        pytest.fail(f"audit child exited {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return rows, queries, pool, jobs, out.read_bytes()


def parse_blocks(buf, n_metrics):
    blocks, off = [], 0
    for _ in range(n_metrics):
        magic, metric, n_jobs, gx, variant, lone_variant = struct.unpack_from("<4I2i", buf, off)
        assert magic == MAGIC
        off += 24
        b = {"metric": metric, "n_jobs": n_jobs, "gx": gx, "variant": variant, "lone_variant": lone_variant}
        for name in ("", "lone_"):
            b[name + "key"] = np.frombuffer(buf, dtype="<f4", count=n_jobs * KP, offset=off).reshape(n_jobs, KP)
            off += n_jobs * KP * 4
            b[name + "pos"] = np.frombuffer(buf, dtype="<u4", count=n_jobs * KP, offset=off).reshape(n_jobs, KP)
            off += n_jobs * KP * 4
        blocks.append(b)
    assert off == len(buf)
    return blocks


def check_job(ctx, case, b, j, plist, kh, tol):
    pos, key = b["pos"][j], b["key"][j]
    m = plist.size
    live = pos != POS_SENTINEL
    c = int(live.sum())
    # (d) structure
    assert live[:c].all() and not live[c:].any(), (ctx, "sentinels inside the list")
    assert c == min(KP, m), (ctx, "live entries", c, m)
    p, kd = pos[:c].astype(np.int64), key[:c]
    assert np.isin(p, plist).all(), (ctx, "a position outside the job's list", p[~np.isin(p, plist)][:4])
    assert len(np.unique(p)) == c, (ctx, "duplicate positions")
    order_ok = (kd[:-1] > kd[1:]) | ((kd[:-1] == kd[1:]) & (p[:-1] < p[1:]))
    assert order_ok.all(), (ctx, "list not sorted by (key desc, pos asc)", np.nonzero(~order_ok)[0][:5])
    # (s) the lone k_scan_subset's list, bit for bit
    assert pos.tolist() == b["lone_pos"][j].tolist(), (ctx, "(s) positions differ from k_scan_subset's")
    assert key[:c].view(np.uint32).tolist() == b["lone_key"][j][:c].view(np.uint32).tolist(), (ctx, "(s) key bits")
    if case.fam == "lattice":  # (e)
        k32 = f32(kh[plist])
        if b["metric"] != COS:
            assert (k32 == kh[plist]).all() and np.abs(k32).max() < 2.0 ** 24
        want = np.lexsort((plist, -k32))[:KP]
        assert p.tolist() == plist[want].tolist(), (ctx, "(e) positions", p[:6], plist[want][:6])
        assert (kd == k32[want]).all(), (ctx, "(e) key bits")
    if case.fam == "ordered" and c < m:  # (b)
        t64 = kd[-1]
        outside = np.setdiff1d(plist, p)
        above = outside[kh[outside] > t64 + tol[outside]]
        assert above.size == 0, (ctx, "(b) rows missing from the list", t64, [(int(i), kh[i], tol[i]) for i in above[:4]])


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_jobs_scan_lists(audit_exe, case, tmp_path):
    rows, queries, pool, jobs, buf = run_case(audit_exe, case, tmp_path)
    blocks = parse_blocks(buf, len(case.metrics))
    h = HostRows(rows)
    g, u, special = shape_of(case.dim)
    ld = (case.dim + 3) // 4 * 4
    sizes = set(int(x) for x in jobs[:, 2])
    if case.n_jobs >= 11:
        assert sizes >= set(boundary_sizes(case.dim, case.gx, N)), "the launch misses a boundary size"
    for b in blocks:
        assert b["n_jobs"] == case.n_jobs and b["gx"] == case.gx
        # the shape that ran is the one the sizes were computed for
        if special:
            assert b["variant"] // 10000 == JOBS_VARIANT_BASE // 10000 + g and b["variant"] % 100 == u, b["variant"]
        else:
            assert b["variant"] == -(JOBS_VARIANT_BASE + g), b["variant"]
        keys = {}
        for j in range(case.n_jobs):
            q, off, m = (int(x) for x in jobs[j])
            if q not in keys:
                keys[q] = host_keys(h, queries[q], b["metric"], ld)
            kh, tol = keys[q]
            plist = pool[off:off + m].astype(np.int64)
            name = "the first job" if j == 0 else "the last job" if j == case.n_jobs - 1 else f"job {j}"
            check_job((case.id, METRIC_NAME[b["metric"]], name, f"m={m}"), case, b, j, plist, kh, tol)
        if case.fam == "ordered":  # the construction: query 0's keys rise with the position, query 1's fall
            assert (np.diff(keys[0][0]) > 0.0).all() and (np.diff(keys[1][0]) < 0.0).all()

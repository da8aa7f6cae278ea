"""Host model of the rounded inputs the candidate filters read, and the case families of their audits.

Shared by tests/test_gpu_filter_audit.py and the batched range audit (tests/_range_batch_cases.py): the device's norms,
1/norm and bf16 rows bit for bit, every filter's key in f64 from those inputs with the u-part of its bound, and the
families of rows and queries.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126  # absolute allowance per term: f32 products and sums below the normal range
KP = 64
POS_SENTINEL = 0xFFFFFFFF
MAGIC = 0x41464C56
COS, EUC, MAN, DOT = 0, 1, 2, 3
F32_QARG, F32_Q64, F32_BATCH, BF16_SINGLE, MFMA_BATCH = range(5)


# ---------------------------------------------------------------------------------------------
# host model of the rounded inputs the kernels read
# ---------------------------------------------------------------------------------------------
def dev_sumsq(x):
    """Sum of squares of every row in the device's order (k_ingest, k_rows_bf16*): lane l adds columns l, l + 64, ...,
    then a butterfly over the 64 lanes -- so the norms, 1/norm and the bf16 rows here are the device's bit for bit."""
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


def bf16_rne(a32):
    """f32 -> bf16 (round to nearest even), returned as f32 values (finite inputs)."""
    b = np.ascontiguousarray(a32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


class HostRows:
    def __init__(self, rows):
        self.rows = rows
        ss = dev_sumsq(rows)
        nrm = np.sqrt(ss)
        self.x32 = f32(rows)
        with np.errstate(divide="ignore"):
            inv = np.where(nrm > 0.0, 1.0 / nrm, 0.0)
        self.inv_norm = f32(inv)                                      # k_ingest: (float)(1.0 / norm)
        self.xh = bf16_rne((rows * inv[:, None]).astype(np.float32)).astype(np.float64)  # x/|x| -> f32 -> bf16
        self.nr = f32(nrm)                                            # |x| and |x|^2 rounded once to f32
        self.sq = f32(ss)


def host_keys(h, q, filt, metric, n_acc):
    """(key, allowance) of every row for query q: the kernel's key in f64 from the same rounded inputs, and the undoubled
    u-part of the bound for that row."""
    g = (n_acc + 4) * U
    if filt in (F32_QARG, F32_Q64, F32_BATCH):
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
    qv = f32(q) if filt == BF16_SINGLE else bf16_rne(f32(q).astype(np.float32)).astype(np.float64)
    p = h.xh @ qv
    a = np.abs(h.xh) @ np.abs(qv)
    if metric == COS:
        return p, g * a + n_acc * TINY
    if metric == DOT:
        return p * h.nr, (g * a + n_acc * TINY) * h.nr
    return 2.0 * p * h.nr - h.sq, (g * a + n_acc * TINY) * 2.0 * h.nr + g * h.sq


# ---------------------------------------------------------------------------------------------
# case families
# ---------------------------------------------------------------------------------------------
def unit(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def halfway(rng, shape, scale):
    """f32 values whose low 16 bits are 0x8000: exactly halfway between two bf16 neighbours."""
    v = (rng.standard_normal(shape) * scale).astype(np.float32).view(np.uint32)
    v = (v & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    return v.view(np.float32).astype(np.float64)


def family(name, rng, n, dim, nq):
    if name == "gauss":
        return rng.standard_normal((n, dim)), rng.standard_normal((nq, dim))
    if name == "scales":  # row norms over the whole domain 2^-40 .. 2^40, queries at both ends
        rows = unit(rng, n, dim) * 2.0 ** rng.uniform(-39.9, 39.9, size=(n, 1))
        rows[5] = 0.0
        rows[5, 0] = 2.0 ** -40
        rows[n // 2] = 0.0
        rows[n // 2, 1] = 2.0 ** 40
        q = unit(rng, nq, dim)
        q[0::2] *= 2.0 ** -39.9
        q[1::2] *= 2.0 ** 39.9
        return rows, q
    if name == "cancel":  # a big common component, a small distinct part, queries nearly orthogonal to it
        base = unit(rng, 1, dim)[0]
        rows = base[None, :] + 1e-3 * rng.standard_normal((n, dim))
        q = rng.standard_normal((nq, dim))
        q -= (q @ base)[:, None] * base[None, :]
        q += 1e-7 * base[None, :]
        q[0] = rows[3] - (rows[3] @ base) * base + 1e-7 * base  # the distinct part of one row: a clear winner
        return rows, q
    if name == "underflow":  # row norms ~2^-40 spread over every column, plus f64 subnormals
        rows = unit(rng, n, dim) * 2.0 ** -39.5  # still >= 2^-40 once 5 % of the columns are subnormal
        mask = rng.random((n, dim)) < 0.05
        rows[mask] = rng.choice([-1.0, 1.0], size=mask.sum()) * 5e-324 * rng.integers(1, 1 << 40, size=mask.sum())
        # a third of the rows: norm ~2^-40 in ONE column, the others 2^-100 .. 2^-155 -- f32 subnormal inputs, inputs that
        # round to 0, and (against the tiny queries) products and differences below the f32 normal range
        t = np.arange(0, n, 3)
        rows[t] = rng.choice([-1.0, 1.0], size=(len(t), dim)) * 2.0 ** rng.uniform(-155.0, -100.0, size=(len(t), dim))
        rows[t, rng.integers(0, dim, size=len(t))] = 2.0 ** -39.9
        q = unit(rng, nq, dim)
        q[1::2] *= 2.0 ** -39.9
        q[0, ::7] = 1e-310
        return rows, q
    if name == "bf16edge":  # x/|x| exactly halfway between bf16 neighbours, and close to +-1
        rows = np.zeros((n, dim))
        h = n // 2
        rows[:h, : dim - 4] = halfway(rng, (h, dim - 4), 0.9 / np.sqrt(dim))
        rest = np.maximum(1.0 - np.sum(rows[:h] ** 2, axis=1), 0.0)
        rows[:h, dim - 4:] = np.sqrt(rest / 4.0)[:, None] * rng.choice([-1.0, 1.0], size=(h, 4))
        rows[h:] = 1e-3 * unit(rng, n - h, dim)
        j = rng.integers(0, dim, size=n - h)
        sign = rng.choice([-1.0, 1.0], size=n - h)
        top = np.where(rng.random(n - h) < 0.5, 1.0 - 2.0 ** -9, 1.0 - 2.0 ** -30)
        rows[h + np.arange(n - h), j] = sign * top
        rows *= 2.0 ** rng.integers(-5, 6, size=(n, 1))  # exact scaling: x/|x| unchanged
        q = halfway(rng, (nq, dim), 1.0)
        q[0] = rows[7]
        q[1] = rows[h + 3]
        return rows, q
    if name == "gemm":  # GEMM-form Euclidean: |q| far below and far above the row norms
        rows = unit(rng, n, dim) * 2.0 ** rng.uniform(0.0, 4.0, size=(n, 1))
        q = unit(rng, nq, dim)
        q[0::2] *= 2.0 ** -12
        q[1::2] *= 2.0 ** 12
        return rows, q
    if name == "ordered":  # cosine / dot / Euclidean keys of query 0 rise with the storage position, those of query 1 fall
        q0 = unit(rng, 1, dim)[0]
        x = unit(rng, n, dim)
        x = x[np.argsort(x @ q0, kind="stable")]
        # The sorted gaussian projections have gaps far below one f32 rounding of a key somewhere among n rows, so the
        # component along q0 is respaced evenly (gap 1.8 / n, thousands of roundings); the part across q0 stays and the
        # rows stay unit: x.q0 = t, cos = t, -|x - q0|^2 = 2t - 2 all rise with t, and -q0 turns every one of them round.
        across = x - (x @ q0)[:, None] * q0[None, :]
        across /= np.linalg.norm(across, axis=1, keepdims=True)
        t = np.linspace(-0.9, 0.9, n)
        rows = t[:, None] * q0[None, :] + np.sqrt(1.0 - t * t)[:, None] * across
        q = rng.standard_normal((nq, dim))
        q[0] = q0
        q[1] = -q0
        return rows, q
    if name in ("ordered-l1", "ordered-l1r"):  # Manhattan keys of query 0 rise (-l1r: fall) with the storage position
        q0 = unit(rng, 1, dim)[0]
        d = unit(rng, n, dim) - q0[None, :]
        l1 = np.abs(d).sum(axis=1)
        order = np.argsort(-l1, kind="stable")  # farthest first
        d, l1 = d[order], l1[order]
        # respaced like `ordered`: every row's offset from q0 is scaled to an evenly spaced L1 distance
        target = np.linspace(1.25 * l1[0], 0.75 * l1[-1], n)
        rows = q0[None, :] + d * (target / l1)[:, None]
        q = rng.standard_normal((nq, dim))
        q[0] = q0
        return (rows[::-1].copy() if name == "ordered-l1r" else rows), q
    if name == "lattice":  # small integers: every f32 partial sum is exact in any order, and the keys tie massively
        rows = rng.integers(-4, 5, size=(n, dim)).astype(np.float64)
        rows[~rows.any(axis=1), 0] = 1.0
        q = rng.integers(-4, 5, size=(nq, dim)).astype(np.float64)
        q[~q.any(axis=1), 0] = 1.0
        return rows, q
    raise ValueError(name)

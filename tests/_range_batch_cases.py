"""Cases, host model and judges of the batched range search audit.

tests/native/range_batch_audit.hip runs the fixed-threshold MFMA pass and the k_rbatch_* tail on the inputs built here and
dumps every buffer whole; tests/test_gpu_range_batch_audit.py judges the dumps with the functions below, and
tests/test_range_batch_model_cpu.py shows the tail model right against FlatOracle and checks every construction's
preconditions without a GPU.  What the expectations about the ring stand on is read from k_mfma_rows<.., MODE 1>: a wave's
32-row block appends 32 entries per query whose threshold every row reaches, the wave flushes its segment after a block
once it holds RS_SEG / 2 entries, and a segment that was asked to hold more than RS_SEG entries marks every query of the
workgroup's chunk with cap + 1.
"""
import os
import re
import struct
from dataclasses import dataclass, field

import numpy as np

from _filter_host_model import (U, TINY, COS, EUC, MAN, DOT, MFMA_BATCH, HostRows, bf16_rne, dev_sumsq, f32, family,  # noqa: F401
                                host_keys)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = 0x42524C56
PASS, TAIL, CHAIN = 0, 1, 2
GUARD = 256
PAT8, PAT32, PAT64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
RBATCH_SEG = 2048
CAND_CAP = 4096
CTR_TOTAL, CTR_NAN, CTR_OFF, CTR_WANT = 0, 1, 2, 3
FLAG_EXACT, FLAG_BOUNDS = 1, 2
RANGE_KEYS_ALL, RANGE_KEYS_FROM, RANGE_KEYS_NONE = 0, 1, 2
METRIC_NAME = {COS: "cosine", EUC: "euclidean", MAN: "manhattan", DOT: "dot"}
ALL4 = (COS, EUC, MAN, DOT)
MFMA_METRICS = (COS, EUC, DOT)
FLT_MAX = np.finfo(np.float32).max
INF32 = np.float32(np.inf)
CUS = 256  # compute units of an MI355X: the default grid is CUS / chunks workgroups per chunk at most


def _constant(name):
    with open(os.path.join(ROOT, "vectorlite_amd", "csrc", "mfma_scan.hpp")) as f:
        return float(re.search(r"constexpr double %s = ([0-9.]+);" % name, f.read()).group(1))


IN_EXTRA_MFMA = _constant("IN_EXTRA_MFMA")
IN_EXTRA_BF16_SINGLE = _constant("IN_EXTRA_BF16_SINGLE")


def mfma_ldb(dim):
    return next(s for s in (128, 256, 384, 512, 768) if dim <= s)


def qpc(ldb):
    """Queries per chunk (rs_qpb)."""
    return 96 if ldb == 768 else 128


def rs_seg(ldb):
    """Entries of a wave's ring segment (rs_seg)."""
    return 128 if ldb == 768 else 192


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def succ32(a):
    return np.nextafter(np.asarray(a, dtype=np.float32), INF32)


def seq_norm(q):
    """|q| as the host stages a query: sequential sum of squares."""
    ss = 0.0
    for v in np.asarray(q, dtype=np.float64):
        ss += v * v
    return float(np.sqrt(ss))


# ---------------------------------------------------------------------------------------------
# the MFMA key of every (query, row), step by step in f32
# ---------------------------------------------------------------------------------------------
def query_bf16(queries):
    return bf16_rne(f32(queries).astype(np.float32)).astype(np.float64)


def mfma_keys32(h, queries, metric, need_exact=True):
    """[nq, n] f32 keys as k_mfma_rows forms them from sums that are exact in any order: acc = x^.q (exact), cosine: acc,
    dot: acc * |x|, Euclidean: (2 acc) * |x| - |x|^2, one f32 rounding per operation.  need_exact: asserts that every
    partial sum of every row is an integer below 2^24 in units of the row's smallest bf16 ulp."""
    qv = query_bf16(queries)
    acc = qv @ h.xh.T
    if need_exact:
        a = np.abs(h.xh)
        mn = np.where(a > 0, a, np.inf).min(axis=1)
        unit = 2.0 ** (np.floor(np.log2(mn)) - 7)
        assert np.isfinite(unit).all() and (h.xh / unit[:, None] == np.round(h.xh / unit[:, None])).all()
        assert (qv == np.round(qv)).all(), "queries must be integers"
        assert ((np.abs(qv) @ a.T) / unit[None, :] < 2.0 ** 24).all(), "a partial sum could round"
    acc = acc.astype(np.float32)
    if metric == COS:
        return acc + np.float32(0.0)
    nr, sq = h.nr.astype(np.float32)[None, :], h.sq.astype(np.float32)[None, :]
    if metric == DOT:
        return acc * nr + np.float32(0.0)
    return (np.float32(2.0) * acc) * nr - sq + np.float32(0.0)


# ---------------------------------------------------------------------------------------------
# cases and their file formats
# ---------------------------------------------------------------------------------------------
@dataclass
class Case:
    kind: int
    name: str
    metrics: tuple
    rows: np.ndarray
    queries: np.ndarray
    cap: int
    emit_cap: int = 0
    thr: dict = field(default_factory=dict)         # pass: metric -> list of f32 [nq]
    cand_pos: dict = field(default_factory=dict)    # tail: metric -> u32 [nq, cap]
    cnt: dict = field(default_factory=dict)         # tail: metric -> u32 [nq]
    min_scores: dict = field(default_factory=dict)  # tail, chain: metric -> f64 [nq]
    grid: int = 0
    stream: int = 1
    flags: int = 0
    note: dict = field(default_factory=dict)        # what the judge of the case needs to know

    @property
    def n(self):
        return self.rows.shape[0]

    @property
    def dim(self):
        return self.rows.shape[1]

    @property
    def nq(self):
        return self.queries.shape[0]

    @property
    def ldb(self):
        return mfma_ldb(self.dim)

    @property
    def n_thr(self):
        return 1 if self.kind == CHAIN else (len(self.thr[self.metrics[0]]) if self.kind == PASS else 0)

    def expected_info(self):
        """(ksteps, chunks, grid_x, stages) the launcher must report."""
        chunks = -(-self.nq // qpc(self.ldb))
        n_blk = -(-self.n // 32)
        return [self.ldb // 16, chunks, max(1, min(-(-n_blk // 8), self.grid or max(1, CUS // chunks))), 1]


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<2I", MAGIC, len(cases)))
        for c in cases:
            mets = list(c.metrics) + [0] * (4 - len(c.metrics))
            f.write(struct.pack("<16I", c.kind, len(c.metrics), *mets, c.n, c.dim, c.nq, c.cap, c.emit_cap, c.n_thr, c.grid,
                                c.stream, c.flags, 0))
            f.write(np.ascontiguousarray(c.rows, dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(c.queries, dtype="<f8").tobytes())
            for m in c.metrics:
                if c.kind == PASS:
                    for t in c.thr[m]:
                        assert t.shape == (c.nq,)
                        f.write(bits32(t).astype("<u4").tobytes())
                elif c.kind == TAIL:
                    assert c.cand_pos[m].shape == (c.nq, c.cap) and c.cnt[m].shape == (c.nq,)
                    f.write(np.ascontiguousarray(c.cand_pos[m], dtype="<u4").tobytes())
                    f.write(np.ascontiguousarray(c.cnt[m], dtype="<u4").tobytes())
                if c.kind != PASS:
                    f.write(np.ascontiguousarray(c.min_scores[m], dtype="<f8").tobytes())


def parse_output(buf, cases):
    """-> per case: {metric: block}."""
    off = 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a

    def guarded(dtype, count):
        a = take(dtype, count)
        return a, take("u1", GUARD)

    out = []
    for c in cases:
        per = {}
        for m in c.metrics:
            magic, kind, metric, nq, nq_pad, n, ldb, cap, emit_cap, n_thr, flags, out_n = take("<u4", 12).tolist()
            assert (magic, kind, metric, nq, n, cap, emit_cap, n_thr) == (MAGIC, c.kind, m, c.nq, c.n, c.cap, c.emit_cap, c.n_thr), c.name
            b = dict(nq_pad=nq_pad, ldb=ldb, out_n=out_n, R=float(take("<f8", 1)[0]), Q=take("<f8", nq), passes=[])
            for _ in range(n_thr if kind != TAIL else 0):
                p = dict(info=take("<u4", 4).tolist(), thr=take("<f4", nq), staged=take("<u4", nq))
                p["cnt"], p["cnt_guard"] = guarded("<u4", nq_pad)
                cand, p["cand_guard"] = guarded("<u4", nq * cap * 2)
                cand = cand.reshape(nq, cap, 2)
                p["key_bits"], p["pos"] = cand[:, :, 0], cand[:, :, 1]
                p["key"] = np.ascontiguousarray(p["key_bits"]).view(np.float32)
                if flags & FLAG_BOUNDS:
                    p["b_key"] = take("<f8", nq * cap).reshape(nq, cap)
                    p["b_pred"] = take("<f8", nq)
                b["passes"].append(p)
            if flags & FLAG_EXACT:
                b["exact"] = take("<f8", nq * n).reshape(nq, n)
            if kind != PASS:
                t = {}
                ctr, t["ctr_guard"] = guarded("<u4", nq * 4)
                t["ctr"] = ctr.reshape(nq, 4)
                t["out_pos"], t["out_pos_guard"] = guarded("<u4", out_n)
                t["out_scores"], t["out_scores_guard"] = guarded("<u8", out_n)
                sv, t["sv_score_guard"] = guarded("<u8", nq * RBATCH_SEG)
                t["sv_score"] = sv.reshape(nq, RBATCH_SEG)
                sv, t["sv_pos_guard"] = guarded("<u4", nq * RBATCH_SEG)
                t["sv_pos"] = sv.reshape(nq, RBATCH_SEG)
                b["tail"] = t
            per[m] = b
        out.append(per)
    assert off == len(buf), (off, len(buf))
    return out


# ---------------------------------------------------------------------------------------------
# judging a pass
# ---------------------------------------------------------------------------------------------
def guards_clean(d, names):
    for k in names:
        assert (d[k] == PAT8).all(), (k, "the guard behind the buffer was written")


def judge_pass(case, metric, b, p, want_sets, want_keys=None, marked=None, key_tol=None):
    """One dumped pass against, per query, the set of rows it must list: want_sets[q] = sorted positions, want_keys [nq, n]
    the keys they must carry (bits, -0.0 taken as +0.0) or, with key_tol [nq, n], carry within that allowance.  marked[q]:
    the query must report cnt > cap instead (its entries are then only checked to be valid and distinct).
    Returns the number of queries judged."""
    ctx = (case.name, METRIC_NAME[metric])
    nq, n, cap = case.nq, case.n, case.cap
    assert p["info"] == case.expected_info(), (ctx, "launch shape", p["info"], case.expected_info())
    guards_clean(p, ("cnt_guard", "cand_guard"))
    assert (p["cnt"][nq:] == 0).all(), (ctx, "a padding query's counter moved", p["cnt"][nq:])
    for q in range(nq):
        cnt = int(p["cnt"][q])
        pos, kb, key = p["pos"][q], p["key_bits"][q], p["key"][q]
        if marked is not None and marked[q]:
            assert cnt > cap, (ctx, q, "not marked", cnt)
            continue
        want = want_sets[q]
        if len(want) > cap:  # the buffer overflowed: the count says so, and the buffer is full of valid, distinct candidates
            assert cnt > cap, (ctx, q, "a full buffer is not reported", cnt, len(want))
            got = pos.astype(np.int64)
            assert len(np.unique(got)) == cap and np.isin(got, want).all(), (ctx, q, "full buffer holds a wrong or double row")
            continue
        assert cnt == len(want), (ctx, q, "cnt", cnt, "rows that reach the threshold", len(want), float(p["thr"][q]))
        assert (pos[cnt:] == PAT32).all() and (kb[cnt:] == PAT32).all(), (ctx, q, "an entry past cnt was written")
        order = np.argsort(pos[:cnt], kind="stable")
        got = pos[:cnt][order].astype(np.int64)
        assert (got < n).all(), (ctx, q, "position past the last row", got[got >= n][:4])
        assert (np.diff(got) > 0).all(), (ctx, q, "a row is listed twice")
        assert got.tolist() == list(want), (ctx, q, "candidate set", sorted(set(got) ^ set(want))[:6])
        gk = key[:cnt][order]
        if want_keys is not None and key_tol is None:
            assert (bits32(gk + np.float32(0.0)) == bits32(want_keys[q][got])).all(), (ctx, q, "key bits")
        elif want_keys is not None:
            bad = np.abs(gk.astype(np.float64) - want_keys[q][got]) > key_tol[q][got]
            assert not bad.any(), (ctx, q, "key beyond the allowance", got[bad][:4])
    return nq


def rank_thresholds(keys32, ranks):
    """Per query (cycling through `ranks`, None = +inf) the key of that rank in descending order, clamped to the last row:
    (on the key: the tie is in, on its f32 successor: the tie is out)."""
    nq, n = keys32.shape
    on = np.full(nq, np.inf, dtype=np.float32)
    for q in range(nq):
        r = ranks[q % len(ranks)]
        if r is not None:
            on[q] = np.sort(keys32[q])[::-1][min(r, n) - 1]
    return on, succ32(on)


def sets_at(keys, thr):
    return [np.nonzero(keys[q] >= thr[q])[0] for q in range(len(thr))]


def predict_marks(case, keys, thr):
    """Which queries the pass must mark because a wave's ring segment overflows, from exact keys: workgroup x of a chunk's
    gx workgroups gives its wave w the 32-row blocks x + gx (w + 8 i); a block adds its (row, query of the chunk) pairs
    with key >= thr to the wave's count; after a block the wave flushes once it holds RS_SEG / 2, and a flush of more than
    RS_SEG marks every query of the chunk."""
    ldb, per = case.ldb, qpc(case.ldb)
    gx, n_blk = case.expected_info()[2], -(-case.n // 32)
    hit = (keys >= np.asarray(thr)[:, None]) & (keys > -np.inf)
    pad = np.zeros((case.nq, n_blk * 32), dtype=np.int64)
    pad[:, :case.n] = hit
    marked = np.zeros(case.nq, dtype=bool)
    for c0 in range(0, case.nq, per):
        per_block = pad[c0:c0 + per].sum(axis=0).reshape(n_blk, 32).sum(axis=1)
        over = False
        for x in range(gx):
            for w in range(8):
                held = 0
                for b in range(x + gx * w, n_blk, gx * 8):
                    held += int(per_block[b])
                    if held >= rs_seg(ldb) // 2:
                        over |= held > rs_seg(ldb)
                        held = 0
        marked[c0:c0 + per] = over
    return marked


# ---- 3.1: lattice, every shape ---------------------------------------------------------------------------------------
PASS_DIMS = (100, 128, 256, 300, 512, 700, 768)
GRID1_TAILS = (0, 1, 15, 16, 17, 31)   # n = 8 * 32 * 4 + r under VL_MFMA_GRID=1: every wave loops 4-5 blocks, the last one masked
SMALL_N = (1, 31, 33, 255)             # default grid: one partial block, idle waves, fewer blocks than waves
RANKS = (None, 1, 5, 40, 300)
# 128 queries at these ranks put 128 * 69 / 33 = 270 candidates into every 32-row block: under one workgroup every segment
# of 192 overflows and the whole chunk is marked -- as predict_marks says it must be.  The same shapes run a second time
# at ranks that the ring holds, so that the looping waves' lists are judged entry by entry as well.
RANKS_LIGHT = (None, 1, 5, 40)
RANKS_LIGHT_SMALL = (None, None, None, 1, 2)  # for the indexes of one to eight blocks


def light_ranks(n):
    return RANKS_LIGHT if n >= 1024 else RANKS_LIGHT_SMALL


def nq_list(ldb):
    return (95, 96, 97, 193) if ldb == 768 else (1, 2, 127, 128, 129, 257)


def lattice_shapes(dim):
    """(n, nq, grid, stream) of the dimension's lattice cases."""
    di, nqs = PASS_DIMS.index(dim), nq_list(mfma_ldb(dim))
    shapes = [(1024 + r, nqs[(i + di) % len(nqs)], 1, (i + di) % 2) for i, r in enumerate(GRID1_TAILS)]
    shapes += [(n, nqs[(i + di + 2) % len(nqs)], 0, (i + di + 1) % 2) for i, n in enumerate(SMALL_N)]
    return shapes


def lattice_case(dim, n, nq, grid, stream, cap=512, ranks=RANKS):
    rng = np.random.default_rng([31, dim, n, nq])
    rows, queries = family("lattice", rng, n, dim, nq)
    c = Case(PASS, f"lattice-d{dim}-n{n}-q{nq}-g{grid}-s{stream}-r{max(r or 0 for r in ranks)}", MFMA_METRICS, rows, queries, cap, grid=grid,
             stream=stream)
    h = HostRows(rows)
    for m in c.metrics:
        keys = mfma_keys32(h, queries, m)
        on, above = rank_thresholds(keys, ranks)
        c.thr[m] = [on, above]
        c.note[m] = keys
        for t in (on, above):  # precondition: nothing here is about a full buffer
            assert max(len(s) for s in sets_at(keys, t)) <= cap, c.name
    return c


def judge_lattice(case, blocks):
    """Returns (queries judged, those among them whose list was compared entry by entry: no segment overflows)."""
    judged = exact = 0
    for m in case.metrics:
        keys = case.note[m]
        for p, t in zip(blocks[m]["passes"], case.thr[m]):
            assert (bits32(p["thr"]) == bits32(t)).all()
            marked = predict_marks(case, keys, t)
            judged += judge_pass(case, m, blocks[m], p, sets_at(keys, t), keys, marked)
            exact += int((~marked).sum())
    return judged, exact


# ---- 3.2: rounded inputs ---------------------------------------------------------------------------------------------
ROUNDED_FAMILIES = ("gauss", "bf16edge", "scales", "gemm")
ROUNDED_DIMS = (128, 256, 384, 512, 768)
GAP_RANKS = (1, 5, 40, 150)  # 24 queries: about 37 candidates per 32-row block, under every flush threshold


def host_model(h, queries, metric, ldb):
    kt = [host_keys(h, q, MFMA_BATCH, metric, ldb) for q in queries]
    return np.stack([k for k, _ in kt]), np.stack([t for _, t in kt])


def gap_thresholds(kh, tol, ranks):
    """Per query an f32 threshold between two consecutive host keys near the wanted rank that every row's key misses by
    more than twice its allowance: no row is undetermined.  Asserts that such a gap exists."""
    nq, n = kh.shape
    thr = np.zeros(nq, dtype=np.float32)
    for q in range(nq):
        order = np.argsort(-kh[q], kind="stable")
        ks = kh[q][order]
        r = min(ranks[q % len(ranks)], n - 1)
        found = False
        for i in sorted(range(1, n), key=lambda i: abs(i - r)):
            t = np.float32(0.5 * (ks[i - 1] + ks[i]))
            if ks[i - 1] > float(t) > ks[i] and (np.abs(kh[q] - float(t)) > 2.0 * tol[q]).all():
                thr[q], found = t, True
                break
        assert found, ("no gap wider than twice the allowance", q)
    return thr


def rounded_case(fam, dim, n=1003, nq=24, grid=1, stream=1, ranks=GAP_RANKS, cap=1024, name=None):
    rng = np.random.default_rng([32, dim, n, nq, sum(map(ord, fam))])
    rows, queries = family(fam, rng, n, dim, nq)
    c = Case(PASS, name or f"{fam}-d{dim}-n{n}-q{nq}-g{grid}-s{stream}", MFMA_METRICS, rows, queries, cap, grid=grid, stream=stream,
             flags=FLAG_EXACT | FLAG_BOUNDS)
    h = HostRows(rows)
    for m in c.metrics:
        kh, tol = host_model(h, queries, m, c.ldb)
        c.thr[m] = [gap_thresholds(kh, tol, ranks)]
        c.note[m] = (kh, tol)
    return c


def judge_rounded(case, blocks, marked_allowed=False):
    """(a) the candidate set is the host model's, (b) every key within the allowance, (c) the certificate.  marked_allowed:
    a query may instead be marked (cnt > cap); returns (queries judged, queries marked)."""
    judged = n_marked = 0
    R = float(np.sqrt(dev_sumsq(case.rows)).max())
    for m in case.metrics:
        b, (kh, tol) = blocks[m], case.note[m]
        p, t = b["passes"][0], case.thr[m][0]
        assert b["R"] == R and b["Q"].tolist() == [seq_norm(q) for q in case.queries], (case.name, "R, Q")
        want = sets_at(kh, t.astype(np.float64))
        marked = (p["cnt"][:case.nq] > case.cap) if marked_allowed else None
        judged += judge_pass(case, m, b, p, want, kh, marked, tol)
        for q in range(case.nq):
            if marked is not None and marked[q]:
                n_marked += 1
                continue
            ex, cnt = b["exact"][q], int(p["cnt"][q])
            out = np.ones(case.n, dtype=bool)
            out[want[q]] = False
            assert not (ex[out] > p["b_pred"][q]).any(), (case.name, m, q, "a row left out beats B(pred(thr))")
            lp = p["pos"][q][:cnt].astype(np.int64)
            assert not (ex[lp] > p["b_key"][q][:cnt]).any(), (case.name, m, q, "a candidate beats B(its key)")
    return judged, n_marked


def rerun_case(case, blocks, grid, stream):
    """(d): the case again under another grid and load form, with the first run's reported keys as thresholds (the entry in
    the middle of every list: on it, and on its successor)."""
    c = Case(PASS, case.name + f"-again-g{grid}-s{stream}", case.metrics, case.rows, case.queries, case.cap, grid=grid, stream=stream)
    for m in case.metrics:
        p = blocks[m]["passes"][0]
        on = np.full(case.nq, np.inf, dtype=np.float32)
        for q in range(case.nq):
            cnt = int(p["cnt"][q])
            if cnt:
                on[q] = np.sort(p["key"][q][:cnt])[cnt // 2]
        c.thr[m] = [on, succ32(on)]
        c.note[m] = p
    return c


def judge_rerun(case, blocks):
    """The second run lists exactly the first run's entries with key >= thr, with identical key bits."""
    judged = 0
    for m in case.metrics:
        first = case.note[m]
        for p, t in zip(blocks[m]["passes"], case.thr[m]):
            keys = np.full((case.nq, case.n), -np.inf, dtype=np.float32)
            for q in range(case.nq):
                cnt = int(first["cnt"][q])
                keys[q, first["pos"][q][:cnt]] = first["key"][q][:cnt] + np.float32(0.0)
            judged += judge_pass(case, m, blocks[m], p, sets_at(keys, t), keys)
    return judged


# ---- 3.3: the edge of the bf16 slack ----------------------------------------------------------------------------------
EDGE_DIMS = (128, 384, 768)
EDGE_LOSS = 0.0075
# squared components, powers of 4, that sum to S = 127/128 + 2^-14 = 16257 / 4^7: a unit vector along them has every
# component at 2^k (1 + t'), t' = S^-1/2 - 1 = 0.99799 * 2^-8 -- just under the bf16 rounding boundary 2^k (1 + 2^-8) at the
# bottom of its binade, so the row's bf16 copy loses t' / (1 + t') of every component
EDGE_EXPONENTS = [-1] * 3 + [-2] * 3 + [-3] * 3 + [-4] * 2 + [-7]
EDGE_T = 0.998 * 2.0 ** -8  # the query is not normalised: its components are scaled by 1 + t themselves
EDGE_VARIANTS = 6


def edge_direction(n_comp):
    e = sorted(EDGE_EXPONENTS, reverse=True)
    while len(e) < n_comp:  # 4^k = 4 * 4^(k-1): more, smaller components, the same sum
        e = sorted(e[1:] + [e[0] - 1] * 4, reverse=True)
    b = 2.0 ** np.array(e, dtype=np.float64)
    assert float((b * b).sum()) == 127.0 / 128.0 + 2.0 ** -14
    return b


def edge_case(dim):
    """Planted pair j: row = rho_j b_j, query = Qs_j (1 + t) b_j with b_j the direction above on columns of its own.  The
    filler rows are shorter than every planted row, so R is a planted norm and R / |x| <= 1.2 for every planted row."""
    rng = np.random.default_rng([33, dim])
    n_fill = 203
    rows = rng.standard_normal((n_fill + EDGE_VARIANTS, dim))
    rows *= 0.5 / np.linalg.norm(rows, axis=1, keepdims=True)
    queries = np.zeros((EDGE_VARIANTS, dim))
    planted = []
    for j in range(EDGE_VARIANTS):
        b = edge_direction((12, 12, 24, 48, 12, 96)[j])
        if j == 0:
            cols = np.arange(len(b))                      # the first K-step
        elif j == 1:
            cols = dim - 1 - np.arange(len(b))            # the last columns
        else:
            cols = rng.permutation(dim)[:len(b)]          # over every K-step
        sign = np.ones(len(b)) if j < 2 else rng.choice([-1.0, 1.0], size=len(b))
        pos = (n_fill + j) if j % 2 else j * 31           # among the fillers, and the last rows (a masked block)
        rho, qs = (3.0, 2.75, 2.5, 3.0, 2.75, 2.5)[j], 2.0 ** (j - 2)
        rows[pos] = 0.0
        rows[pos, cols] = rho * sign * b
        queries[j, cols] = qs * (1.0 + EDGE_T) * sign * b
        planted.append(pos)
    c = Case(PASS, f"edge-d{dim}", MFMA_METRICS, rows, queries, 256, flags=FLAG_EXACT | FLAG_BOUNDS)
    c.note["planted"] = planted
    return c


def edge_product_and_key(case, metric):
    """(exact x.q, the key's part that stands for it) of every planted pair, from the host model."""
    h = HostRows(case.rows)
    out = []
    for j, pos in enumerate(case.note["planted"]):
        kh, _ = host_keys(h, case.queries[j], MFMA_BATCH, metric, case.ldb)
        x, q = case.rows[pos], case.queries[j]
        exact = float(x @ q)
        if metric == COS:
            exact /= float(np.linalg.norm(x))
            part = kh[pos]
        elif metric == DOT:
            part = kh[pos]
        else:
            part = 0.5 * (kh[pos] + h.sq[pos])
        out.append((exact, float(part)))
    return out


def slack_share(metric, exact_score, key, b_key, ldb, R, Q):
    """(exact - key) / (B(key) - key) in the space the bound is linear in: the cosine / dot score itself, and for Euclidean
    the GEMM form |q|^2 - |x - q|^2 (score_bound.hpp: s_lo = Q^2 - key - err)."""
    if metric == COS:
        return (exact_score - key / Q) / (b_key - key / Q)
    if metric == DOT:
        return (exact_score - key) / (b_key - key)
    err = 2.0 * IN_EXTRA_MFMA * R * Q + 4.0 * (ldb + 4) * U * (R * Q + R * R)
    d = 1.0 / exact_score - 1.0
    return (Q * Q - d * d - key) / err


# ---- 3.4: ring and capacity --------------------------------------------------------------------------------------------
RING_N = 1041
RING_DIMS = (128, 384, 512, 768)
HOT = np.float32(-FLT_MAX)


def ring_case(dim, n_hot, metric_keys=None):
    """VL_MFMA_GRID=1, two chunks: n_hot queries of chunk 0 take every row; its other queries have their threshold directly
    above their largest key (no candidate: a full segment has no room for one); chunk 1's queries cut at ranks."""
    ldb = mfma_ldb(dim)
    nq = qpc(ldb) + 9
    rng = np.random.default_rng([34, dim])
    rows, queries = family("lattice", rng, RING_N, dim, nq)
    c = Case(PASS, f"ring-d{dim}-hot{n_hot}", MFMA_METRICS, rows, queries, CAND_CAP, grid=1)
    hot = (np.arange(n_hot) * 17) % qpc(ldb)  # spread over the chunk's query blocks
    h = HostRows(rows)
    for m in c.metrics:
        keys = mfma_keys32(h, queries, m)
        on, _ = rank_thresholds(keys, (5, 40, 1, None, 300))
        thr = on.copy()
        thr[:qpc(ldb)] = succ32(keys[:qpc(ldb)].max(axis=1))
        thr[hot] = HOT
        c.thr[m] = [thr]
        c.note[m] = keys
    c.note["hot"] = hot
    c.note["per_block"] = 32 * n_hot
    return c


def carry_case(dim, k):
    """Always-hot queries and k queries that are hot only on the rows of each wave's SECOND block (rows 256 .. 511 under one
    workgroup of 8 waves): column `dim - 1` is 1 there and 0 elsewhere, and those queries are a multiple of its unit
    vector, so their key is positive there and <= 0 elsewhere."""
    ldb = mfma_ldb(dim)
    always = 1 if ldb == 768 else 2
    nq = qpc(ldb) + 5
    rng = np.random.default_rng([35, dim, k])
    rows, queries = family("lattice", rng, RING_N, dim, nq)
    rows[:, dim - 1] = 0.0
    rows[256:512, dim - 1] = 1.0
    rows[~rows.any(axis=1), 0] = 1.0
    region = 20 + 16 * np.arange(k)
    queries[region] = 0.0
    queries[region, dim - 1] = 2.0 ** 14  # Euclidean: 2 M - |x|^2 > 0 on the region (|x|^2 <= 16 dim), -|x|^2 < 0 elsewhere
    c = Case(PASS, f"carry-d{dim}-k{k}", MFMA_METRICS, rows, queries, CAND_CAP, grid=1)
    h = HostRows(rows)
    for m in c.metrics:
        keys = mfma_keys32(h, queries, m, need_exact=False)  # the region queries are one product per row: exact as well
        on, _ = rank_thresholds(keys, (5, None, 40))
        thr = on.copy()
        thr[:qpc(ldb)] = succ32(keys[:qpc(ldb)].max(axis=1))
        thr[np.arange(always) * 7] = HOT
        thr[region] = np.float32(2.0 ** -100)
        c.thr[m] = [thr]
        c.note[m] = keys
        for q in region:
            assert (np.nonzero(keys[q] >= thr[q])[0] == np.arange(256, 512)).all(), (c.name, m)
    first, second = 32 * always, 32 * (always + k)
    assert first < rs_seg(ldb) // 2, "the first block must not flush"
    c.note["second_block_total"] = first + second
    return c


def ring_marked(case, fill):
    """Which queries the ring must mark when a wave's segment is asked to hold `fill` entries: all of chunk 0, or none."""
    over = fill > rs_seg(case.ldb)
    return np.arange(case.nq) < (qpc(case.ldb) if over else 0)


def judge_ring(case, blocks, fill):
    judged = 0
    marked = ring_marked(case, fill)
    for m in case.metrics:
        keys, p, t = case.note[m], blocks[m]["passes"][0], case.thr[m][0]
        judged += judge_pass(case, m, blocks[m], p, sets_at(keys, t), keys, marked)
        if not marked.any():
            assert (p["cnt"][:case.nq] <= case.cap).all(), (case.name, "marked without an overflow")
    return judged


# ---------------------------------------------------------------------------------------------
# the tail: host model, cases, judge
# ---------------------------------------------------------------------------------------------
def pair_scores(calc, metric, rows, q, positions):
    """calc's score of every listed position (clamped below n as the kernel clamps it)."""
    p = np.minimum(np.asarray(positions, dtype=np.int64), len(rows) - 1)
    uniq, inv = np.unique(p, return_inverse=True)
    return np.array([calc(metric, rows[i], q) for i in uniq], dtype=np.float64)[inv], p


def tail_model(calc, metric, rows, queries, cand_pos, cnt, cap, min_scores, emit_cap):
    """Per query: survivors (position, score bits) as a sorted multiset, total, the NaN flag, want, off and the emitted
    (position, score bits) in (score desc with -0.0 == +0.0, position asc) order."""
    res, off = [], 0
    for q in range(len(queries)):
        m = int(cnt[q])
        r = dict(total=0, nan=0, want=0, off=0, sv_pos=np.zeros(0, np.int64), sv_bits=np.zeros(0, np.uint64),
                 out_pos=np.zeros(0, np.int64), out_bits=np.zeros(0, np.uint64))
        if 0 < m <= cap:
            sc, p = pair_scores(calc, metric, rows, queries[q], cand_pos[q][:m])
            keep = sc >= min_scores[q]
            r["nan"] = int(np.isnan(sc).any())
            r["total"] = int(keep.sum())
            sp, ss = p[keep], sc[keep]
            order = np.lexsort((sp, -(ss + 0.0)))  # x + 0.0 turns -0.0 into +0.0: the two tie and leave by position
            r["sv_pos"], r["sv_bits"] = sp[order], bits64(ss[order])
            if not r["nan"] and r["total"] <= RBATCH_SEG:
                r["want"] = min(r["total"], emit_cap)
            r["out_pos"], r["out_bits"] = r["sv_pos"][:r["want"]], r["sv_bits"][:r["want"]]
        r["off"] = off
        off += r["want"]
        res.append(r)
    return res


def judge_tail(case, metric, t, model):
    """The dumped tail against the model; returns the number of queries judged."""
    ctx = (case.name, METRIC_NAME[metric])
    guards_clean(t, ("ctr_guard", "out_pos_guard", "out_scores_guard", "sv_score_guard", "sv_pos_guard"))
    packed = 0
    for q, r in enumerate(model):
        ctr = t["ctr"][q].tolist()
        want = [r["total"], r["nan"], r["off"], r["want"]]
        assert ctr == want, (ctx, q, "ctr (total, nan, off, want)", ctr, want)
        o, w = r["off"], r["want"]
        assert t["out_pos"][o:o + w].tolist() == r["out_pos"].tolist(), (ctx, q, "emitted positions")
        assert t["out_scores"][o:o + w].tolist() == r["out_bits"].tolist(), (ctx, q, "emitted score bits")
        packed = o + w
        # the survivor segment: the first min(total, RBATCH_SEG) slots hold survivors (all of them up to RBATCH_SEG, in
        # the order the atomics handed the slots out), the others are untouched
        held = min(r["total"], RBATCH_SEG)
        sp, sb = t["sv_pos"][q], t["sv_score"][q]
        assert (sp[held:] == PAT32).all() and (sb[held:] == PAT64).all(), (ctx, q, "survivor slot past the count written")
        got = np.stack([sp[:held].astype(np.uint64), sb[:held]], axis=1)
        exp = np.stack([r["sv_pos"].astype(np.uint64), r["sv_bits"]], axis=1)
        if r["total"] <= RBATCH_SEG:
            assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, exp.tolist())), (ctx, q, "survivors")
        else:
            assert set(map(tuple, got.tolist())) <= set(map(tuple, exp.tolist())), (ctx, q, "a stored survivor is none")
    assert (t["out_pos"][packed:] == PAT32).all() and (t["out_scores"][packed:] == PAT64).all(), (ctx, "written behind the packed answers")
    return len(model)


def tail_case(name, metric, rows, queries, cand_pos, cnt, cap, min_scores, emit_cap):
    nq = len(queries)
    pos = np.full((nq, cap), 0x7FFFFFF0, dtype=np.uint32)  # what lies past cnt must never be read as a row
    for q in range(nq):
        k = min(len(cand_pos[q]), cap)
        pos[q, :k] = cand_pos[q][:k]
    return Case(TAIL, name, (metric,), rows, queries, cap, emit_cap, cand_pos={metric: pos},
                cnt={metric: np.asarray(cnt, dtype=np.uint32)}, min_scores={metric: np.asarray(min_scores, dtype=np.float64)})


def mixed_rows(rng, n, dim):
    """Small integers over 2: scores tie massively and every product is exact."""
    rows = rng.integers(-3, 4, size=(n, dim)).astype(np.float64) / 2.0
    rows[~rows.any(axis=1), 0] = 0.5
    return rows


TAIL_DIMS = (1, 47, 48, 49, 192, 384, 768)
TAIL_CNTS = (0, 1, 15, 16, 17, 127, 128, 129)     # and cap, cap + 1 (cap = 130)
TAIL_TOTALS = (0, 1, 2, 3, 2047, 2048, 2049, 4096)
TAIL_NQS = (1, 255, 256, 257, 2048)


def tail_cnt_cases(dim):
    """Every metric at this width: one query per candidate count, all of them survivors (min_score = -inf)."""
    cap, n = 130, 300
    cases = []
    for metric in ALL4:
        rng = np.random.default_rng([36, dim, metric])
        rows = mixed_rows(rng, n, dim)
        cnts = list(TAIL_CNTS) + [cap, cap + 1]
        queries = rng.integers(-3, 4, size=(len(cnts), dim)).astype(np.float64)
        cand = [rng.integers(0, n, size=cap) for _ in cnts]
        cases.append(tail_case(f"tail-cnt-d{dim}-{METRIC_NAME[metric]}", metric, rows, queries, cand, cnts, cap,
                               [-np.inf] * len(cnts), RBATCH_SEG))
    return cases


def split_by_score(calc, metric, rows, q, frac):
    """(cut, rows with score >= cut, rows below) with about `frac` of the rows in; cut is one of the scores."""
    sc = np.array([calc(metric, r, q) for r in rows])
    cut = np.sort(sc)[::-1][max(0, int(frac * len(rows)) - 1)]
    return float(cut), np.nonzero(sc >= cut)[0], np.nonzero(sc < cut)[0]


def tail_total_case(calc, metric, emit_cap=RBATCH_SEG, totals=TAIL_TOTALS, dim=48):
    """One query per number of survivors among 4096 candidates: `total` of them drawn from the rows at or above the cut
    (which lies ON a score), the others from the rows below it, shuffled."""
    rng = np.random.default_rng([37, metric, emit_cap, len(totals)])
    n, cap = 300, CAND_CAP
    rows = mixed_rows(rng, n, dim)
    queries = rng.integers(-3, 4, size=(len(totals), dim)).astype(np.float64)
    queries[~queries.any(axis=1), 0] = 1.0
    cand, cuts = [], []
    for q, total in enumerate(totals):
        cut, above, below = split_by_score(calc, metric, rows, queries[q], 0.3)
        assert len(above) and len(below)
        cand.append(rng.permutation(np.concatenate([rng.choice(above, size=total), rng.choice(below, size=cap - total)])))
        cuts.append(cut)
    return tail_case(f"tail-total-{METRIC_NAME[metric]}-e{emit_cap}", metric, rows, queries, cand, [cap] * len(totals), cap, cuts,
                     emit_cap)


def tail_nq_case(calc, metric, nq, dim=47):
    """Many queries with 0 .. cap + 1 candidates and 3 emitted at most: the packed output and its offsets."""
    rng = np.random.default_rng([38, metric, nq])
    n, cap = 300, 4
    rows = mixed_rows(rng, n, dim)
    queries = rng.integers(-3, 4, size=(nq, dim)).astype(np.float64)
    cnts = rng.integers(0, cap + 2, size=nq)
    cand = [rng.integers(0, n, size=cap) for _ in range(nq)]
    cut = float(np.median([calc(metric, rows[i], queries[0]) for i in range(n)]))
    return tail_case(f"tail-nq{nq}-{METRIC_NAME[metric]}", metric, rows, queries, cand, cnts, cap, [cut] * nq, 3)


def tail_cut_case(calc, metric, dim=49):
    """min_score on a candidate's score (in), on its f64 successor (out), -inf and +inf."""
    rng = np.random.default_rng([39, metric])
    n, cap = 300, 64
    rows = mixed_rows(rng, n, dim)
    q0 = rng.integers(-3, 4, size=dim).astype(np.float64)
    q0[0] = 1.0
    queries = np.tile(q0, (4, 1))
    cand = [rng.permutation(n)[:cap]] * 4
    sc = np.sort([calc(metric, rows[i], q0) for i in cand[0]])
    on = float(sc[cap // 2])
    return tail_case(f"tail-cut-{METRIC_NAME[metric]}", metric, rows, queries, cand, [cap] * 4, cap,
                     [on, float(np.nextafter(on, np.inf)), -np.inf, np.inf], RBATCH_SEG)


def tail_tie_case(metric, dim=192):
    """Runs of identical rows that straddle the tiles of 16 candidates, listed in scrambled order; one position listed
    twice; under dot also rows of +0.0 and of -0.0 (scores +0.0 and -0.0 against a positive query)."""
    rng = np.random.default_rng([40, metric])
    n, cap = 120, 100
    rows = mixed_rows(rng, n, dim)
    rows[10:31] = rows[10]
    rows[50:83] = rows[50]
    queries = np.abs(rng.integers(1, 4, size=(3, dim)).astype(np.float64))
    if metric == DOT:
        rows[90:94] = 0.0
        rows[94:98] = -0.0
        rows[98] = 0.0
    c0 = rng.permutation(np.arange(5, 100))[:cap]
    c1 = np.concatenate([rng.permutation(np.arange(86, 100)), [97, 91, 12, 12]])   # position 12 twice, 97 and 91 twice
    c2 = rng.permutation(np.concatenate([np.arange(8, 35), np.arange(8, 35)]))     # every position twice
    cnts = [len(c0), len(c1), len(c2)]
    return tail_case(f"tail-ties-{METRIC_NAME[metric]}", metric, rows, queries, [c0, c1, c2], cnts, cap, [-np.inf] * 3, RBATCH_SEG)


def tail_nan_case(metric, dim=384):
    """Query 1 lists a row that holds a NaN: its flag, want = 0, and the neighbours' offsets as if it had no answer."""
    rng = np.random.default_rng([41, metric])
    n, cap = 60, 40
    rows = mixed_rows(rng, n, dim)
    rows[7, dim // 2] = np.nan
    queries = rng.integers(-3, 4, size=(3, dim)).astype(np.float64)
    queries[:, dim // 2] = 1.0
    cand = [np.arange(8, 8 + cap), np.arange(0, cap), np.arange(20, 20 + cap)]
    return tail_case(f"tail-nan-{METRIC_NAME[metric]}", metric, rows, queries, cand, [cap, cap, cap], cap, [-np.inf] * 3, 16)


# ---- 3.6: chain ---------------------------------------------------------------------------------------------------------
CHAIN_DIMS = (256, 512)


def chain_case(calc_rank, dim, n=RING_N, nq=129, emit_cap=64):
    """Gaussian unit rows; min_scores from the oracle's own ranking of every query (calc_rank(metric, rows, q) -> positions,
    scores in rank order): ON the score of a rank that cycles through 1, 5 and 20; one query of chunk 0 at rank 300; +inf and
    -inf for two queries; the one query of chunk 1 takes every row (few enough candidates per 32-row block that no ring
    segment is expected to overflow -- the judge does not depend on that)."""
    rng = np.random.default_rng([42, dim])
    rows, queries = family("gauss", rng, n, dim, nq)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    c = Case(CHAIN, f"chain-d{dim}", MFMA_METRICS, rows, queries, CAND_CAP, emit_cap, flags=0)
    for m in c.metrics:
        ranks, ms = [], np.zeros(nq)
        for q in range(nq):
            pos, sc = calc_rank(m, rows, queries[q])
            ranks.append((pos, sc))
            ms[q] = sc[(1, 5, 20)[q % 3] - 1]
        ms[3] = ranks[3][1][299]
        ms[7], ms[8] = np.inf, -np.inf
        ms[nq - 1] = ranks[nq - 1][1][n - 1]
        c.min_scores[m] = ms
        c.note[m] = ranks
    return c


def judge_chain(case, blocks):
    """Steps 2-5 of the pipeline on one set of buffers.  Returns (queries the device answered, queries it handed back)."""
    answered = handed = 0
    for m in case.metrics:
        b = blocks[m]
        p, t = b["passes"][0], b["tail"]
        guards_clean(p, ("cnt_guard", "cand_guard"))
        guards_clean(t, ("ctr_guard", "out_pos_guard", "out_scores_guard", "sv_score_guard", "sv_pos_guard"))
        assert p["info"] == case.expected_info(), (case.name, p["info"])
        off = 0
        for q in range(case.nq):
            ctx = (case.name, METRIC_NAME[m], q)
            pos, sc = case.note[m][q]
            ms = case.min_scores[m][q]
            keep = sc >= ms
            total, nan, o, want = t["ctr"][q].tolist()
            cnt = int(p["cnt"][q])
            assert o == off and nan == 0, (ctx, "offset / NaN flag", o, off, nan)
            off += want
            if not p["staged"][q]:  # no key is provably out: search_range_batch_mfma peels the query off before the launch
                assert ms == -np.inf and cnt == 0 and total == 0 and want == 0, ctx
                handed += 1
            elif cnt > case.cap:    # a full buffer or ring segment: left alone
                assert total == 0 and want == 0, (ctx, "a marked query was rescored")
                handed += 1
            else:
                assert total == int(keep.sum()), (ctx, "total", total, int(keep.sum()), cnt)
                if total > RBATCH_SEG:
                    assert want == 0, ctx
                    handed += 1
                    continue
                assert want == min(total, case.emit_cap), (ctx, "want", want)
                assert t["out_pos"][o:o + want].tolist() == pos[:want].tolist(), (ctx, "positions")
                assert t["out_scores"][o:o + want].tolist() == bits64(sc[:want]).tolist(), (ctx, "score bits")
                answered += 1
        assert (t["out_pos"][off:] == PAT32).all(), (case.name, "written behind the packed answers")
    return answered, handed


def with_cap(case, cap):
    """The same pass case with smaller candidate buffers."""
    return Case(PASS, f"{case.name}-cap{cap}", case.metrics, case.rows, case.queries, cap, thr=case.thr, note=case.note,
                grid=case.grid, stream=case.stream)

"""Synthetic candidate lists for the merge / finalize / selection launchers, and the host model that judges them.

Shared by tests/test_gpu_finalize_audit.py (which runs the cases through tests/native/finalize_audit.hip on the GPU) and
tests/test_finalize_model_cpu.py (which shows the model right against FlatOracle before it judges a kernel).  Nothing
here has a tolerance: every comparison is on bits or integers.

The model, per query (FINALIZE, BATCH) or per search (MULTI):
  merged candidates  the top 64 of the union of the lists by (key desc, position asc); n_cand = the real entries
  scores             oracle.calculate(metric, row, query) per candidate
  ranking            (score desc with -0.0 == +0.0, position asc); k_eff = min(k, n_rows)
  flags              rank_check_emit / k_merge_finalize_multi restated, with B handed in (the tool's device value)
  writes             pos / score of ranks < min(k_eff, n_cand), n_out = k_eff, flags, seq iff asked, the sink planes;
                     every other byte of what the tool dumps keeps its 0xA5 fill
"""
import struct
from dataclasses import dataclass

import numpy as np

KP = 64
POS_SENTINEL = 0xFFFFFFFF
MAGIC = 0x4E464C56
FINALIZE, MULTI, BATCH, SELECT = range(4)
MODE_NAME = {FINALIZE: "finalize", MULTI: "multi", BATCH: "batch", SELECT: "select"}
COS, EUC, MAN, DOT = 0, 1, 2, 3
ALL4 = (COS, EUC, MAN, DOT)
METRIC_NAME = {COS: "cosine", EUC: "euclidean", MAN: "manhattan", DOT: "dot"}
NEEDS_EXACT, HAS_NAN = 1, 2
FILL32 = 0xA5A5A5A5
FILL64 = 0xA5A5A5A5A5A5A5A5
KMULTI_MAX = 220
SELECT_MAX_ROUNDS = 16
# in_extra codes of the tool: 0, IN_EXTRA_I8_SINGLE, IN_EXTRA_BF16_SINGLE, IN_EXTRA_MFMA (the tool reports the value)
IN_EXTRA_CODES = (0, 1, 2, 3)
HIP_INVALID_VALUE = 1

BLOCK = np.dtype([("n_out", "<u4"), ("flags", "<u4"), ("pos", "<u4", (KP,)), ("score", "<u8", (KP,)), ("seq", "<u4"),
                  ("pad", "<u4")])
assert BLOCK.itemsize == 784

LIST_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 31, 32, 33, 47, 48, 49, 60, 63, 64, 65, 127, 128, 129, 768, 1024,
               4095, 4096)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def desc_key(s):
    """u64 whose ascending order is the descending order of the score, -0.0 == +0.0 (k_sort_init's desc_key)."""
    b = bits(np.asarray(s, dtype=np.float64) + 0.0)
    asc = np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(1 << 63))
    return ~asc


def f32_to_ordered(f):
    b = int(np.float32(f).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def ordered_to_f32(o):
    b = (o & 0x7FFFFFFF) if o & 0x80000000 else (~o & 0xFFFFFFFF)
    return np.uint32(b).view(np.float32)


def py_bound(metric, t_key, n, R, Q, in_extra):
    """bound_for_key of score_bound.hpp in Python floats (the same IEEE operations in the same order)."""
    u = 2.0 ** -24
    nn, t = float(n), float(np.float32(t_key))
    if metric == COS:
        return float("inf") if not Q > 0.0 else t / Q + 2.0 * (nn + 4.0) * u + in_extra + 1e-12
    if metric == DOT:
        return t + (2.0 * (nn + 2.0) * u + in_extra) * R * Q + 1e-12 * (1.0 + R * Q)
    if metric == EUC and in_extra > 0.0:
        err = 2.0 * in_extra * R * Q + 4.0 * (nn + 4.0) * u * (R * Q + R * R)
        s_lo = Q * Q - t - err
        if not s_lo > 0.0:
            s_lo = 0.0
        return (1.0 / (1.0 + float(np.sqrt(s_lo)) * (1.0 - 1e-12))) * (1.0 + 1e-15)
    ts = -t if t < 0.0 else 0.0
    if metric == EUC:
        d_lo = float(np.sqrt(ts)) * (1.0 - 2.0 * (nn + 2.0) * u) - 4.0 * u * (R + Q)
    else:
        d_lo = ts * (1.0 - 2.0 * (nn + 2.0) * u) - 4.0 * u * float(np.sqrt(nn)) * (R + Q)
    if not d_lo > 0.0:
        d_lo = 0.0
    return (1.0 / (1.0 + d_lo * (1.0 - 1e-12))) * (1.0 + 1e-15)


def seq_norm(v):
    """|v| as the host stages a query: sequential sum of squares, one sqrt."""
    ss = 0.0
    for x in np.asarray(v, dtype=np.float64):
        ss += float(x) * float(x)
    return float(np.sqrt(ss))


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
@dataclass
class Sink:
    ks: int
    q0: int
    row_offset: int
    pos_to_id: np.ndarray


@dataclass
class ListCase:
    """One launch of a list launcher.  The lists' real entries lie list after list in (keys, pos); lens[l] of them belong
    to list l.  FINALIZE: nq * n_lists lists, query-major.  MULTI: n_lists lists in all, n_parts partitions.  BATCH: nq."""
    mode: int
    metric: int
    rows: np.ndarray        # [m, dim] master rows (reuse_master: the tool keeps the previous case's, same array)
    queries: np.ndarray     # [nq, dim]
    lens: np.ndarray
    keys: np.ndarray
    pos: np.ndarray
    n_lists: int
    n_rows: int
    k: int
    R: float
    n_parts: int = 0
    code: int = 0
    seq: int = 0
    sink: Sink = None
    reuse_master: bool = False
    expect_refuse: bool = False
    expect_flags: object = None   # per query, where the construction fixes them (the decision pairs, branch cases)
    name: str = ""
    qn: np.ndarray = None

    def __post_init__(self):
        self.queries = np.ascontiguousarray(self.queries, dtype=np.float64)
        self.lens = np.ascontiguousarray(self.lens, dtype=np.uint32)
        self.keys = np.ascontiguousarray(self.keys, dtype=np.float32)
        self.pos = np.ascontiguousarray(self.pos, dtype=np.uint32)
        if self.qn is None:
            self.qn = np.array([seq_norm(q) for q in self.queries])
        assert int(self.lens.sum()) == len(self.keys) == len(self.pos) and (self.lens <= KP).all()
        assert len(self.pos) == 0 or int(self.pos.max()) < len(self.rows)

    @property
    def nq(self):
        return len(self.queries)

    @property
    def dim(self):
        return self.queries.shape[1]

    def group_lists(self):
        """(first list, lists) of every merge group: a query, or a partition of MULTI (None: the launcher must refuse)."""
        if self.mode == FINALIZE:
            return [(q * self.n_lists, self.n_lists) for q in range(self.nq)]
        if self.mode == BATCH:
            return [(q, 1) for q in range(self.nq)]
        if self.expect_refuse:
            return []
        per = self.n_lists // self.n_parts
        return [(p * per, per) for p in range(self.n_parts)]


@dataclass
class SelectCase:
    scores: np.ndarray
    krs: tuple
    flag_word: int = 0
    name: str = ""
    mode: int = SELECT


@dataclass
class Merged:
    idx: np.ndarray      # indices of the merged entries into the case's (keys, pos), best first
    keys: np.ndarray
    pos: np.ndarray
    lists: np.ndarray    # list of every merged entry, counted within the group
    slots: np.ndarray    # its slot in that list

    @property
    def n_cand(self):
        return len(self.idx)

    @property
    def key64(self):
        return self.keys[KP - 1] if len(self.keys) == KP else np.float32(-np.inf)  # a sentinel's key


def merge_groups(case):
    """The merged candidates of every group: top 64 of the union by (key desc, position asc); sentinels never enter."""
    off = np.concatenate([[0], np.cumsum(case.lens, dtype=np.int64)])
    out = []
    for first, cnt in case.group_lists():
        lo, hi = int(off[first]), int(off[first + cnt])
        k, p = case.keys[lo:hi], case.pos[lo:hi]
        order = np.lexsort((p, -k.astype(np.float64)))[:KP]
        idx = lo + order
        lst = np.searchsorted(off, idx, side="right") - 1
        out.append(Merged(idx, k[order], p[order], lst - first, idx - off[lst]))
    return out


def lists_sorted(case):
    """Every list is sorted by (key desc, position asc) and no position occurs twice in a group."""
    off = np.concatenate([[0], np.cumsum(case.lens, dtype=np.int64)])
    if len(case.keys) > 1:
        k, p = case.keys.astype(np.float64), case.pos.astype(np.int64)
        ok = (k[:-1] > k[1:]) | ((k[:-1] == k[1:]) & (p[:-1] < p[1:]))
        ok[off[1:-1][(off[1:-1] > 0) & (off[1:-1] < len(k))] - 1] = True  # list boundaries
        if not ok.all():
            return False
    for first, cnt in case.group_lists():
        p = case.pos[int(off[first]):int(off[first + cnt])]
        if len(np.unique(p)) != len(p):
            return False
    return True


def rank_scores(scores, pos):
    """Order of the candidates by (score desc with -0.0 == +0.0, position asc)."""
    return np.lexsort((pos, desc_key(scores)))


def flags_single(nan, n_cand, n_rows, k_eff, s_cut, B):
    """rank_check_emit's flag logic."""
    f = (HAS_NAN | NEEDS_EXACT) if nan else 0
    if n_rows <= KP:
        if n_cand < n_rows:
            f |= NEEDS_EXACT     # the list must hold EVERY row
    elif n_cand < KP:
        f |= NEEDS_EXACT
    elif k_eff < 1 or not (s_cut > B):  # no entry is ranked k_eff - 1 when k_eff = 0
        f |= NEEDS_EXACT
    return f


def flags_multi(nan, n_cands, n_rows, k_eff, s_cut, Bs):
    """k_merge_finalize_multi's flag logic; Bs[p] = B(64th key of partition p)."""
    f = (HAS_NAN | NEEDS_EXACT) if nan else 0
    total = int(sum(n_cands))
    full = [p for p, c in enumerate(n_cands) if c == KP]
    excluded = bool(full)
    has_cut = 1 <= k_eff <= total
    if not has_cut or total < k_eff:
        f |= NEEDS_EXACT
    elif excluded:
        B = max([-1.0e300] + [Bs[p] for p in full])
        if not (s_cut > B):
            f |= NEEDS_EXACT
    if total < n_rows and not excluded:
        f |= NEEDS_EXACT
    return f


@dataclass
class Answer:
    nan: bool
    n_cand: int
    k_eff: int
    pos: np.ndarray      # ranked positions, all candidates
    score: np.ndarray    # ranked score bits
    s_cut: float
    flags: int = -1


def model_answers(case, score_fn, merged=None):
    """Per query (MULTI: one for the search) the ranked candidates; flags are filled in by set_flags once B is known."""
    merged = merged if merged is not None else merge_groups(case)
    k_eff = min(case.k, case.n_rows)
    if case.mode == MULTI:
        if case.expect_refuse:
            return []
        groups = [merged]
    else:
        groups = [[m] for m in merged]
    out = []
    for qi, g in enumerate(groups):
        pos = np.concatenate([m.pos for m in g]).astype(np.int64)
        sc = np.array([score_fn(case.metric, case.rows[p], case.queries[qi]) for p in pos], dtype=np.float64)
        nan = bool(np.isnan(sc).any())
        if nan:
            out.append(Answer(True, len(pos), k_eff, pos, bits(sc), float("nan")))
            continue
        order = rank_scores(sc, pos)
        s_cut = float(sc[order[k_eff - 1]]) if 1 <= k_eff <= len(pos) else 0.0
        out.append(Answer(False, len(pos), k_eff, pos[order], bits(sc[order]), s_cut))
    return out


def set_flags(case, merged, answers, B):
    """B[i]: the bound at merged[i].key64, R, the group's query norm and the case's in_extra."""
    if case.mode == MULTI:
        for a in answers:
            a.flags = flags_multi(a.nan, [m.n_cand for m in merged], case.n_rows, a.k_eff, a.s_cut, B)
    else:
        for a, m, b in zip(answers, merged, B):
            a.flags = flags_single(a.nan, m.n_cand, case.n_rows, a.k_eff, a.s_cut, b)


def expected_blocks(case, answers, n_blocks):
    blk = np.frombuffer(bytes([0xA5]) * (BLOCK.itemsize * n_blocks), dtype=BLOCK).copy()
    for qi, a in enumerate(answers):
        base = 0 if case.mode == MULTI else qi
        blk["n_out"][base] = a.k_eff
        blk["flags"][base] = a.flags
        if case.seq:
            blk["seq"][base] = case.seq
        if a.nan:
            continue
        for r in range(min(a.k_eff, a.n_cand)):
            b = base + (r // KP if case.mode == MULTI else 0)
            blk["pos"][b][r % KP] = a.pos[r]
            blk["score"][b][r % KP] = a.score[r]
    return blk


def expected_sink(case, answers):
    s = case.sink
    nqs = s.q0 + case.nq
    cnt = np.full(nqs, FILL64, dtype=np.uint64)
    planes = [np.full(nqs * s.ks, FILL64, dtype=np.uint64) for _ in range(3)]
    for qi, a in enumerate(answers):
        offered = min(a.k_eff, s.ks) if a.flags == 0 else 0
        cnt[s.q0 + qi] = offered
        for r in range(min(offered, a.n_cand)):
            e = (s.q0 + qi) * s.ks + r
            planes[0][e] = a.score[r]
            planes[1][e] = s.row_offset + int(a.pos[r])
            planes[2][e] = s.pos_to_id[a.pos[r]]
    return cnt, planes


def select_model(scores, krs, flag_word):
    """Expected result blocks of a chain of launch_exact_select rounds."""
    n = len(scores)
    order = np.lexsort((np.arange(n), desc_key(scores)))
    blk = np.frombuffer(bytes([0xA5]) * (BLOCK.itemsize * len(krs)), dtype=BLOCK).copy()
    ninf = bits(np.array([-np.inf]))[0]
    for r, kr in enumerate(krs):
        k_eff = min(kr, n)
        blk["n_out"][r] = k_eff
        blk["flags"][r] = HAS_NAN if flag_word else 0
        for j in range(KP if kr == KP else k_eff):  # a full round carries all 64 slots for the next one
            rank = KP * r + j
            blk["pos"][r][j] = order[rank] if rank < n else POS_SENTINEL
            blk["score"][r][j] = bits(scores[order[rank]:order[rank] + 1])[0] if rank < n else ninf
    return blk


# ---------------------------------------------------------------------------------------------
# case files
# ---------------------------------------------------------------------------------------------
def write_cases(path, cases, bkeys=None):
    """bkeys[i]: (keys f32, query index u32) the tool evaluates the bound at, for list case i."""
    with open(path, "wb") as f:
        f.write(struct.pack("<2I", MAGIC, len(cases)))
        for i, c in enumerate(cases):
            if c.mode == SELECT:
                h = [SELECT, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, c.flag_word, len(c.krs), 0, 0, 0, 0, 0]
                f.write(struct.pack("<20I", *h))
                f.write(struct.pack("<3Qd", 0, len(c.scores), 0, 0.0))
                f.write(np.ascontiguousarray(c.scores, dtype="<f8").tobytes())
                f.write(np.asarray(c.krs, dtype="<u4").tobytes())
                continue
            bk, bq = bkeys[i] if bkeys else (np.zeros(0, np.float32), np.zeros(0, np.uint32))
            s = c.sink
            h = [c.mode, c.metric, c.nq, c.n_lists, c.n_parts, c.dim, 0 if c.reuse_master else len(c.rows), c.k, c.seq,
                 1 if s else 0, s.ks if s else 0, s.q0 if s else 0, c.code, 0, 0, 1 if c.expect_refuse else 0, len(bk),
                 len(c.keys), 0, 0]
            f.write(struct.pack("<20I", *h))
            f.write(struct.pack("<3Qd", c.n_rows, 0, s.row_offset if s else 0, c.R))
            if not c.reuse_master:
                f.write(np.ascontiguousarray(c.rows, dtype="<f8").tobytes())
            f.write(c.queries.tobytes())
            f.write(np.ascontiguousarray(c.qn, dtype="<f8").tobytes())
            f.write(c.lens.tobytes())
            f.write(c.keys.tobytes())
            f.write(c.pos.tobytes())
            f.write(np.ascontiguousarray(bk, dtype="<f4").tobytes())
            f.write(np.ascontiguousarray(bq, dtype="<u4").tobytes())
            if s:
                f.write(np.ascontiguousarray(s.pos_to_id, dtype="<u8").tobytes())


def parse_output(buf, cases):
    magic, n = struct.unpack_from("<2I", buf, 0)
    assert magic == MAGIC and n == len(cases)
    off = 8
    outs = []

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a

    for c in cases:
        magic, mode, rc, n_blocks, n_b, sink_q = struct.unpack_from("<6I", buf, off)
        off += 24
        assert magic == MAGIC and mode == c.mode
        o = dict(rc=rc, in_extra=float(take("<f8", 1)[0]), blocks=take(BLOCK, n_blocks))
        if mode != SELECT:
            if c.sink:
                assert sink_q == c.sink.q0 + c.nq
                o["cnt"] = take("<u8", sink_q)
                o["planes"] = [take("<u8", sink_q * c.sink.ks) for _ in range(3)]
            if mode == BATCH:
                o["scratch"] = take("<u8", c.nq * KP).reshape(c.nq, KP)
            o["B_dev"] = take("<f8", n_b)
            o["B_host"] = take("<f8", n_b)
        outs.append(o)
    assert off == len(buf)
    return outs


def bound_requests(case, merged):
    """The keys the tool evaluates the bound at: every group's key64 with its query's norm."""
    bk = np.array([m.key64 for m in merged], dtype=np.float32)
    bq = np.zeros(len(merged), dtype=np.uint32) if case.mode == MULTI else np.arange(len(merged), dtype=np.uint32)
    return bk, bq


# ---------------------------------------------------------------------------------------------
# judging
# ---------------------------------------------------------------------------------------------
def _same(got, want, ctx, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(np.asarray(got).ravel() != np.asarray(want).ravel())[0]
        raise AssertionError((ctx, what, "first differences at", bad[:6].tolist(),
                              np.asarray(got).ravel()[bad[:6]].tolist(), np.asarray(want).ravel()[bad[:6]].tolist()))


def judge_list_case(case, merged, answers, o):
    """Compare everything the tool dumped with the model; returns the number of queries judged."""
    ctx = (case.name, MODE_NAME[case.mode], METRIC_NAME[case.metric])
    n_blocks = len(o["blocks"])
    fill = np.frombuffer(bytes([0xA5]) * (BLOCK.itemsize * n_blocks), dtype=BLOCK)
    if case.expect_refuse:
        assert o["rc"] == HIP_INVALID_VALUE, (ctx, "launcher status", o["rc"])
        assert o["blocks"].tobytes() == fill.tobytes(), (ctx, "a refused launch wrote a result block")
        return 0
    assert o["rc"] == 0, (ctx, "launcher status", o["rc"])
    # the device's and the host's bound agree bit for bit at every key64 used
    _same(bits(o["B_dev"]), bits(o["B_host"]), ctx, "bound_for_key: device vs host bits")
    set_flags(case, merged, answers, [float(b) for b in o["B_dev"]])
    want = expected_blocks(case, answers, n_blocks)
    got = o["blocks"]
    judged = 0
    for qi, a in enumerate(answers):
        base = 0 if case.mode == MULTI else qi
        c2 = ctx + (f"query {qi}",)
        assert int(got["n_out"][base]) == a.k_eff, (c2, "n_out", int(got["n_out"][base]), a.k_eff)
        assert int(got["flags"][base]) == a.flags, (c2, "flags", int(got["flags"][base]), a.flags, "n_cand", a.n_cand)
        if case.expect_flags is not None:
            assert a.flags == case.expect_flags[qi], (c2, "the construction fixes the flags", a.flags, case.expect_flags[qi])
        if a.nan:
            assert a.flags == (HAS_NAN | NEEDS_EXACT)
        else:
            span = range(n_blocks) if case.mode == MULTI else [base]
            for b in span:
                _same(got["pos"][b], want["pos"][b], c2, f"positions of block {b}")
                _same(got["score"][b], want["score"][b], c2, f"score bits of block {b}")
        for b in (range(n_blocks) if case.mode == MULTI else [base]):
            assert int(got["seq"][b]) == int(want["seq"][b]) and int(got["pad"][b]) == FILL32, (c2, "seq / pad", b)
            if case.mode == MULTI and b > 0:
                assert int(got["n_out"][b]) == FILL32 and int(got["flags"][b]) == FILL32, (c2, "header of a later block")
        judged += 1
    if case.sink:
        cnt, planes = expected_sink(case, answers)
        _same(o["cnt"], cnt, ctx, "sink cnt")
        for name, g, w in zip(("score bits", "gpos", "ids"), o["planes"], planes):
            _same(g, w, ctx, "sink " + name)
    if case.mode == BATCH:  # the rescoring kernel writes all 64 slots of every query: scores, then zeros
        for qi, (a, m) in enumerate(zip(answers, merged)):
            sc = np.zeros(KP, dtype=np.uint64)
            if a.nan:
                continue
            # scratch is in LIST order (the merged order of one list = the list itself)
            inv = {int(p): s for p, s in zip(a.pos, a.score)}
            sc[:m.n_cand] = [inv[int(p)] for p in m.pos]
            _same(o["scratch"][qi], sc, ctx + (f"query {qi}",), "score scratch")
    return judged


def judge_select_case(case, o):
    ctx = (case.name, "select")
    assert o["rc"] == 0, (ctx, "launcher status", o["rc"])
    want = select_model(case.scores, case.krs, case.flag_word)
    got = o["blocks"]
    for r in range(len(case.krs)):
        for fld in ("n_out", "flags", "pos", "score", "seq", "pad"):
            _same(got[fld][r], want[fld][r], ctx + (f"round {r}",), fld)
    return len(case.krs)


# ---------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------
def mixed_rows(rng, m, dim):
    """Half small integers (score ties, decided by position), half Gaussian."""
    rows = rng.standard_normal((m, dim))
    lat = rng.integers(-2, 3, size=(m // 2, dim)).astype(np.float64)
    lat[~lat.any(axis=1), 0] = 1.0
    rows[: m // 2] = lat
    return rows[rng.permutation(m)]


def cancel_rows(rng, m, dim):
    """Neighbouring columns nearly cancel and the magnitudes span 2^-20 .. 2^20: a sum taken in another order, or a fused
    multiply-add, changes the bits of the score."""
    a = rng.standard_normal((m, dim)) * 2.0 ** rng.integers(-20, 21, size=(m, dim))
    a[:, 1::2] = -a[:, 0:dim - (dim % 2):2] * (1.0 + 2.0 ** -30 * rng.standard_normal((m, dim // 2)))
    return a


def cancel_queries(rng, nq, dim):
    q = rng.standard_normal((nq, dim))
    q[:, 1::2] = q[:, 0:dim - (dim % 2):2] * (1.0 + 2.0 ** -28 * rng.standard_normal((nq, dim // 2)))
    return q


def required_lists(n_lists):
    """Lists that must hold a winner somewhere in a list-count case: the first and last list of every group of 4 a wave
    folds (which includes the first and last list of every block of 64), list 0 and the last list."""
    l = np.arange(n_lists)
    return l[(l % 4 == 0) | (l % 4 == 3) | (l == n_lists - 1)]


def variants_for(n_lists):
    """The queries of a list-count case: (kind, lists that get planted entries)."""
    req = required_lists(n_lists)
    v = [("spread", None), ("last", None)]
    v += [("sweep", req[i:i + 56]) for i in range(0, len(req), 56)]
    v += [("short", None), ("empty", None), ("few", None)]
    return v


def build_query(rng, n_lists, kind, planted, dense):
    """(list index, key) of every entry of one query's lists.  Keys are small integers: filler entries 0..3, planted
    entries 4..6, so ties are everywhere and the cut of every fold is decided by position."""
    if kind == "empty":
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    if kind == "few":  # fewer than 64 real entries in all
        cnt = min(n_lists, 40) if n_lists > 1 else 1
        li = np.sort(rng.choice(n_lists, size=cnt, replace=False))
        li = np.repeat(li, 40 if n_lists == 1 else 1)
        return li.astype(np.int64), rng.integers(0, 7, size=len(li)).astype(np.float32)
    high = np.zeros(n_lists, dtype=np.int64)
    if kind == "short":
        fill = rng.integers(0, 4, size=n_lists)
        fill[rng.integers(0, n_lists)] = 3
    else:
        full = rng.random(n_lists) < (0.5 if dense else 0.03)
        fill = np.where(full, KP, rng.integers(0, KP if dense else 4, size=n_lists))
    if kind == "spread":  # 64 planted entries over min(64, n_lists) lists, list 0 and the last among them
        t = min(KP, n_lists)
        mid = rng.choice(np.arange(1, n_lists - 1), size=t - 2, replace=False) if t > 2 else np.zeros(0, np.int64)
        lists = np.unique(np.concatenate([[0, n_lists - 1], mid]).astype(np.int64))
        high[lists] = KP // len(lists)
        high[lists[: KP - int(high.sum())]] += 1
    elif kind == "last":  # all 64 winners in the last list
        high[n_lists - 1] = KP
    elif kind == "sweep":
        high[planted] = 1
        high[planted[:4]] = 2  # a winner in slot 1 of its list
    fill = np.minimum(fill, KP - high)
    li = np.concatenate([np.repeat(np.arange(n_lists), fill), np.repeat(np.arange(n_lists), high)])
    key = np.concatenate([rng.integers(0, 4, size=int(fill.sum())), rng.integers(4, 7, size=int(high.sum()))])
    return li.astype(np.int64), key.astype(np.float32)


def assemble(rng, per_query, n_lists, m_rows):
    """Positions (a random permutation per query: unique within the query), every list sorted by (key desc, pos asc)."""
    lens, keys, pos = [], [], []
    for li, key in per_query:
        p = rng.permutation(m_rows)[: len(li)].astype(np.uint32)
        order = np.lexsort((p, -key.astype(np.float64), li))
        lens.append(np.bincount(li, minlength=n_lists).astype(np.uint32))
        keys.append(key[order])
        pos.append(p[order])
    return np.concatenate(lens), np.concatenate(keys), np.concatenate(pos)


def finalize_shape_case(seed, n_lists, nq, metric, k=KP, dim=4, sink=None, name=""):
    """nq queries of n_lists lists each, the variants of variants_for(n_lists) in turn."""
    rng = np.random.default_rng([seed, n_lists, nq])
    var = variants_for(n_lists)
    dense = nq * n_lists <= 129
    per_query = [build_query(rng, n_lists, *var[q % len(var)], dense) for q in range(nq)]
    m_rows = max(KP + 1, max(len(li) for li, _ in per_query))
    lens, keys, pos = assemble(rng, per_query, n_lists, m_rows)
    rows = mixed_rows(rng, m_rows, dim)
    queries = mixed_rows(rng, nq + 2, dim)[:nq]
    R = float(np.linalg.norm(rows, axis=1).max())
    return ListCase(FINALIZE, metric, rows, queries, lens, keys, pos, n_lists, m_rows, k, R, sink=sink,
                    name=name or f"L{n_lists}-q{nq}")


def list_count_cases(n_lists):
    """The FINALIZE list-count cases of one n_lists: every variant as its own nq = 1 launch, cosine always and one of the
    other metrics in turn (all of them for the counts up to 129, where the file stays small)."""
    n_var = len(variants_for(n_lists))
    idx = LIST_COUNTS.index(n_lists)
    metrics = (COS,) if n_lists > 129 else (COS, ALL4[1 + idx % 3])
    cases = []
    for metric in metrics:
        big = finalize_shape_case(7, n_lists, n_var, metric)
        off = np.concatenate([[0], np.cumsum(big.lens, dtype=np.int64)])
        for q in range(n_var):
            lo, hi = int(off[q * n_lists]), int(off[(q + 1) * n_lists])
            cases.append(ListCase(FINALIZE, metric, big.rows, big.queries[q:q + 1], big.lens[q * n_lists:(q + 1) * n_lists],
                                  big.keys[lo:hi], big.pos[lo:hi], n_lists, big.n_rows, KP, big.R, reuse_master=bool(cases),
                                  seq=(q + 1) if q % 3 == 0 else 0,
                                  name=f"L{n_lists}-{METRIC_NAME[metric]}-{variants_for(n_lists)[q][0]}{q}"))
            if cases[-1].reuse_master:
                cases[-1].rows = cases[0].rows
    return cases


def check_list_count_coverage(n_lists, cases, merged_per_case):
    """The planted winners cover what the issue asks of a list-count case (asserted on the host, before the device is
    judged).  A winner is an entry of a query's merged top 64; with k = 64 every one of them is checked."""
    by_metric = {}
    for c, m in zip(cases, merged_per_case):
        by_metric.setdefault(c.metric, []).append(m[0])
    for metric, ms in by_metric.items():
        ctx = (n_lists, METRIC_NAME[metric])
        seen = np.zeros(n_lists, dtype=bool)
        slots = set()
        all_last = spread = False
        for m in ms:
            seen[m.lists] = True
            slots.update(int(s) for s in m.slots)
            all_last |= m.n_cand == KP and (m.lists == n_lists - 1).all()
            spread |= len(np.unique(m.lists)) == min(KP, n_lists)
        req = required_lists(n_lists)
        assert seen[0] and seen[n_lists - 1], (ctx, "list 0 / the last list hold no winner")
        assert seen[req].all(), (ctx, "group-of-4 / block-of-64 edge lists without a winner", req[~seen[req]][:8])
        l = np.arange(n_lists)
        assert seen[(l % 64 == 0) | (l % 64 == 63)].all(), ctx
        assert {0, 1, 62, 63} <= slots, (ctx, "winner slots", sorted(slots)[:8])
        assert all_last, (ctx, "no query with all 64 winners in the last list")
        assert spread, (ctx, "no query with winners in min(64, n_lists) lists")
        assert any(m.n_cand == 0 for m in ms) and any(0 < m.n_cand < KP for m in ms), (ctx, "empty / short queries")


def full_list(rng, m_rows, n_cand, keys=None):
    """One sorted list of n_cand entries at distinct random positions."""
    pos = rng.choice(m_rows, size=n_cand, replace=False).astype(np.uint32)
    if keys is None:
        keys = rng.integers(0, 5, size=n_cand).astype(np.float32)
    order = np.lexsort((pos, -np.asarray(keys, dtype=np.float64)))
    return np.asarray(keys, dtype=np.float32)[order], pos[order]


def keys_above(tau, which):
    """64 descending keys: 63 above both tau and its successor, the 64th = tau (which = 0) or the next f32 above (1)."""
    o = f32_to_ordered(tau)
    return np.array([ordered_to_f32(o + 1 + (KP - 1 - i)) for i in range(KP - 1)] + [ordered_to_f32(o + which)],
                    dtype=np.float32)


def split_lists(keys, pos, n_lists):
    """A sorted run of entries dealt round-robin into n_lists sorted lists."""
    parts = [(keys[i::n_lists], pos[i::n_lists]) for i in range(n_lists)]
    return (np.array([len(k) for k, _ in parts], dtype=np.uint32), np.concatenate([k for k, _ in parts]),
            np.concatenate([p for _, p in parts]))


# ---- the decision: key64 on either side of the bound ---------------------------------------------------------------
DECISION_KS = (1, 10, 60, 64)


@dataclass
class Setup:
    """A decision pair before its keys exist: the tool's tau(s_cut) places key64."""
    mode: int
    metric: int
    code: int
    k: int
    rows: np.ndarray
    query: np.ndarray
    pos: list            # per partition (one for FINALIZE / BATCH): the 64 candidates' positions
    s_cut: float
    R: float
    Q: float
    n_parts: int = 0
    top: int = 0         # MULTI: the partition that carries the largest bound

    def tau_request(self):
        ld = (self.rows.shape[1] + 3) & ~3
        return (self.metric, ld, self.R, self.Q, self.s_cut, self.code)


def decision_setups(mode, metric, score_fn, dim=8, m_rows=100):
    rng = np.random.default_rng([11, mode, metric])
    out = []
    for code in IN_EXTRA_CODES:
        for k in DECISION_KS:
            rows = rng.standard_normal((m_rows, dim))
            q = rng.standard_normal(dim)
            pos = rng.choice(m_rows, size=KP, replace=False)
            sc = np.array([score_fn(metric, rows[p], q) for p in pos])
            s_cut = float(sc[rank_scores(sc, pos)[k - 1]])
            out.append(Setup(mode, metric, code, k, rows, q, [pos], s_cut, float(np.linalg.norm(rows, axis=1).max()), seq_norm(q)))
    return out


def multi_decision_setups(score_fn, dim=8, m_rows=400, k=100):
    rng = np.random.default_rng([12])
    out = []
    for metric in ALL4:
        for n_parts in (2, 3, 4):
            for top in sorted({0, n_parts // 2, n_parts - 1}):
                rows = rng.standard_normal((m_rows, dim))
                q = rng.standard_normal(dim)
                pos = rng.choice(m_rows, size=KP * n_parts, replace=False)
                sc = np.array([score_fn(metric, rows[p], q) for p in pos])
                s_cut = float(sc[rank_scores(sc, pos)[k - 1]])
                out.append(Setup(MULTI, metric, 0, k, rows, q, [pos[p * KP:(p + 1) * KP] for p in range(n_parts)], s_cut,
                                 float(np.linalg.norm(rows, axis=1).max()), seq_norm(q), n_parts, top))
    return out


def decision_pair(st, tau):
    """The two cases of a setup: key64 = tau certifies (flags 0), the next f32 above does not (NEEDS_EXACT)."""
    pair = []
    for which in (0, 1):
        lens, keys, pos = [], [], []
        for p, ppos in enumerate(st.pos):
            if st.mode == MULTI and p != st.top:  # a smaller 64th key: a bound that is not above the top partition's
                kk = keys_above(tau, 0)
                kk[KP - 1] = ordered_to_f32(f32_to_ordered(tau) - 1000)
            else:
                kk = keys_above(tau, which)
            order = np.argsort(ppos, kind="stable")  # distinct keys: any assignment is a sorted list
            n_l = 1 if st.mode != FINALIZE else 3
            l, k2, p2 = split_lists(kk, np.asarray(ppos)[order].astype(np.uint32), n_l)
            lens.append(l)
            keys.append(k2)
            pos.append(p2)
        n_lists = {FINALIZE: 3, BATCH: 1, MULTI: len(st.pos)}[st.mode]
        pair.append(ListCase(st.mode, st.metric, st.rows, st.query[None, :], np.concatenate(lens), np.concatenate(keys),
                             np.concatenate(pos), n_lists, len(st.rows), st.k, st.R, n_parts=st.n_parts, code=st.code,
                             expect_flags=[NEEDS_EXACT if which else 0],
                             name=f"decision-{METRIC_NAME[st.metric]}-e{st.code}-k{st.k}-p{st.n_parts}t{st.top}-{'above' if which else 'tau'}"))
    return pair


# ---- branches of rank_check_emit -----------------------------------------------------------------------------------
def branch_cases(mode):
    """k = 0: the launchers accept it (n_out = 0, nothing else written; a full list with rows outside it is not
    certified, since no entry is ranked k_eff - 1).  The library never gets there: every search entry point of FlatIndex
    returns an empty answer for k == 0 before it stages a query."""
    rng = np.random.default_rng([13, mode])
    dim, m = 8, 120
    rows = rng.standard_normal((m, dim))
    rows[5] = 0.0                       # a zero row: cosine scores it 0.0
    rows[7, 2] = np.nan                 # a NaN row
    rows[20:52] = rows[60:92]           # equal rows at different positions
    good = np.array([p for p in range(m) if p != 7])
    R = float(np.linalg.norm(np.nan_to_num(rows), axis=1).max())
    n_l = 1 if mode == BATCH else 3
    cases = []

    def add(name, metric, cand, n_rows, k, q=None, key_lo=None, expect=None):
        q = rng.standard_normal(dim) if q is None else q
        keys = np.arange(len(cand), 0, -1).astype(np.float32)
        if key_lo is not None and len(keys):
            keys[-1] = key_lo
        order = np.arange(len(cand))
        lens, k2, p2 = split_lists(keys, np.asarray(cand, dtype=np.uint32)[order], n_l)
        cases.append(ListCase(mode, metric, rows, q[None, :], lens, k2, p2, n_l, n_rows, k, R, reuse_master=bool(cases),
                              expect_flags=None if expect is None else [expect], name="branch-" + name))

    for metric in ALL4:
        c40 = rng.choice(good, size=40, replace=False)
        add("rows<=64-all", metric, c40, 40, 10, expect=0)
        add("rows<=64-missing", metric, c40[:30], 40, 10, expect=NEEDS_EXACT)
        add("rows>64-short", metric, rng.choice(good, size=50, replace=False), m, 10, expect=NEEDS_EXACT)
        add("k>rows", metric, c40, 40, KP, expect=0)
        add("k0-small", metric, c40, 40, 0, expect=0)
        add("k0-full", metric, rng.choice(good, size=KP, replace=False), m, 0, expect=NEEDS_EXACT)
        nanc = rng.choice(good, size=KP, replace=False)
        nanc[17] = 7
        add("nan", metric, nanc, m, 10, expect=HAS_NAN | NEEDS_EXACT)
    full = rng.choice(good[good != 5], size=KP, replace=False)
    full[3] = 5
    # cosine: a key far below every score certifies (B ~ key / Q); a zero query makes B = +inf
    add("zero-row", COS, full, m, 10, key_lo=-1.0e6, expect=0)
    add("zero-query", COS, full, m, 10, q=np.zeros(dim), key_lo=-1.0e6, expect=NEEDS_EXACT)
    # the candidates are 32 pairs of equal rows, so every odd k puts the cut inside a pair: the lower position ranks first
    # and the tie in score at the cut still certifies, being above B
    cand = np.concatenate([np.arange(20, 52), np.arange(60, 92)])
    for k in (1, 3, 9, 31, 63):
        add(f"tie-cut-k{k}", COS, cand, m, k, key_lo=-1.0e6, expect=0)
    return cases


# ---- rescoring widths ----------------------------------------------------------------------------------------------
FINALIZE_DIMS = (1, 3, 47, 48, 49, 383, 384, 385, 767, 768, 769, 1000)
BATCH_DIMS = (1, 47, 48, 49, 100, 191, 192, 193, 384, 700, 768)
BATCH_NCAND = (0, 1, 15, 16, 17, 48, 63, 64)
FAMILIES = (("gauss", lambda r, m, d: r.standard_normal((m, d)), lambda r, n, d: r.standard_normal((n, d))),
            ("cancel", cancel_rows, cancel_queries))


def width_cases(mode, dim, m_rows=66):
    rng = np.random.default_rng([14, mode, dim])
    cases = []
    combo = 0
    for fam, mk_rows, mk_q in FAMILIES:
        rows = mk_rows(rng, m_rows, dim)
        R = float(np.linalg.norm(rows, axis=1).max())
        first = True
        for metric in ALL4:
            shapes = [(1, (nc,)) for nc in (1, 63, 64)] if mode == FINALIZE else \
                [(nq, tuple(BATCH_NCAND[(i + combo) % 8] for i in range(nq))) for nq in (1, 4, 5, 33)]
            for nq, ncs in shapes:
                ls = [full_list(rng, m_rows, nc) for nc in ncs]
                cases.append(ListCase(mode, metric, rows, mk_q(rng, nq, dim), [len(k) for k, _ in ls],
                                      np.concatenate([k for k, _ in ls]), np.concatenate([p for _, p in ls]), 1, m_rows, 10, R,
                                      reuse_master=not first, name=f"width-d{dim}-{fam}-q{nq}-c{ncs[0]}"))
                first = False
            combo += 1
    return cases


# ---- batch shapes (FINALIZE, nq > 1) -------------------------------------------------------------------------------
BATCH_SHAPES = ((8, 64), (8, 65), (8, 2048), (512, 1), (512, 32), (512, 64), (3, 1))


def batch_shape_cases(nq, n_lists):
    """One shape without a sink and with ks below, equal to and above k, q0 != 0."""
    k = 10
    base = finalize_shape_case(9, n_lists, nq, ALL4[(nq + n_lists) % 4], k=k)
    ids = np.random.default_rng([15, nq, n_lists]).integers(1, 1 << 62, size=len(base.rows)).astype(np.uint64)
    cases = [base]
    for ks in (k - 3, k, k + 5):
        c = ListCase(FINALIZE, base.metric, base.rows, base.queries, base.lens, base.keys, base.pos, n_lists, base.n_rows, k,
                     base.R, sink=Sink(ks, 3, 1 << 33, ids), reuse_master=True, name=f"{base.name}-ks{ks}")
        cases.append(c)
    return cases


# ---- MULTI ---------------------------------------------------------------------------------------------------------
MULTI_PARTS = (2, 3, 4)
MULTI_L = (1, 4, 5, 64, 65, 1024)
MULTI_KS = (61, 64, 128, 129, 192, 220)


def multi_cases(n_parts, L):
    rng = np.random.default_rng([16, n_parts, L])
    combo = MULTI_PARTS.index(n_parts) * len(MULTI_L) + MULTI_L.index(L)
    dim, m = 4, 2000
    rows = mixed_rows(rng, m, dim)
    nan_rows = rows.copy()
    nan_rows[::50, 1] = np.nan
    R = float(np.linalg.norm(rows, axis=1).max())
    cases = []

    def add(name, counts, k, n_rows=None, rws=rows):
        # counts[p] entries of partition p over its L lists (each list at most 64), lattice keys, positions unique in all
        li, total = [], 0
        for p, c in enumerate(counts):
            c = min(c, L * KP)
            slots = rng.permutation(L * KP)[:c] // KP  # a list never gets more than 64
            li.append(p * L + slots)
            total += c
        li = np.concatenate(li).astype(np.int64)
        key = rng.integers(0, 10, size=total).astype(np.float32)
        lens, keys, pos = assemble(rng, [(li, key)], n_parts * L, m)
        if rws is nan_rows:  # make sure a NaN row is a candidate: the best key of partition 0
            j = int(np.argmax(lens > 0))
            j = int(np.concatenate([[0], np.cumsum(lens)])[j])
            taken = set(pos.tolist())
            pos[j] = next(p for p in range(0, m, 50) if p not in taken or p == pos[j])
            keys[j] = 100.0
        cases.append(ListCase(MULTI, ALL4[(combo + len(cases)) % 4], rws, rng.standard_normal((1, dim)), lens, keys, pos,
                              n_parts * L, total if n_rows == "total" else m, k, R, n_parts=n_parts,
                              reuse_master=bool(cases) and rws is cases[-1].rows, name=f"multi-p{n_parts}-L{L}-{name}"))

    ks = [MULTI_KS[(combo + i) % 6] for i in range(6)]
    fullc = [KP + int(rng.integers(0, 100)) for _ in range(n_parts)]
    add("full", fullc, ks[0])
    add("full-b", [KP] * n_parts, ks[1])
    add("mixed", [20] + fullc[1:], ks[2])
    add("short-uncovered", [30 + 5 * p for p in range(n_parts)], ks[3])
    add("short-covering", [30 + 5 * p for p in range(n_parts)], ks[4], n_rows="total")
    add("below-k", [10] * n_parts, 220)
    add("nan", fullc, ks[5], rws=nan_rows)
    return cases


def multi_refusal_cases():
    rng = np.random.default_rng([17])
    rows = mixed_rows(rng, 700, 4)
    out = []
    for n_lists, n_parts in ((7, 2), (4, 1), (10, 5), (4, 0)):
        ls = [full_list(rng, 700, KP) for _ in range(n_lists)]
        out.append(ListCase(MULTI, COS, rows, rng.standard_normal((1, 4)), [KP] * n_lists, np.concatenate([k for k, _ in ls]),
                            np.concatenate([p for _, p in ls]), n_lists, 700, 100, 3.0, n_parts=n_parts, expect_refuse=True,
                            reuse_master=bool(out), name=f"multi-refuse-{n_lists}-{n_parts}"))
    return out


# ---- SELECT --------------------------------------------------------------------------------------------------------
SELECT_N = (1, 63, 64, 65, 255, 256, 257, 1000, 16384, 16385, 262144, 300000)
SELECT_FAMILIES = ("distinct", "few", "runs", "zeros", "inf", "subnormal")
SELECT_CHAINS = (1, 2, 3, 8, 16)
SELECT_LAST = (1, 36, 64)


def select_scores(rng, fam, n):
    if fam == "distinct":
        return (rng.permutation(n) - n / 3.0) * 0.37
    if fam == "few":
        return rng.integers(0, 3, size=n).astype(np.float64)
    if fam == "runs":  # in rank order, runs of 64 equal scores centred on every multiple of 64
        return (-((np.arange(n) + 32) // 64).astype(np.float64))[rng.permutation(n)]
    if fam == "zeros":
        return rng.choice([0.0, -0.0, 1.0, -1.0], size=n)
    if fam == "inf":
        return rng.choice([np.inf, -np.inf, 0.5, -0.5, 2.0], size=n)
    return rng.integers(-5, 6, size=n) * 5e-324


def select_cases(n):
    rng = np.random.default_rng([18, n])
    ni = SELECT_N.index(n)
    cases = []
    for fi, fam in enumerate(SELECT_FAMILIES):
        idx = fi + 6 * ni
        rounds = SELECT_MAX_ROUNDS if fam == "runs" else SELECT_CHAINS[idx % 5]
        last = SELECT_LAST[(idx // 5) % 3]
        cases.append(SelectCase(select_scores(rng, fam, n), (KP,) * (rounds - 1) + (last,), 1 if idx % 4 == 3 else 0,
                                name=f"select-n{n}-{fam}-r{rounds}-k{last}"))
    return cases


# ---- a score exactly ON the bound ----------------------------------------------------------------------------------
EQ_DIM, EQ_R = 8, 16.0


def equality_probe():
    """One tiny case per in_extra code that makes the tool evaluate B(key 1.0) for the equality cases' dim, R and query."""
    q = np.zeros((1, EQ_DIM))
    q[0, 0] = 1.0
    rows = np.zeros((KP + 1, EQ_DIM))
    cases = [ListCase(BATCH, DOT, rows, q, [1], [1.0], [0], 1, KP + 1, 1, EQ_R, code=code, name=f"probe-e{code}")
             for code in IN_EXTRA_CODES]
    return cases, [(np.array([1.0], np.float32), np.zeros(1, np.uint32))] * len(cases)


def equality_cases(mode, B_of):
    """The strictness of `s_cut > B`: under the dot product with the query e0 a row (v, 0, ..) scores exactly v, and R is a
    parameter of the launch, so the row ranked k_eff - 1 can be given the score B(key64) itself -- not certified -- or the
    next f64 above it -- certified.  B_of[code]: the device's B(1.0) from equality_probe (MULTI always checks with code 0)."""
    rng = np.random.default_rng([19, mode])
    dim, m, R = EQ_DIM, 300, EQ_R
    q = np.zeros(dim)
    q[0] = 1.0
    n_parts = 2 if mode == MULTI else 0
    n_cand = KP * max(n_parts, 1)
    cases = []
    for code in (IN_EXTRA_CODES if mode != MULTI else (0,)):
        for k in ((1, 10, 64) if mode != MULTI else (61, 100, 128)):
            B = B_of[code]
            for which in (0, 1):
                s_cut = B if which == 0 else float(np.nextafter(B, np.inf))
                v = np.concatenate([s_cut + 1.0 + rng.random(k - 1), [s_cut], s_cut - 1.0 - rng.random(n_cand - k)])
                rows = np.zeros((m, dim))
                pos = rng.choice(m, size=n_cand, replace=False)
                rows[pos, 0] = v[rng.permutation(n_cand)]
                lens, keys, ps = [], [], []
                for p in range(max(n_parts, 1)):
                    kk = 1.0 + np.arange(KP - 1, -1, -1, dtype=np.float32)  # 64, 63, .., 1: key64 = 1.0
                    l, k2, p2 = split_lists(kk, pos[p * KP:(p + 1) * KP].astype(np.uint32), 3 if mode == FINALIZE else 1)
                    lens.append(l), keys.append(k2), ps.append(p2)
                n_lists = {FINALIZE: 3, BATCH: 1, MULTI: n_parts}[mode]
                cases.append(ListCase(mode, DOT, rows, q[None, :], np.concatenate(lens), np.concatenate(keys), np.concatenate(ps),
                                      n_lists, m, k, R, n_parts=n_parts, code=code, expect_flags=[0 if which else NEEDS_EXACT],
                                      name=f"equal-e{code}-k{k}-{'above' if which else 'on'}"))
                cases[-1].s_cut_planted = s_cut
    return cases

"""Audit of the lists the three masked scans of an exclusion filter write (k_scan_masked, k_scan_bf16_masked,
k_scan_i8_masked: DESIGN.md section 23).

The end-to-end tests cannot see a list that lost a row: the certificate refuses it, the exact kernels over the position
list repair the answer.  So the lists themselves are audited.  tests/native/masked_scan_audit.hip ingests one case (N rows,
one query, a set of keep bitmaps), runs each masked kernel once per (mask, metric), merges its lists with the library's
k_merge_lists and writes the 64-entry list -- and the yardstick list beside it: k_scan_subset on the ascending kept
positions for the f32 stage; for bf16 and int8 the unmasked kernel of the same stage on a compacted copy of the slab that
holds only the kept rows, positions mapped back through the kept list.  Per list:
  (d) structure: (key desc, pos asc), no duplicates, every position kept, min(64, m) live entries followed by sentinels;
  (s) positions and key bits equal the yardstick's exactly;
  (e) lattice rows on the f32 stage (small integers: every f32 partial sum is exact, so the host key is the device's bit
      for bit): the list is exactly the host's top 64 of the kept rows by (key desc, position asc).
The masks above are built on the host.  What the library itself builds is audited in the same child: the resolution kernels
of an exclusion token (k_filter_count and k_filter_compact with the predicate inverted, k_filter_bits) run on an id table
with duplicate ids and an id set with absent ids, and
  (r) their count, keep bitmap (every word, no bit at or past N) and position list equal numpy's.
The masks sit on the kernels' boundaries (nothing kept, one row at either end, all, all but one, alternating rows, 63 / 64 /
65 kept, a whole wave step excluded beside a full one, only the partial last step, single bits around the word boundaries).
"""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KP = 64
POS_SENTINEL = 0xFFFFFFFF
MAGIC = 0x414D4C56
COS, EUC, MAN, DOT = 0, 1, 2, 3
METRIC_NAME = {COS: "cosine", EUC: "euclidean", MAN: "manhattan", DOT: "dot"}
STAGE_NAME = ("f32", "bf16", "int8")
VARIANT_BASE = (7_000_000, 8_000_000, 9_000_000)
N = 4133  # 64 full bitmap words and 37 rows: the last row sits in a partial step at every shape
WORDS = (N + 63) // 64

# (lanes per row G, row groups in flight U) of the shape each stage runs at a dim (the first listed shape of the stride)
F32_SHAPES = {128: (8, 3), 384: (8, 1), 768: (16, 1), 1024: (16, 1)}
BF16_SHAPES = {128: (8, 1), 384: (8, 1), 768: (16, 1)}
I8_SHAPES = {128: (8, 1), 384: (8, 1), 768: (8, 1)}
BF16_METRICS, I8_METRICS = (COS, EUC, DOT), (COS, DOT)


# ---- host model of what the f32 kernel reads (tests/test_gpu_subset_jobs_audit.py) ------------------------------------
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


def host_keys(rows, q, metric):
    """The f32 kernel's key of every row, in f64 from the same rounded inputs (exact for lattice rows up to cosine's one
    rounding of key = sum * (1 / |row|))."""
    x32, q32 = f32(rows), f32(q)
    if metric in (COS, DOT):
        p = x32 @ q32
        if metric == COS:
            nrm = np.sqrt(dev_sumsq(rows))
            with np.errstate(divide="ignore"):
                inv = f32(np.where(nrm > 0.0, 1.0 / nrm, 0.0))  # k_ingest: (float)(1.0 / norm)
            return p * inv
        return p
    d = x32 - q32[None, :]
    return -(np.sum(d * d, axis=1) if metric == EUC else np.sum(np.abs(d), axis=1))


def family(name, rng, n, dim):
    if name == "gauss":
        return rng.standard_normal((n, dim)), rng.standard_normal(dim)
    if name == "lattice":  # small integers: every f32 partial sum is exact in any order, and the keys tie massively
        rows = rng.integers(-4, 5, size=(n, dim)).astype(np.float64)
        rows[~rows.any(axis=1), 0] = 1.0
        q = rng.integers(-4, 5, size=dim).astype(np.float64)
        if not q.any():
            q[0] = 1.0
        return rows, q
    raise ValueError(name)


# ---- masks ----------------------------------------------------------------------------------------------------------
def build_masks(rng):
    """[(name, bool[N])]: the keep flags of every mask."""
    def only(rows_kept):
        k = np.zeros(N, dtype=bool)
        k[np.asarray(rows_kept, dtype=np.int64)] = True
        return k

    def without(rows_out):
        k = np.ones(N, dtype=bool)
        k[np.asarray(rows_out, dtype=np.int64)] = False
        return k

    last_full = (N // 64 - 1) * 64  # the first row of the last full word
    toggles = [31, 32, 63, 64, 65, last_full, last_full + 63]
    masks = [
        ("nothing", only([])),
        ("row-0", only([0])),
        ("row-last", only([N - 1])),
        ("all", without([])),
        ("all-but-one", without([N // 2])),
        ("all-but-first", without([0])),
        ("all-but-last", without([N - 1])),
        ("even", only(np.arange(0, N, 2))),
        ("odd", only(np.arange(1, N, 2))),
    ]
    for c in (63, 64, 65):
        masks.append((f"kept-{c}", only(rng.choice(N, size=c, replace=False))))
    # 16 rows are whole wave steps at every shape here (2, 4 or 8 rows per step), beside full ones
    masks.append(("steps-excluded", without(np.arange(128, 144))))
    masks.append(("steps-kept", only(np.arange(128, 144))))
    masks.append(("partial-last-step", only(np.arange(N // 8 * 8, N))))  # rows 4128 .. 4132
    masks.append(("toggles-out", without(toggles)))
    masks.append(("toggles-in", only(toggles)))
    return masks


def pack_masks(masks):
    out = np.zeros((len(masks), WORDS), dtype=np.uint64)
    for i, (_, keep) in enumerate(masks):
        bits = np.zeros(WORDS * 64, dtype=np.uint8)
        bits[:N] = keep
        out[i] = np.packbits(bits.reshape(WORDS, 64), axis=1, bitorder="little").view("<u8").ravel()
    return out


# ---- the audit child ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    d = tmp_path_factory.mktemp("masked_scan_audit")
    exe, obj = d / "masked_scan_audit", d / "masked_scan_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "masked_scan_audit.hip"), "-o", str(obj)],
                arch + [str(obj), os.path.join(vbuild.OBJ, "mfma_scan.o"), "-o", str(exe)]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


_STATE = {"failed_child": None}
CASES = [(fam, dim) for dim in (128, 384, 768, 1024) for fam in ("gauss", "lattice")]


def run_case(exe, fam, dim, tmp_path):
    if _STATE["failed_child"]:
        pytest.fail(f"not started: the audit child of {_STATE['failed_child']} failed")
    rng = np.random.default_rng([dim, sum(map(ord, fam))])
    rows, q = family(fam, rng, N, dim)
    masks = build_masks(rng)
    stages = 1 | (2 if dim in BF16_SHAPES else 0) | (4 if dim in I8_SHAPES else 0)
    pos_ids, id_set = resolution_case(rng, fam, dim)
    src, out = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<11I", MAGIC, 4, COS, EUC, MAN, DOT, N, dim, len(masks), stages, id_set.size))
        f.write(np.ascontiguousarray(rows, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(q, dtype="<f8").tobytes())
        f.write(pack_masks(masks).astype("<u8").tobytes())
        f.write(pos_ids.astype("<u8").tobytes())
        f.write(id_set.astype("<u8").tobytes())
    # the flag is set BEFORE the child starts and cleared only when it exits cleanly: a hang (TimeoutExpired), a crash or
    # any other exception leaves it set, so no later case starts a process on a card that may be wedged
    _STATE["failed_child"] = f"{fam}-d{dim}"
    r = subprocess.run([exe, str(src), str(out)], capture_output=True, text=True, timeout=120)
    if r.returncode == 0 and "audit ok" in r.stdout:
        _STATE["failed_child"] = None
    else:
        pytest.fail(f"audit child exited {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return rows, q, masks, stages, out.read_bytes(), pos_ids, id_set


def resolution_case(rng, fam, dim):
    """(position -> id table with duplicate ids, ascending unique id set with absent ids): the set's size and where its
    rows sit differ per case -- empty, one id, rows 0 and N - 1, a tenth, half, every id."""
    pos_ids = rng.permutation(np.arange(N, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 40))
    pos_ids[100:110] = pos_ids[2000]  # rows that share an id go together
    absent = np.uint64(1 << 41) + np.arange(7, dtype=np.uint64)
    kind = (dim, fam)
    if kind == (128, "gauss"):
        chosen = np.zeros(0, np.uint64)                       # the empty set keeps every row (nf = 0)
    elif kind == (128, "lattice"):
        chosen = pos_ids[[0, N - 1, 2000]]                    # both ends and the duplicated id
    elif kind == (384, "gauss"):
        chosen = np.concatenate([rng.choice(pos_ids, size=N // 10, replace=False), absent])
    elif kind == (384, "lattice"):
        chosen = np.concatenate([pos_ids[::2], absent])       # alternating rows
    elif kind == (768, "gauss"):
        chosen = pos_ids                                       # every id: nothing kept
    elif kind == (768, "lattice"):
        chosen = pos_ids[64:4096]                              # whole words out, the first and the partial last kept
    elif kind == (1024, "gauss"):
        chosen = absent                                        # only ids the table lacks
    else:
        chosen = pos_ids[pos_ids != pos_ids[N // 2]]          # all but one row
    return pos_ids, np.unique(chosen)


def check_resolution(ctx, buf, off, pos_ids, id_set):
    magic, m = struct.unpack_from("<2I", buf, off)
    assert magic == MAGIC
    off += 8
    keep = ~np.isin(pos_ids, id_set)
    assert m == int(keep.sum()), (ctx, "(r) count", m, int(keep.sum()))
    words = np.frombuffer(buf, dtype="<u8", count=WORDS, offset=off)
    off += WORDS * 8
    want = pack_masks([("resolution", keep)])[0]
    assert words.tolist() == want.tolist(), (ctx, "(r) keep bitmap", np.nonzero(words != want)[0][:5])
    plist = np.frombuffer(buf, dtype="<u4", count=m, offset=off)
    off += m * 4
    assert plist.tolist() == np.nonzero(keep)[0].tolist(), (ctx, "(r) position list")
    return off


def parse_blocks(buf, n_blocks):
    blocks, off = [], 0
    while len(blocks) < n_blocks:
        magic, mask, metric, stage, ran, variant, m, yard = struct.unpack_from("<5IiII", buf, off)
        assert magic == MAGIC
        off += 32
        b = {"mask": mask, "metric": metric, "stage": stage, "ran": ran, "variant": variant, "m": m, "yard": yard}
        for name in ([""] if ran else []) + (["yard_"] if yard else []):
            b[name + "key"] = np.frombuffer(buf, dtype="<f4", count=KP, offset=off)
            off += KP * 4
            b[name + "pos"] = np.frombuffer(buf, dtype="<u4", count=KP, offset=off)
            off += KP * 4
        blocks.append(b)
    return blocks, off


def check_list(ctx, b, keep):
    pos, key = b["pos"], b["key"]
    kept = np.nonzero(keep)[0]
    m = kept.size
    assert b["m"] == m, (ctx, "the tool counted other rows", b["m"], m)
    live = pos != POS_SENTINEL
    c = int(live.sum())
    # (d) structure
    assert live[:c].all() and not live[c:].any(), (ctx, "sentinels inside the list")
    assert c == min(KP, m), (ctx, "live entries", c, m)
    p, kd = pos[:c].astype(np.int64), key[:c]
    assert (p < N).all() and keep[p].all(), (ctx, "an excluded position in the list", p[~keep[np.minimum(p, N - 1)]][:4])
    assert len(np.unique(p)) == c, (ctx, "duplicate positions")
    if c > 1:
        order_ok = (kd[:-1] > kd[1:]) | ((kd[:-1] == kd[1:]) & (p[:-1] < p[1:]))
        assert order_ok.all(), (ctx, "list not sorted by (key desc, pos asc)", np.nonzero(~order_ok)[0][:5])
    # (s) the yardstick's list, bit for bit
    assert b["yard"] == (1 if m else 0)
    if m:
        assert pos.tolist() == b["yard_pos"].tolist(), (ctx, "(s) positions differ from the yardstick's")
        assert key[:c].view(np.uint32).tolist() == b["yard_key"][:c].view(np.uint32).tolist(), (ctx, "(s) key bits")
    return p, kd, kept


@pytest.mark.parametrize("fam,dim", CASES, ids=[f"{f}-d{d}" for f, d in CASES])
def test_masked_scan_lists(audit_exe, fam, dim, tmp_path):
    rows, q, masks, stages, buf, pos_ids, id_set = run_case(audit_exe, fam, dim, tmp_path)
    blocks, off = parse_blocks(buf, len(masks) * 4 * 3)
    assert check_resolution(f"{fam}-d{dim}", buf, off, pos_ids, id_set) == len(buf)
    ran = {0: 0, 1: 0, 2: 0}
    keys = {}
    for b in blocks:
        name, keep = masks[b["mask"]]
        stage, metric = b["stage"], b["metric"]
        served = (stage == 0 or (stage == 1 and dim in BF16_SHAPES and metric in BF16_METRICS)
                  or (stage == 2 and dim in I8_SHAPES and metric in I8_METRICS))
        assert bool(b["ran"]) == served, (name, METRIC_NAME[metric], STAGE_NAME[stage])
        if not served:
            continue
        ran[stage] += 1
        g, u = (F32_SHAPES, BF16_SHAPES, I8_SHAPES)[stage][dim]
        v = b["variant"] - VARIANT_BASE[stage]
        assert v // 10000 == g and v % 100 == u, (STAGE_NAME[stage], b["variant"])  # the shape the masks were laid out for
        ctx = (f"{fam}-d{dim}", name, METRIC_NAME[metric], STAGE_NAME[stage])
        p, kd, kept = check_list(ctx, b, keep)
        if fam == "lattice" and stage == 0 and kept.size:  # (e)
            if metric not in keys:
                keys[metric] = host_keys(rows, q, metric)
            k32 = f32(keys[metric][kept])
            if metric != COS:
                assert (k32 == keys[metric][kept]).all() and np.abs(k32).max() < 2.0 ** 24
            want = np.lexsort((kept, -k32))[:KP]
            assert p.tolist() == kept[want].tolist(), (ctx, "(e) positions", p[:6], kept[want][:6])
            assert (kd == k32[want]).all(), (ctx, "(e) key bits")
    assert ran[0] == len(masks) * 4
    assert ran[1] == (len(masks) * 3 if dim in BF16_SHAPES else 0)
    assert ran[2] == (len(masks) * 2 if dim in I8_SHAPES else 0)

"""Audit of the 64-entry lists the mask-aware MFMA batch filter writes (launch_mfma_candidates_masked).

The end-to-end tests (tests/test_gpu_masked_batch.py) cannot see a list that lost a row: the certificate refuses it and the
jobs route repairs the answer.  tests/native/masked_mfma_audit.hip runs the launcher on a data set with one keep bitmap per
query and dumps every list; judged here:
  * structure: sorted by (key desc, position asc), no duplicates, every position kept and below N, min(64, kept) live
    entries and sentinels behind them;
  * lattice rows (small integers: every bf16 product sum is exact in any order): the list is the host's top 64 of the
    kept rows -- positions and keys -- computed with the key model of tests/_range_batch_cases.py;
  * gaussian rows: positions and key bits equal the UNMASKED launch_mfma_candidates on a slab of the kept rows only,
    positions mapped back (a row's key does not depend on its position), for every mask keeping >= MFMA_MIN_ROWS rows;
  * a candidate buffer may overflow only under the masks that keep fewer than 64 rows; anywhere else an overflow is a
    failed case.
N = 8192 + 32 * 3 + 5 rows (above MFMA_MIN_ROWS, last block and last bitmap word partial), strides 128 / 384 / 768, 3 queries
(one chunk: the streaming pass 1) and 130 (two chunks: the plain one), VL_MFMA_STAGES 1 and 4 (k_refine_thresholds on masked
candidates), three metrics.  One child process at a time; after a child failed, crashed or timed out no later case starts one.
"""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _range_batch_cases as RB  # noqa: E402
from _filter_host_model import HostRows, family  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAGIC = 0x4D4D4C56
N = 8192 + 32 * 3 + 5
NQ_ALL = 130
KP = 64
CAP = 4096
MIN_ROWS = 8192
SENTINEL = 0xFFFFFFFF
N_TYPES = 14
_STATE = {"failed_child": None}
COUNTS = {"lists judged": 0, "compared with the host's top 64": 0, "compared with the unmasked yardstick": 0}


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    vbuild.build()  # the MFMA launchers: mfma_scan.o of the library build
    d = tmp_path_factory.mktemp("masked_mfma_audit")
    exe, obj = d / "masked_mfma_audit", d / "masked_mfma_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "masked_mfma_audit.hip"), "-o", str(obj)],
                arch + [str(obj), os.path.join(vbuild.OBJ, "mfma_scan.o"), "-o", str(exe)]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


@pytest.fixture(scope="module", autouse=True)
def count_report():
    yield
    print("\nmasked MFMA audit: " + ", ".join(f"{v} {k}" for k, v in COUNTS.items()))


def run_child(args, what):
    """One child at a time; once one has failed, hung or crashed no later case starts a process on the card."""
    if _STATE["failed_child"]:
        pytest.fail(f"not started: the audit child of {_STATE['failed_child']} failed")
    _STATE["failed_child"] = what  # cleared only on a clean exit: a timeout or a crash leaves it set
    r = subprocess.run(args, capture_output=True, text=True, timeout=180)
    if r.returncode == 0 and r.stdout.rstrip().endswith("audit ok"):
        _STATE["failed_child"] = None
    else:
        pytest.fail(f"audit child exited {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")


def make_masks(order):
    """One keep mask (bool [N]) per query, the 14 kinds cycled; order[q] = rows by decreasing (approximate) key of query q."""
    last_full_word = (N // 64) * 64  # first row of the partial last word
    toggles = [31, 32, 63, 64, 65, last_full_word - 65, last_full_word - 64, last_full_word - 1, last_full_word, last_full_word + 1]
    tail = np.arange((N // 32) * 32, N)  # the partial last block's rows
    masks = []
    for q in range(NQ_ALL):
        kind, keep = q % N_TYPES, np.ones(N, bool)
        if kind == 1:
            keep[N - 2] = False                      # all but one (a row of the partial last block)
        elif kind == 2:
            keep[order[q][:KP]] = False              # the query's own top 64
        elif kind == 3:
            keep[1::2] = False                       # even rows
        elif kind == 4:
            keep[0::2] = False                       # odd rows
        elif kind == 5:
            keep[7 * 32:8 * 32] = False              # a whole 32-row block beside full ones
        elif kind == 6:
            keep[tail] = False                       # only the partial last block's rows
        elif kind == 7:
            keep[:] = False
            keep[tail] = True                        # ... and only those kept
        elif kind == 8:
            keep[toggles] = False                    # single bits at the field and word borders
        elif kind == 9:
            keep[:] = False
            keep[toggles] = True
        elif kind in (10, 11, 12):
            keep[:] = False
            keep[order[q][3:3 + 53 + kind]] = True   # exactly 63 / 64 / 65 rows
        elif kind == 13:
            keep[:] = False                          # nothing
        masks.append(keep)
    return masks


def pack(mask):
    bits = np.zeros(-(-N // 64) * 64, np.uint8)
    bits[:N] = mask
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8")


def run_case(exe, tmp_path, rows, queries, masks, runs):
    src, out = tmp_path / "case.bin", tmp_path / "out.bin"
    dim = rows.shape[1]
    with open(src, "wb") as f:
        f.write(struct.pack("<5I", MAGIC, N, dim, NQ_ALL, len(runs)))
        f.write(np.asarray(runs, dtype="<u4").tobytes())
        f.write(np.ascontiguousarray(rows, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(queries, dtype="<f8").tobytes())
        f.write(np.asarray([RB.seq_norm(q) for q in queries], dtype="<f8").tobytes())
        f.write(np.concatenate([pack(m) for m in masks]).tobytes())
    run_child([exe, str(src), str(out)], f"dim {dim}")
    buf, at, res = out.read_bytes(), 0, []
    for kind, metric, nq, stages, mask in runs:
        magic, scanned = struct.unpack_from("<2I", buf, at)
        assert magic == MAGIC
        at += 8
        cnt = np.frombuffer(buf, "<u4", nq, at)
        at += 4 * nq
        ent = np.frombuffer(buf, "<u4", nq * KP * 2, at).reshape(nq, KP, 2)
        at += 8 * nq * KP
        res.append({"scanned": scanned, "cnt": cnt, "key": ent[:, :, 0].copy().view("<f4"), "pos": ent[:, :, 1]})
    assert at == len(buf)
    return res


def judge_structure(ctx, keep, cnt, key, pos):
    """Returns the live (keys, positions) of one masked list; None for a buffer that overflowed where it may."""
    m = int(keep.sum())
    if cnt > CAP and m < KP:  # fewer than 64 kept rows leave the thresholds at -inf: the host redoes such a query
        return None
    assert cnt <= CAP, (ctx, "candidate overflow", int(cnt), m)
    live = min(KP, m)
    assert (pos[live:] == SENTINEL).all() and (pos[:live] != SENTINEL).all(), (ctx, "live entries", live, pos.tolist())
    p, k = pos[:live].astype(np.int64), key[:live]
    assert (p < N).all() and keep[p].all(), (ctx, "an excluded or out-of-range row in the list")
    assert len(set(p.tolist())) == live, (ctx, "duplicates")
    for a in range(live - 1):
        assert k[a] > k[a + 1] or (k[a] == k[a + 1] and p[a] < p[a + 1]), (ctx, "order", a)
    COUNTS["lists judged"] += 1
    return k, p


def masked_runs():
    return [(0, metric, nq, stages, 0) for metric in RB.MFMA_METRICS for nq in (3, NQ_ALL) for stages in (1, 4)]


@pytest.mark.parametrize("dim", [128, 384, 768])
def test_lattice_lists_are_the_top_64_of_the_kept_rows(audit_exe, dim, tmp_path):
    rng = np.random.default_rng([24, dim])
    rows, queries = family("lattice", rng, N, dim, NQ_ALL)
    h = HostRows(rows)
    keys = {m: RB.mfma_keys32(h, queries, m) for m in RB.MFMA_METRICS}
    order = [np.lexsort((np.arange(N), -keys[RB.COS][q].astype(np.float64))) for q in range(NQ_ALL)]
    masks = make_masks(order)
    runs = masked_runs()
    for run, o in zip(runs, run_case(audit_exe, tmp_path, rows, queries, masks, runs)):
        _, metric, nq, stages, _ = run
        for q in range(nq):
            ctx = ("lattice", dim, RB.METRIC_NAME[metric], nq, stages, q, q % N_TYPES)
            live = judge_structure(ctx, masks[q], o["cnt"][q], o["key"][q], o["pos"][q])
            if live is None:
                continue
            k, p = live
            kept = np.nonzero(masks[q])[0]
            kk = keys[metric][q][kept]
            top = kept[np.lexsort((kept, -kk.astype(np.float64)))][:KP]
            assert p.tolist() == top.tolist(), (ctx, "positions")
            assert (k == keys[metric][q][top]).all(), (ctx, "keys")
            COUNTS["compared with the host's top 64"] += 1


@pytest.mark.parametrize("dim", [128, 384, 768])
def test_gaussian_lists_equal_the_unmasked_filter_on_the_kept_rows(audit_exe, dim, tmp_path):
    rng = np.random.default_rng([25, dim])
    rows, queries = family("gauss", rng, N, dim, NQ_ALL)
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    order = [np.argsort(-(unit @ q), kind="stable") for q in queries]
    masks = make_masks(order)
    # yardsticks: one unmasked run per metric on the kept rows of every distinct mask that keeps >= MFMA_MIN_ROWS rows --
    # the kinds shared by all their queries once, the per-query kind (own top 64 excluded) for its first two queries
    packed = [pack(m).tobytes() for m in masks]
    first = {}
    for q in range(NQ_ALL):
        if masks[q].sum() >= MIN_ROWS and (q % N_TYPES != 2 or q < 2 * N_TYPES):
            first.setdefault(packed[q], q)
    yard = [(1, metric, NQ_ALL, 1, q) for metric in RB.MFMA_METRICS for q in first.values()]
    runs = masked_runs() + yard
    outs = run_case(audit_exe, tmp_path, rows, queries, masks, runs)
    ref = {}
    for run, o in zip(runs, outs):
        if run[0] == 1:
            assert o["scanned"] == masks[run[4]].sum() and (o["cnt"] <= CAP).all(), ("the yardstick overflowed", run)
            ref[(run[1], packed[run[4]])] = o
    compared = 0
    for run, o in zip(runs, outs):
        kind, metric, nq, stages, _ = run
        if kind != 0:
            continue
        for q in range(nq):
            ctx = ("gauss", dim, RB.METRIC_NAME[metric], nq, stages, q, q % N_TYPES)
            live = judge_structure(ctx, masks[q], o["cnt"][q], o["key"][q], o["pos"][q])
            y = ref.get((metric, packed[q]))
            if y is None:
                continue
            assert live is not None
            k, p = live
            back = np.nonzero(masks[q])[0]
            assert p.tolist() == back[y["pos"][q].astype(np.int64)].tolist(), (ctx, "positions against the yardstick")
            assert k.view(np.uint32).tolist() == y["key"][q].view(np.uint32).tolist(), (ctx, "key bits against the yardstick")
            compared += 1
    assert compared >= 3 * 2 * (3 + 40), compared  # every metric and stage count, both batch sizes
    COUNTS["compared with the unmasked yardstick"] += compared

"""The batched diversified (MMR) search as far as it can be checked without a GPU: the three symbols
through every layer, the argument checks that need no device, the routing rule of csrc/mmr_batch_plan.hpp through a
stand-alone host program, the gfx950 ISA of the two new kernels (k_mmr_batch_rank, k_mmr_batch_select, three metrics each),
and the register / scratch / LDS figures of the kernels the batch runs beside or leaves alone, which must be those of the
commit before this entry point existed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vl_index_search_mmr_batch", "vl_index_set_mmr_batch", "vl_index_last_mmr_batch")
VL_ERR_INVALID_ARG = 8
LDS_PER_WORKGROUP = 64 * 1024  # the static limit a gfx950 workgroup may declare


@pytest.fixture(scope="module")
def L():
    from vectorlite_amd import _lib
    return _lib.load()


def test_the_symbols_are_declared_exported_and_bound(L):
    from vectorlite_amd import _lib
    header = open(os.path.join(ROOT, "include", "vectorlite_amd.h")).read()
    for s in NEW:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in _lib.SYMBOLS
        assert hasattr(L, s)
    import vectorlite_amd as V
    for name in ("search_mmr_batch_arrays", "search_mmr_batch", "set_mmr_batch", "last_mmr_batch"):
        assert hasattr(V.FlatIndex, name)
    for name in ("search_mmr_batch_arrays", "search_mmr_batch"):
        assert hasattr(V.HNSWIndex, name)
        assert hasattr(V.MultiFlatIndex, name)
    assert V.MMR_BATCH_MODES == {"off": 0, "on": 1, "auto": 2}
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "index", "gpu.rs")).read()
    for s in NEW:
        assert ("fn %s(" % s) in rust
    assert "pub fn search_mmr_batch(" in rust


def _call(L, h, k, fetch_k, lam, nq=2, out_n=True, stride=None):
    q = np.zeros((max(nq, 1), 4))
    stride = k if stride is None else stride
    ids = np.zeros(max(nq * stride, 1), dtype=np.uint64)
    sc = np.zeros(ids.size)
    n = np.full(max(nq, 1), 77, dtype=np.uint64)
    rc = L.vl_index_search_mmr_batch(h, 0, q.ctypes.data, nq, 4, k, fetch_k, lam, 0, stride, ids.ctypes.data, sc.ctypes.data,
                                     n.ctypes.data if out_n else None)
    return rc, n, L.vl_last_error().decode()


def test_argument_checks_that_need_no_device(L):
    # the single call's checks in its order and with its texts, before the handle is looked at
    q = (C.c_double * 4)(1, 0, 0, 0)
    one = C.c_uint64(0)

    def single(k, fetch_k, lam):
        rc = L.vl_index_search_mmr(None, 0, C.cast(q, C.c_void_p), 4, k, fetch_k, lam, 0, 8, None, None, C.byref(one))
        return rc, L.vl_last_error().decode()

    for k, fetch_k, lam, word in ((4, 20, float("nan"), "lambda"), (4, 20, -0.1, "lambda"), (4, 20, 1.1, "lambda"),
                                  (21, 20, 0.5, "fetch_k must be at least k"), (4, 1025, 0.5, "VL_MMR_MAX_FETCH")):
        rc, n, msg = _call(L, None, k, fetch_k, lam)
        assert rc == VL_ERR_INVALID_ARG and word in msg, (k, fetch_k, lam, rc, msg)
        assert (rc, msg) == single(k, fetch_k, lam)
        assert n.tolist() == [77, 77]  # nothing was written
    # lambda is checked before fetch_k < k, that before the limit
    assert "lambda" in _call(L, None, 21, 20, 2.0)[2]
    assert "at least k" in _call(L, None, 2000, 1025, 0.5)[2]
    # a null handle with everything else in order (nq = 0 included), the limits themselves
    assert _call(L, None, 4, 20, 0.5)[0] == VL_ERR_INVALID_ARG
    assert _call(L, None, 4, 20, 0.5, nq=0)[0] == VL_ERR_INVALID_ARG
    assert _call(L, None, 4, 1024, 1.0)[0] == VL_ERR_INVALID_ARG
    assert L.vl_index_set_mmr_batch(None, 1) == VL_ERR_INVALID_ARG
    v = C.c_uint64(0)
    assert L.vl_index_last_mmr_batch(None, C.byref(v), None, None, None) == VL_ERR_INVALID_ARG


def test_a_null_out_n_nq_zero_and_an_unknown_mode(L):
    # (a flat handle needs a device; without one the null handle is what answers -- the refusals have the same status)
    h = C.c_void_p()
    made = L.vl_flat_create(4, 0, C.byref(h)) == 0
    try:
        rc, _, _ = _call(L, h if made else None, 4, 20, 0.5, out_n=False)
        assert rc == VL_ERR_INVALID_ARG
        if made:
            assert L.vl_index_set_mmr_batch(h, 3) == VL_ERR_INVALID_ARG and L.vl_index_set_mmr_batch(h, -1) == VL_ERR_INVALID_ARG
            for mode in (0, 1, 2):
                assert L.vl_index_set_mmr_batch(h, mode) == 0
            rc, n, _ = _call(L, h, 4, 20, 0.5, nq=0, out_n=False)  # nq = 0 is fine and writes nothing
            assert rc == 0 and n.tolist() == [77]
            rc, n, _ = _call(L, h, 4, 20, 1.1, nq=0)  # ... after the argument checks
            assert rc == VL_ERR_INVALID_ARG
            rc, n, _ = _call(L, h, 4, 20, 0.5)  # an empty index: zeros
            assert rc == 0 and n.tolist() == [0, 0]
            v = [C.c_uint64(9) for _ in range(4)]
            assert L.vl_index_last_mmr_batch(h, *[C.byref(x) for x in v]) == 0
            assert [x.value for x in v] == [0, 0, 0, 0]
    finally:
        if made:
            L.vl_index_destroy(h)


# ---- the routing rule ----------------------------------------------------------------------------------------------------
def test_the_routing_rule_on_the_cpu(tmp_path):
    exe = tmp_path / "mmr_batch_plan_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "mmr_batch_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "mmr batch plan ok" in r.stdout
    assert "20000 shapes checked" in r.stdout


def test_the_plan_header_is_host_only_and_says_its_estimates_are_derived():
    text = open(os.path.join(ROOT, "vectorlite_amd", "csrc", "mmr_batch_plan.hpp")).read()
    assert "hip" not in text.split("#pragma once", 1)[1].lower()
    assert "BOTH ESTIMATES ARE DERIVED" in text and "not fitted" in text


# ---- the ISA of the new kernels, and the figures of the old ones ------------------------------------------------------------
@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    d = tmp_path_factory.mktemp("isa_mmr_batch")
    procs = {}
    for src in ("mmr.hip", "kernels.hip"):
        cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
            "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, src), "-o", str(d / (src + ".s"))]
        procs[src] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    for src, p in procs.items():
        out, _ = p.communicate(timeout=1200)
        assert p.returncode == 0, out.decode()[-3000:]
    return {src: (d / (src + ".s")).read_text() for src in procs}


def _kernels_of(asm, pattern):
    """{mangled name: (body, metadata)} of the kernels whose name matches `pattern`"""
    meta = {}
    for block in asm.split("- .agpr_count:")[1:]:
        meta[re.search(r"\.name:\s+(\S+)", block).group(1)] = "- .agpr_count:" + block
    found = {}
    for m in re.finditer(r"^(_Z\S*?%s\S*):[^\n]*\n(.*?)s_endpgm" % pattern, asm, flags=re.S | re.M):
        found[m.group(1)] = (m.group(2), meta[m.group(1)])
    return found


def _int(meta, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def _figures(meta):
    return (_int(meta, "vgpr_count"), _int(meta, "agpr_count"), _int(meta, "sgpr_count"), _int(meta, "private_segment_fixed_size"),
            _int(meta, "group_segment_fixed_size"))


def _no_scratch_no_spills(name, body, meta):
    print("%s: VGPRs %d, AGPRs %d, SGPRs %d, scratch %d, LDS %d" % ((name,) + _figures(meta)))
    assert _int(meta, "private_segment_fixed_size") == 0 and "scratch_" not in body
    assert _int(meta, "vgpr_spill_count") == 0 and _int(meta, "sgpr_spill_count") == 0
    assert _int(meta, "group_segment_fixed_size") <= LDS_PER_WORKGROUP


def test_the_rank_kernel_has_three_forms_without_scratch_spills_or_lds(device_asm):
    ks = _kernels_of(device_asm["mmr.hip"], "16k_mmr_batch_rank")
    assert sorted(int(re.search(r"k_mmr_batch_rankILi(\d)E", n).group(1)) for n in ks) == [0, 1, 3]
    for name, (body, meta) in ks.items():
        _no_scratch_no_spills(name, body, meta)
        assert _int(meta, "group_segment_fixed_size") == 0 and "ds_" not in body
        assert "v_readlane_b32" in body  # the ranking reads candidates lane by lane
        # no arithmetic of the reference's is done here: scores pass through as their bits.  (The bound's own division and
        # square root are expanded by the compiler with v_fma_f64, as in k_batch_rank_collapse.)
        first_fma = body.find("v_fma_f64")
        assert first_fma == -1 or "v_rsq_f64" in body[:first_fma] or "v_rcp_f64" in body[:first_fma], name


def test_the_select_kernel_has_three_forms_and_rounds_every_multiply_and_add_separately(device_asm):
    ks = _kernels_of(device_asm["mmr.hip"], "18k_mmr_batch_select")
    metrics = {int(re.search(r"k_mmr_batch_selectILi(\d)E", n).group(1)): v for n, v in ks.items()}
    assert sorted(metrics) == [0, 1, 3]  # cosine, Euclidean, dot: the batch filter's metrics
    for name, (body, meta) in ks.items():
        _no_scratch_no_spills(name, body, meta)
        # the 60 x 60 similarity matrix and one chunk of 64 staged rows live in LDS
        assert 60 * 60 * 8 + 64 * 32 * 8 <= _int(meta, "group_segment_fixed_size") <= 48 * 1024
        assert "v_mul_f64" in body and "v_add_f64" in body
    # dot: no square root, no division -- no v_fma_f64 anywhere, neither in the chains nor in the selection
    assert "v_fma_f64" not in metrics[3][0]
    # cosine and Euclidean: score() ends in a correctly rounded sqrt and division, which the compiler expands WITH v_fma_f64;
    # the exact kernels' rule (tests/test_mmr_search_cpu.py): nothing in front of the first v_rsq_f64 / v_rcp_f64 -- the
    # chains -- contains one; the selection's two multiplies and its subtraction come behind the last of them; and there
    # are at most as many as the up to seven score() expansions of a thread hold (nine each under cosine)
    for metric in (0, 1):
        body = metrics[metric][0]
        first_fma, last_fma = body.find("v_fma_f64"), body.rfind("v_fma_f64")
        assert first_fma != -1
        assert "v_rsq_f64" in body[:first_fma] or "v_rcp_f64" in body[:first_fma], metric
        assert body.count("v_fma_f64") <= 7 * 9, metric
        assert body[last_fma:].count("v_mul_f64") >= 2 and "v_add_f64" in body[last_fma:], metric


# A compiler upgrade changes these figures without any kernel change.  To regenerate the table: check out the commit before
# this entry point (the parent of "Add exact batched diversified (MMR) search"), compile csrc/kernels.hip and csrc/mmr.hip
# there with build.COMMON + ["--cuda-device-only", "-S"] as the device_asm fixture below does, and read vgpr_count,
# agpr_count, sgpr_count, private_segment_fixed_size and group_segment_fixed_size of each kernel's metadata block
# (_figures); then run this test on the current tree with the new compiler.
# (vgpr, agpr, sgpr, scratch bytes, LDS bytes) of the parent commit's build, same compiler and flags: k_batch_rescore,
# k_batch_rank_emit, k_batch_rank_emit_rows, k_batch_rank_collapse (kernels.hip), k_mmr_pairwise, k_mmr_select (mmr.hip)
PARENT_FIGURES = {
    "k_batch_rescoreILi0E": (76, 0, 41, 0, 15824), "k_batch_rescoreILi1E": (76, 0, 32, 0, 8416),
    "k_batch_rescoreILi2E": (76, 0, 32, 0, 8416), "k_batch_rescoreILi3E": (76, 0, 32, 0, 8416),
    "k_batch_rank_emitILi0E": (22, 0, 42, 0, 0), "k_batch_rank_emitILi1E": (22, 0, 42, 0, 0),
    "k_batch_rank_emitILi2E": (22, 0, 42, 0, 0), "k_batch_rank_emitILi3E": (16, 0, 46, 0, 0),
    "k_batch_rank_emit_rowsILi0E": (24, 0, 25, 0, 0), "k_batch_rank_emit_rowsILi1E": (24, 0, 26, 0, 0),
    "k_batch_rank_emit_rowsILi2E": (24, 0, 25, 0, 0), "k_batch_rank_emit_rowsILi3E": (18, 0, 30, 0, 0),
    "k_batch_rank_collapseILi0E": (22, 0, 33, 0, 0), "k_batch_rank_collapseILi1E": (22, 0, 37, 0, 0),
    "k_batch_rank_collapseILi3E": (14, 0, 37, 0, 0),
    "k_mmr_pairwiseILi0E": (88, 0, 36, 0, 8448), "k_mmr_pairwiseILi1E": (64, 0, 36, 0, 8448),
    "k_mmr_pairwiseILi2E": (64, 0, 36, 0, 8448), "k_mmr_pairwiseILi3E": (64, 0, 36, 0, 8448),
    "k_mmr_selectENS": (42, 0, 30, 0, 20992),
}


def test_the_kernels_left_alone_keep_the_parent_builds_figures(device_asm):
    seen = {}
    for src, pattern in (("kernels.hip", r"\d+k_batch_(?:rescore|rank_emit|rank_emit_rows|rank_collapse)I"),
                         ("mmr.hip", r"\d+k_mmr_(?:pairwiseI|selectE)")):
        for name, (body, meta) in _kernels_of(device_asm[src], pattern).items():
            key = re.search(r"\d+(k_(?:batch|mmr)_\w+?(?:ILi\dE|ENS))", name).group(1)
            seen[key] = _figures(meta)
    assert seen == PARENT_FIGURES

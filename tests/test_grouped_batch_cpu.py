"""The batched grouped search as far as it can be checked without a GPU: the three symbols through every
layer, the argument checks that need no device, the routing rule of csrc/grouped_batch_plan.hpp through a stand-alone host
program, and the gfx950 ISA of the two new kernels (k_batch_rank_collapse in three metrics, k_group_keep_bits)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vl_index_search_grouped_batch", "vl_index_set_grouped_batch", "vl_index_last_grouped_batch")
VL_ERR_INVALID_ARG = 8


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
    for name in ("search_grouped_batch_arrays", "search_grouped_batch", "set_grouped_batch", "last_grouped_batch"):
        assert hasattr(V.FlatIndex, name)
    for name in ("search_grouped_batch_arrays", "search_grouped_batch"):
        assert hasattr(V.HNSWIndex, name)
    assert V.VL_ERR_INVALID_ARG == VL_ERR_INVALID_ARG


def _call(L, h, groups, k, nq=2, out_n=True, stride=None):
    q = np.zeros((max(nq, 1), 4))
    stride = k if stride is None else stride
    keys = np.zeros(max(nq * stride, 1), dtype=np.uint64)
    ids = np.zeros_like(keys)
    sc = np.zeros(keys.size)
    n = np.full(max(nq, 1), 77, dtype=np.uint64)
    rc = L.vl_index_search_grouped_batch(h, groups, 0, q.ctypes.data, nq, 4, k, 0, stride, keys.ctypes.data, ids.ctypes.data,
                                         sc.ctypes.data, n.ctypes.data if out_n else None)
    return rc, n


def test_argument_checks_that_need_no_device(L):
    # k beyond the limit: the single call's status and text, before the handle is looked at
    rc, n = _call(L, None, 5, 1025)
    assert rc == VL_ERR_INVALID_ARG
    assert L.vl_last_error().decode() == "grouped search: k exceeds VL_GROUPED_MAX_K (1024)"
    q = np.zeros(4)
    one = C.c_uint64(0)
    assert L.vl_index_search_grouped(None, 5, 0, q.ctypes.data, 4, 1025, 0, 0, None, None, None, C.byref(one)) == VL_ERR_INVALID_ARG
    assert L.vl_last_error().decode() == "grouped search: k exceeds VL_GROUPED_MAX_K (1024)"
    # token 0 is no table: the single call's text again
    rc, n = _call(L, None, 0, 10)
    assert rc == VL_ERR_INVALID_ARG
    assert L.vl_last_error().decode() == "unknown or destroyed group table"
    # k is checked before the token
    rc, n = _call(L, None, 0, 1025)
    assert rc == VL_ERR_INVALID_ARG and "VL_GROUPED_MAX_K" in L.vl_last_error().decode()
    # a null handle, with everything else in order; nothing was written
    rc, n = _call(L, None, 5, 10)
    assert rc == VL_ERR_INVALID_ARG and n.tolist() == [77, 77]
    rc, n = _call(L, None, 5, 10, nq=0)
    assert rc == VL_ERR_INVALID_ARG
    assert L.vl_index_set_grouped_batch(None, 1) == VL_ERR_INVALID_ARG
    v = C.c_uint64(0)
    assert L.vl_index_last_grouped_batch(None, C.byref(v), None, None, None) == VL_ERR_INVALID_ARG


def test_a_null_out_n_is_refused_by_a_live_handle_or_a_null_one(L):
    # (a flat handle needs a device; without one the null handle is what answers -- either way the status is the same)
    h = C.c_void_p()
    made = L.vl_flat_create(4, 0, C.byref(h)) == 0
    try:
        rc, _ = _call(L, h if made else None, 5, 10, out_n=False)
        assert rc == VL_ERR_INVALID_ARG
        if made:
            assert L.vl_index_set_grouped_batch(h, 3) == VL_ERR_INVALID_ARG
            assert L.vl_index_set_grouped_batch(h, 0) == 0 and L.vl_index_set_grouped_batch(h, 2) == 0
            rc, n = _call(L, h, 5, 10, nq=0, out_n=False)  # nq = 0 is fine and writes nothing
            assert rc == 0
    finally:
        if made:
            L.vl_index_destroy(h)


# ---- the routing rule ----------------------------------------------------------------------------------------------------
def test_the_routing_rule_on_the_cpu(tmp_path):
    exe = tmp_path / "grouped_batch_plan_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "grouped_batch_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "grouped batch plan ok" in r.stdout
    assert "20000 shapes checked" in r.stdout


def test_the_plan_header_is_host_only_and_says_its_estimates_are_derived():
    text = open(os.path.join(ROOT, "vectorlite_amd", "csrc", "grouped_batch_plan.hpp")).read()
    assert "hip" not in text.split("#pragma once", 1)[1].lower()
    assert "DERIVED" in text and "profiles/grouped_batch_10000000x384.jsonl" in text
    assert os.path.exists(os.path.join(ROOT, "profiles", "grouped_batch_10000000x384.jsonl"))


# ---- the ISA of the new kernels ------------------------------------------------------------------------------------------
def _kernels_of(src, tmp, pattern):
    """{mangled name: (body, metadata)} of the kernels of csrc/<src> whose name matches `pattern`"""
    from vectorlite_amd import build as vbuild
    out = tmp / (src + ".s")
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
        "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, src), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    asm = out.read_text()
    meta = {}
    for block in asm.split("- .agpr_count:")[1:]:
        meta[re.search(r"\.name:\s+(\S+)", block).group(1)] = "- .agpr_count:" + block
    found = {}
    for m in re.finditer(r"^(_Z\S*?%s\S*):[^\n]*\n(.*?)s_endpgm" % pattern, asm, flags=re.S | re.M):
        found[m.group(1)] = (m.group(2), meta[m.group(1)])
    return found


def _int(meta, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def _no_scratch_no_spills(name, meta):
    print("%s: %d VGPRs, %d SGPRs, scratch %d, LDS %d" % (name, _int(meta, "vgpr_count"), _int(meta, "sgpr_count"),
                                                          _int(meta, "private_segment_fixed_size"), _int(meta, "group_segment_fixed_size")))
    assert _int(meta, "private_segment_fixed_size") == 0
    assert _int(meta, "vgpr_spill_count") == 0 and _int(meta, "sgpr_spill_count") == 0


def test_the_collapse_kernel_has_three_forms_without_scratch_spills_or_lds(tmp_path):
    ks = _kernels_of("kernels.hip", tmp_path, "21k_batch_rank_collapse")
    metrics = sorted(int(re.search(r"k_batch_rank_collapseILi(\d)E", n).group(1)) for n in ks)
    assert metrics == [0, 1, 3]  # cosine, Euclidean, dot: the batch filter's metrics
    for name, (body, meta) in ks.items():
        _no_scratch_no_spills(name, meta)
        assert _int(meta, "group_segment_fixed_size") == 0
        assert "v_readlane_b32" in body  # the ranking and the collapse read candidates lane by lane
        assert "ds_" not in body


def test_the_keep_bits_kernel_has_no_scratch_and_no_spills(tmp_path):
    ks = _kernels_of("grouped.hip", tmp_path, "17k_group_keep_bits")
    assert len(ks) == 1
    for name, (body, meta) in ks.items():
        _no_scratch_no_spills(name, meta)
        assert _int(meta, "group_segment_fixed_size") == 0

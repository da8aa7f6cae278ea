"""CPU-side checks of the diversified (MMR) search (vl_index_search_mmr): the symbol, the argument checks that need no
device, and the gfx950 ISA of its two kernels (mmr.hip, cross-compiled here).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VL_ERR_INVALID_ARG = 8


@pytest.fixture(scope="module")
def lib():
    from vectorlite_amd import build
    build.build()
    from vectorlite_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    assert "mmr.hip" in vbuild.SOURCES
    out = tmp_path_factory.mktemp("isa_mmr") / "mmr.s"
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
        "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, "mmr.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def _kernel(asm, mangled_fragment):
    m = re.search(r"^(_Z\S*%s\S*):[^\n]*\n(.*?)s_endpgm" % re.escape(mangled_fragment), asm, flags=re.S | re.M)
    assert m, mangled_fragment
    name = m.group(1)
    meta = [b for b in asm.split("- .agpr_count:")[1:] if re.search(r"\.name:\s+%s\s" % re.escape(name), b)]
    assert len(meta) == 1, name
    return m.group(2), meta[0]


def _meta_int(meta, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def _no_spills(body, meta):
    assert "scratch_" not in body and "buffer_store" not in body
    assert _meta_int(meta, "private_segment_fixed_size") == 0
    assert not re.search(r"\.(vgpr|sgpr)_spill_count:\s+[1-9]", meta)


def test_symbol_is_declared_and_exported(lib):
    from vectorlite_amd import _lib
    header = open(os.path.join(ROOT, "include", "vectorlite_amd.h")).read()
    assert re.search(r"\bvl_index_search_mmr\s*\(", header)
    assert re.search(r"#define\s+VL_MMR_MAX_FETCH\s+1024\b", header)
    assert hasattr(lib, "vl_index_search_mmr")
    assert "vl_index_search_mmr" in _lib.SYMBOLS


def test_argument_checks_need_no_device(lib):
    q = (C.c_double * 4)(1, 0, 0, 0)
    out_ids = (C.c_uint64 * 8)()
    out_sc = (C.c_double * 8)()

    def call(k, fetch_k, lam, h=None):
        n = C.c_uint64(7)
        rc = lib.vl_index_search_mmr(h, 0, C.cast(q, C.c_void_p), 4, k, fetch_k, lam, 0, 8, C.cast(out_ids, C.c_void_p),
                                     C.cast(out_sc, C.c_void_p), C.byref(n))
        return rc, n.value, lib.vl_last_error().decode()

    # the argument checks answer before the handle is looked at: their own message, *out_n = 0
    for lam in (float("nan"), -0.1, 1.5):
        rc, n, msg = call(4, 20, lam)
        assert rc == VL_ERR_INVALID_ARG and n == 0 and "lambda" in msg, (lam, rc, msg)
    rc, n, msg = call(21, 20, 0.5)
    assert rc == VL_ERR_INVALID_ARG and n == 0 and "fetch_k" in msg
    rc, n, msg = call(4, 1025, 0.5)
    assert rc == VL_ERR_INVALID_ARG and n == 0 and "VL_MMR_MAX_FETCH" in msg
    rc, n, _ = call(4, 20, 0.5)  # a null handle
    assert rc == VL_ERR_INVALID_ARG and n == 0
    rc, n, _ = call(4, 1024, 1.0)  # the limits themselves pass the argument checks: still the null handle
    assert rc == VL_ERR_INVALID_ARG and n == 0
    assert lib.vl_index_search_mmr(None, 0, C.cast(q, C.c_void_p), 4, 4, 20, 0.5, 0, 8, C.cast(out_ids, C.c_void_p),
                                   C.cast(out_sc, C.c_void_p), None) == VL_ERR_INVALID_ARG


def test_select_rounds_v_with_separate_multiplies_and_a_subtract(device_asm):
    body, meta = _kernel(device_asm, "12k_mmr_select")
    assert "v_mul_f64" in body and "v_add_f64" in body  # (the subtraction is v_add_f64 with a negated operand)
    assert "v_fma_f64" not in body
    _no_spills(body, meta)
    # rel, red, the flags (1024 x 20 bytes) and the per-wave argmax slots live in LDS
    assert 20 * 1024 <= _meta_int(meta, "group_segment_fixed_size") <= 24 * 1024
    assert not re.search(r"\bs_(atomic|buffer_atomic)", body)


def test_pairwise_rounds_every_multiply_and_add_separately(device_asm):
    # the exact kernels' rule: no v_fma_f64 in the accumulation; the score's correctly rounded sqrt and division are expanded
    # by the compiler WITH v_fma_f64, so everything in front of the first v_rsq_f64 / v_rcp_f64 must be free of it
    for frag in ("14k_mmr_pairwiseILi0E", "14k_mmr_pairwiseILi1E", "14k_mmr_pairwiseILi3E"):
        body, meta = _kernel(device_asm, frag)
        assert "v_mul_f64" in body and "v_add_f64" in body
        first_fma = body.find("v_fma_f64")
        assert first_fma == -1 or "v_rsq_f64" in body[:first_fma] or "v_rcp_f64" in body[:first_fma], frag
        _no_spills(body, meta)
    body, meta = _kernel(device_asm, "14k_mmr_pairwiseILi2E")  # Manhattan: |x - y| summed, no multiply to contract
    assert "v_add_f64" in body and "v_rcp_f64" in body and "v_fma_f64" not in body[:body.find("v_rcp_f64")]
    _no_spills(body, meta)


def test_kernel_names_do_not_capture_the_existing_isa_checks(device_asm):
    names = re.findall(r"^(_Z\S*):", device_asm, flags=re.M)
    kernels = [n for n in names if "k_" in n]
    assert kernels and all("k_mmr_" in n for n in kernels), kernels
    for frag in ("k_exact_scan", "k_scan", "k_range_rescore"):
        assert not any(frag in n for n in kernels)

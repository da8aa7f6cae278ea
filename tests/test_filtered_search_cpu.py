"""CPU-side checks of the id-filtered search (vl_index_filter_* / vl_index_search_filtered): the symbols, the argument checks
that need no device, and the gfx950 ISA of the subset kernels (cross-compiled here).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vl_index_filter_create", "vl_index_filter_rows", "vl_index_filter_destroy", "vl_index_search_filtered",
       "vl_index_search_batch_filtered"]
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
    out = tmp_path_factory.mktemp("isa_subset") / "kernels.s"
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
        "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, "kernels.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def _kernel_body(asm, mangled_fragment):
    m = re.search(r"^(_Z\S*%s\S*):[^\n]*\n(.*?)s_endpgm" % re.escape(mangled_fragment), asm, flags=re.S | re.M)
    assert m, mangled_fragment
    return m.group(2)


def test_new_symbols_are_declared_and_exported(lib):
    from vectorlite_amd import _lib
    header = open(os.path.join(ROOT, "include", "vectorlite_amd.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS


def test_argument_checks_need_no_device(lib):
    tok, rows, n = C.c_uint64(0), C.c_uint64(0), C.c_uint64(7)
    ids = (C.c_uint64 * 2)(1, 2)
    q = (C.c_double * 4)(0, 0, 0, 0)
    out_ids = (C.c_uint64 * 4)()
    out_sc = (C.c_double * 4)()
    null = None
    assert lib.vl_index_filter_create(null, ids, 2, C.byref(tok), C.byref(rows)) == VL_ERR_INVALID_ARG
    assert lib.vl_index_filter_rows(null, 1, C.byref(rows)) == VL_ERR_INVALID_ARG
    assert lib.vl_index_filter_destroy(null, 1) == VL_ERR_INVALID_ARG
    assert lib.vl_index_search_filtered(null, 1, C.cast(q, C.c_void_p), 4, 2, 0, 4, C.cast(out_ids, C.c_void_p),
                                        C.cast(out_sc, C.c_void_p), C.cast(C.pointer(n), C.c_void_p)) == VL_ERR_INVALID_ARG
    assert lib.vl_index_search_filtered(null, 1, C.cast(q, C.c_void_p), 4, 2, 0, 4, C.cast(out_ids, C.c_void_p),
                                        C.cast(out_sc, C.c_void_p), None) == VL_ERR_INVALID_ARG
    assert lib.vl_index_search_batch_filtered(null, 1, q, 1, 4, 2, 0, 4, out_ids, out_sc,
                                              C.cast(C.pointer(n), C.POINTER(C.c_uint64))) == VL_ERR_INVALID_ARG
    # a handle that cannot exist without a device is refused before anything touches one; token 0 is never a filter
    assert lib.vl_index_filter_rows(null, 0, C.byref(rows)) == VL_ERR_INVALID_ARG


def test_every_subset_scan_instantiation_is_compiled(device_asm):
    names = set(re.findall(r"^(_Z\S*k_scan_subset\S*):", device_asm, flags=re.M))
    # (G, VPL, U) default shapes of the specialised strides: kernel-argument query up to 768 floats, f64 query beyond
    qarg = [(8, 4, 3), (8, 8, 2), (8, 12, 1), (8, 16, 1), (16, 12, 1)]
    q64 = [(16, 16, 1), (16, 24, 1)]
    for metric in range(4):
        for g, vpl, u in qarg:
            frag = "13k_scan_subsetILi%dELi%dELi%dELi%dE" % (metric, g, vpl, u)
            assert any(frag in n for n in names), frag
        for g, vpl, u in q64:
            frag = "17k_scan_subset_q64ILi%dELi%dELi%dELi%dE" % (metric, g, vpl, u)
            assert any(frag in n for n in names), frag
        for g in (1, 2, 4, 8, 16, 32, 64):
            frag = "21k_scan_subset_genericILi%dELi%dE" % (metric, g)
            assert any(frag in n for n in names), frag
    for frag in ("14k_filter_count", "13k_filter_scan", "16k_filter_compact"):
        assert re.search(r"^_Z\S*%s\S*:" % frag, device_asm, flags=re.M), frag


def test_subset_scan_streams_rows_with_16_byte_nontemporal_loads(device_asm):
    frag = "13k_scan_subsetILi0ELi8ELi12ELi1E"  # cosine, dim 384
    body = _kernel_body(device_asm, frag)
    lines = body.splitlines()
    nt = [i for i, l in enumerate(lines) if re.search(r"global_load_dwordx4 .* nt", l)]
    assert len(nt) == 12  # one row group: 12 float4 per lane
    first_fma = min(i for i, l in enumerate(lines) if re.search(r"\bv_(pk_)?fmac?_f32", l))
    assert nt[-1] < first_fma  # all of them in flight before the arithmetic starts
    assert "scratch_" not in body and "buffer_store" not in body
    meta = re.search(r"\.name:\s+_ZN2vl12_GLOBAL__N_1%s.*?\.vgpr_count:\s+(\d+)" % frag, device_asm, re.S)
    assert meta and int(meta.group(1)) <= 128


def test_subset_exact_scan_does_not_contract_multiply_add(device_asm):
    for frag in ("19k_exact_scan_subsetILi0E", "19k_exact_scan_subsetILi1E", "19k_exact_scan_subsetILi3E"):
        body = _kernel_body(device_asm, frag)
        assert "v_mul_f64" in body and "v_add_f64" in body
        first_fma = body.find("v_fma_f64")
        assert first_fma == -1 or "v_rsq_f64" in body[:first_fma] or "v_rcp_f64" in body[:first_fma], frag


def test_new_kernels_do_not_capture_the_existing_isa_checks(device_asm):
    # the fragments tests/test_isa_checks.py looks up still name exactly one kernel each
    for frag in ("12k_exact_scanILi0E", "12k_exact_scanILi1E", "12k_exact_scanILi3E", "6k_scanILi0ELi8ELi12ELi1E"):
        hits = re.findall(r"^(_Z\S*%s\S*):" % re.escape(frag), device_asm, flags=re.M)
        assert len(hits) == 1, (frag, hits)
    names = re.findall(r"\.name:\s+(_ZN2vl12_GLOBAL__N_16k_scanILi0ELi8ELi12ELi1E\S*)", device_asm)
    assert len(set(names)) == 1

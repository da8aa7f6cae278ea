"""CPU-side checks of the grouped search (vl_index_groups_* / vl_index_search_grouped): the symbols, the argument checks that
need no device, and the gfx950 ISA of its pass-1 scan (kernels.hip, cross-compiled here).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VL_ERR_INVALID_ARG = 8
NAMES = ("vl_index_groups_create", "vl_index_groups_rows", "vl_index_groups_destroy", "vl_index_search_grouped")


@pytest.fixture(scope="module")
def lib():
    from vectorlite_amd import build
    build.build()
    from vectorlite_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_grouped") / "kernels.s"
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
        "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, "kernels.hip"), "-o", str(out)]
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


def test_symbols_are_declared_exported_and_listed(lib):
    from vectorlite_amd import _lib
    header = open(os.path.join(ROOT, "include", "vectorlite_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name


def test_the_limit_is_1024():
    import vectorlite_amd as V
    header = open(os.path.join(ROOT, "include", "vectorlite_amd.h")).read()
    assert re.search(r"#define\s+VL_GROUPED_MAX_K\s+1024\b", header)
    assert V.VL_GROUPED_MAX_K == 1024


def test_argument_checks_need_no_device(lib):
    q = (C.c_double * 4)(1, 0, 0, 0)
    keys = (C.c_uint64 * 8)()
    ids = (C.c_uint64 * 8)()
    sc = (C.c_double * 8)()

    def search(groups, k, h=None, n_ptr=True):
        n = C.c_uint64(7)
        rc = lib.vl_index_search_grouped(h, groups, 0, C.cast(q, C.c_void_p), 4, k, 0, 8, C.cast(keys, C.c_void_p),
                                         C.cast(ids, C.c_void_p), C.cast(sc, C.c_void_p), C.byref(n) if n_ptr else None)
        return rc, n.value, lib.vl_last_error().decode()

    rc, n, msg = search(5, 1025)  # answered before the handle is looked at: its own message, *out_n = 0
    assert rc == VL_ERR_INVALID_ARG and n == 0 and "VL_GROUPED_MAX_K" in msg
    rc, n, msg = search(0, 4)     # token 0 is never a table
    assert rc == VL_ERR_INVALID_ARG and n == 0 and "group table" in msg
    rc, n, _ = search(5, 4)       # a null handle
    assert rc == VL_ERR_INVALID_ARG and n == 0
    rc, n, _ = search(5, 1024)    # the limit itself passes the argument check: still the null handle
    assert rc == VL_ERR_INVALID_ARG and n == 0
    assert search(5, 4, n_ptr=False)[0] == VL_ERR_INVALID_ARG

    out = C.c_uint64(9)
    assert lib.vl_index_groups_rows(None, 5, C.byref(out), None) == VL_ERR_INVALID_ARG
    assert lib.vl_index_groups_destroy(None, 5) == VL_ERR_INVALID_ARG


def test_a_conflicting_table_is_rejected_on_the_host(lib):
    tok, rows = C.c_uint64(9), C.c_uint64(0)
    ids = (C.c_uint64 * 4)(11, 12, 11, 13)
    bad = (C.c_uint64 * 4)(1, 2, 3, 2)       # id 11 with keys 1 and 3
    good = (C.c_uint64 * 4)(1, 2, 1, 2)      # id 11 twice with key 1
    # no handle at all: the pairs are judged first, with their own message
    rc = lib.vl_index_groups_create(None, ids, bad, 4, C.byref(tok), C.byref(rows))
    assert rc == VL_ERR_INVALID_ARG and tok.value == 0
    assert "id 11" in lib.vl_last_error().decode() and "two different group keys" in lib.vl_last_error().decode()
    rc = lib.vl_index_groups_create(None, ids, good, 4, C.byref(tok), C.byref(rows))
    assert rc == VL_ERR_INVALID_ARG and tok.value == 0  # the null handle, not the pairs
    assert lib.vl_index_groups_create(None, ids, good, 4, None, None) == VL_ERR_INVALID_ARG


DIM384 = "ILi0ELi8ELi12ELi1ELb%dEE"  # cosine, the default shape for dim = 384; whole index / listed rows


@pytest.mark.parametrize("subset", [0, 1])
def test_group_best_scan_streams_like_k_scan_and_raises_with_a_64_bit_max(device_asm, subset):
    body, meta = _kernel(device_asm, "17k_scan_group_best" + DIM384 % subset)
    assert len(re.findall(r"global_load_dwordx4 .* nt", body)) == 12  # the row loads of k_scan
    assert "scratch_" not in body and "buffer_store" not in body     # no spills, no scratch
    assert _meta_int(meta, "private_segment_fixed_size") == 0
    assert not re.search(r"\.(vgpr|sgpr)_spill_count:\s+[1-9]", meta)
    assert _meta_int(meta, "group_segment_fixed_size") == 0          # no LDS list, no block merge
    assert "global_atomic_umax_x2" in body                            # the hardware's 64-bit max ...
    assert "cmpswap" not in body                                      # ... and no compare-and-swap loop in its place


def test_every_form_of_the_group_best_scan_is_clean(device_asm):
    names = re.findall(r"^(_Z\S*k_scan_group_best\S*):", device_asm, flags=re.M)
    forms = {"17k_scan_group_bestIL": 0, "21k_scan_group_best_q64IL": 0, "25k_scan_group_best_genericIL": 0}
    for name in names:
        for frag in forms:
            if frag in name:
                forms[frag] += 1
        body, meta = _kernel(device_asm, name[2:])
        assert "scratch_" not in body and _meta_int(meta, "private_segment_fixed_size") == 0, name
        assert _meta_int(meta, "group_segment_fixed_size") == 0, name
        assert "global_atomic_umax_x2" in body and "cmpswap" not in body, name
    assert all(forms.values()), forms  # the kernel-argument form, the q64 form, the run-time-stride form

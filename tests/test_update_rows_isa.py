"""Static checks on the gfx950 ISA of the in-place update's kernels (CPU only, cross-compiles of kernels.hip and
mfma_scan.hip): k_update_rows and k_update_copies use no scratch, the master row is written in 16-byte stores, and the four
converters whose row bodies the update kernels share -- k_ingest, k_rows_bf16, k_rows_bf16_frag, k_rows_i8 -- keep the
registers, scratch and LDS they had before their bodies became functions.

The constants below were read from the code-object metadata (.vgpr_count, .agpr_count, .sgpr_count,
.private_segment_fixed_size, .group_segment_fixed_size) of the same cross-compile (hipcc --offload-arch=gfx950 with the
build's flags, --cuda-device-only -S) of the commit before the update kernels were added."""
import os
import re
import subprocess

import pytest

# kernel -> (vgpr, agpr, sgpr, scratch bytes, LDS bytes) before the row bodies were factored out
BEFORE = {
    "8k_ingestE": (32, 0, 56, 0, 0),
    "11k_rows_bf16E": (30, 0, 42, 0, 0),
    "16k_rows_bf16_fragE": (50, 0, 49, 0, 0),
    "9k_rows_i8E": (56, 0, 52, 0, 0),
}


def _asm(tmp_path_factory, source):
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_update") / (source + ".s")
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
        "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, source), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


@pytest.fixture(scope="module")
def kernels_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "kernels.hip")


@pytest.fixture(scope="module")
def mfma_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "mfma_scan.hip")


def _kernel(asm, mangled_fragment):
    m = re.search(r"^(_Z\S*%s\S*):[^\n]*\n(.*?)s_endpgm" % re.escape(mangled_fragment), asm, flags=re.S | re.M)
    assert m, mangled_fragment
    name = m.group(1)
    meta = [b for b in asm.split("- .agpr_count:")[1:] if re.search(r"\.name:\s+%s\s" % re.escape(name), b)]
    assert len(meta) == 1, name
    return m.group(2), meta[0]


def _meta_int(meta, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def _resources(meta):
    return (_meta_int(meta, "vgpr_count"), int(meta.split()[0]), _meta_int(meta, "sgpr_count"),
            _meta_int(meta, "private_segment_fixed_size"), _meta_int(meta, "group_segment_fixed_size"))


def test_update_rows_kernel_has_no_scratch_and_writes_the_master_row_16_bytes_at_a_time(kernels_asm):
    body, meta = _kernel(kernels_asm, "13k_update_rowsILi16EE")
    assert "scratch_" not in body
    assert _meta_int(meta, "private_segment_fixed_size") == 0 and _meta_int(meta, "group_segment_fixed_size") == 0
    assert re.search(r"\bglobal_load_dwordx4\b", body)
    assert re.search(r"\bglobal_store_dwordx4\b", body)
    body, meta = _kernel(kernels_asm, "13k_update_rowsILi8EE")  # odd dims: 8-byte copies, nothing spilled either
    assert "scratch_" not in body and _meta_int(meta, "private_segment_fixed_size") == 0


def test_update_copies_kernels_have_no_scratch_and_stay_at_their_converters_level(mfma_asm):
    converter = {"0": "11k_rows_bf16E", "1": "16k_rows_bf16_fragE", "2": "9k_rows_i8E"}
    for copy, conv in converter.items():
        body, meta = _kernel(mfma_asm, "15k_update_copiesILi%sEE" % copy)
        assert "scratch_" not in body
        assert _meta_int(meta, "private_segment_fixed_size") == 0 and _meta_int(meta, "group_segment_fixed_size") == 0
        # the same row body plus one position load: a few registers around the converter's, not another class of kernel
        assert _meta_int(meta, "vgpr_count") <= BEFORE[conv][0] + 8, (copy, _meta_int(meta, "vgpr_count"))
    body, _ = _kernel(mfma_asm, "15k_update_copiesILi1EE")
    assert re.search(r"\bglobal_store_dwordx4\b", body)  # a fragment-major row is its own 16-byte pieces


def test_the_four_converters_keep_their_registers_scratch_and_lds(kernels_asm, mfma_asm):
    got = {"8k_ingestE": _resources(_kernel(kernels_asm, "8k_ingestE")[1])}
    for frag in ("11k_rows_bf16E", "16k_rows_bf16_fragE", "9k_rows_i8E"):
        got[frag] = _resources(_kernel(mfma_asm, frag)[1])
    assert got == BEFORE

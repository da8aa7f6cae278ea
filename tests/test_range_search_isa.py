"""Static checks on the gfx950 ISA of the range search's kernels (CPU only, cross-compile of kernels.hip)."""
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_range") / "kernels.s"
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


@pytest.mark.parametrize("subset", [0, 1])
def test_range_scan_streams_like_k_scan_and_appends_with_one_atomic(device_asm, subset):
    # the default shape for dim = 384, whole index and filter forms
    body, meta = _kernel(device_asm, "12k_scan_rangeILi0ELi8ELi12ELi1ELb%dEE" % subset)
    nt = re.findall(r"global_load_dwordx4 .* nt", body)
    assert len(nt) == 12  # 12 float4 per lane (one row group of 8 rows) in flight, as in k_scan
    assert "scratch_" not in body and "buffer_store" not in body  # no spills
    assert _meta_int(meta, "private_segment_fixed_size") == 0
    assert _meta_int(meta, "group_segment_fixed_size") == 0       # no LDS top list, no block merge
    assert not re.search(r"\bds_(read|write|load|store)", body)
    assert _meta_int(meta, "vgpr_count") <= 128
    # one vector atomic add reserves a wave's slots; nothing atomic per row
    assert len(re.findall(r"\bglobal_atomic_add\b", body)) == 1
    assert len(re.findall(r"\b(global|flat|buffer)_atomic", body)) == 1
    loop = body[body.index("Loop Header"):]
    assert len(re.findall(r"\bglobal_atomic_add\b", loop)) == 1
    assert not re.search(r"\bs_(atomic|buffer_atomic)", body)


def test_range_rescore_rounds_every_multiply_and_add_separately(device_asm):
    # the reference's f64 loops are separate multiply and add: no v_fma_f64 in the accumulation.  The score's correctly
    # rounded sqrt and division are expanded by the compiler WITH v_fma_f64 (that is how they are correctly rounded), so
    # "no v_fma_f64" is asserted for everything in front of the first v_rsq_f64 / v_rcp_f64: the rule of the exact kernels
    for frag in ("15k_range_rescoreILi0E", "15k_range_rescoreILi1E", "15k_range_rescoreILi3E"):
        body, _ = _kernel(device_asm, frag)
        assert "v_mul_f64" in body and "v_add_f64" in body
        first_fma = body.find("v_fma_f64")
        assert first_fma == -1 or "v_rsq_f64" in body[:first_fma] or "v_rcp_f64" in body[:first_fma], frag
    body, _ = _kernel(device_asm, "15k_range_rescoreILi2E")  # Manhattan: |x - y| summed, no multiply to contract
    assert "v_add_f64" in body and "v_fma_f64" not in body[:body.find("v_rcp_f64")]

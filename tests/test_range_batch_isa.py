"""Static checks on the gfx950 ISA of the batched range search's kernels (CPU only, cross-compiles of kernels.hip and
mfma_scan.hip)."""
import os
import re
import subprocess

import pytest


def _asm(tmp_path_factory, source):
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_range_batch") / (source + ".s")
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


def test_rescore_rounds_every_multiply_and_add_separately(kernels_asm):
    # the reference's f64 loops are separate multiply and add: no v_fma_f64 in the accumulation.  The score's correctly
    # rounded sqrt and division are expanded by the compiler WITH v_fma_f64, so "no v_fma_f64" is asserted for everything
    # in front of the first v_rsq_f64 / v_rcp_f64: the rule of the exact kernels (tests/test_range_search_isa.py)
    for metric in (0, 1, 3):
        body, meta = _kernel(kernels_asm, "20k_rbatch_rescore_cutILi%dE" % metric)
        assert "v_mul_f64" in body and "v_add_f64" in body
        first_fma = body.find("v_fma_f64")
        assert first_fma == -1 or "v_rsq_f64" in body[:first_fma] or "v_rcp_f64" in body[:first_fma], metric
        assert "scratch_" not in body and _meta_int(meta, "private_segment_fixed_size") == 0  # no spills
        assert len(re.findall(r"\bglobal_atomic_add\b", body)) == 1  # one reservation per tile of candidates
        assert not re.search(r"\bs_(atomic|buffer_atomic)", body)


def test_rank_and_offsets_fit_their_workgroups(kernels_asm):
    body, meta = _kernel(kernels_asm, "18k_rbatch_rank_emit")
    assert _meta_int(meta, "private_segment_fixed_size") == 0 and "scratch_" not in body
    assert _meta_int(meta, "group_segment_fixed_size") == 2 * 2048 * 8  # keys and payloads of one query's 2048 survivors
    assert "v_fma_f64" not in body  # desc_key's `s + 0.0` is an add; scores leave as their own bits
    body, meta = _kernel(kernels_asm, "16k_rbatch_offsets")
    assert _meta_int(meta, "private_segment_fixed_size") == 0 and "scratch_" not in body


def test_the_pass_needs_no_k_mfma_rows_mode_of_its_own(mfma_asm):
    """The batch launches pass 1 (MODE 1) of k_mfma_rows as the top-k batch ships it: no range-only MODE exists."""
    modes = set(re.findall(r"^_ZN2vl\S*11k_mfma_rowsILi\d+ELi(\d+)E", mfma_asm, flags=re.M))
    assert modes == {"0", "1"}, modes

"""Static checks on the gfx950 code objects of the id-filtered HNSW walks, k_hnsw_search_filt and k_hnsw_search_ref_filt
(hnsw.hip; CPU only, cross-compile): every instantiation the launcher can pick exists, and the sorted list -- three
registers per entry and lane, up to eight entries per lane -- stays in registers.  Resource facts only."""
import os
import re
import subprocess

import pytest

KERNELS = ("k_hnsw_search_filt", "k_hnsw_search_ref_filt")
METRICS = (0, 1, 2, 3)
SLOTS = (1, 2, 4, 8)
# scratch bytes per lane of the S = 8 instantiations as the build shows them, both kernels, all metrics
S8_SCRATCH = 0


@pytest.fixture(scope="module")
def hnsw_asm(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_hnsw_filt") / "hnsw.s"
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
        "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, "hnsw.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def _frag(kernel, metric, s):
    return "%d%sILi%dELi%dEE" % (len(kernel), kernel, metric, s)


def _meta(asm, frag, key):
    for block in asm.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if frag in name:
            return int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
    raise AssertionError(frag)


def test_every_filtered_instantiation_exists(hnsw_asm):
    for kernel in KERNELS:
        for metric in METRICS:
            for s in SLOTS:
                assert re.search(r"^_Z\S*%s\S*:" % re.escape(_frag(kernel, metric, s)), hnsw_asm, flags=re.M), (kernel, metric, s)
    assert re.search(r"^_Z\S*18k_hnsw_filter_bits\S*:", hnsw_asm, flags=re.M)


def test_no_scratch_below_eight_slots_and_eight_pinned(hnsw_asm):
    for kernel in KERNELS:
        for metric in METRICS:
            for s in SLOTS:
                scratch = _meta(hnsw_asm, _frag(kernel, metric, s), "private_segment_fixed_size")
                assert scratch == (S8_SCRATCH if s == 8 else 0), (kernel, metric, s, scratch)


def test_no_register_spills_and_two_waves_per_simd(hnsw_asm):
    """256 threads per workgroup = one wave per SIMD; 256 VGPRs or fewer leave room for a second workgroup's wave."""
    for kernel in KERNELS:
        for metric in METRICS:
            for s in SLOTS:
                frag = _frag(kernel, metric, s)
                assert _meta(hnsw_asm, frag, "vgpr_spill_count") == 0, (kernel, metric, s)
                assert _meta(hnsw_asm, frag, "vgpr_count") <= 256, (kernel, metric, s)

"""Static checks on the gfx950 ISA of k_scan_subset_jobs, the scan of a filtered batch (CPU only, cross-compile of
kernels.hip).  The yardstick is k_scan_subset of the same shape from the same compile: the jobs kernel must stream as
many non-temporal 16-byte loads per step, keep everything in registers, and allow as many waves per SIMD."""
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_subset_jobs") / "kernels.s"
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


def _waves_per_simd(vgprs):
    """Waves per SIMD the unified 512-entry register file allows: registers are allocated in granules of 8."""
    alloc = max(8, (vgprs + 7) // 8 * 8)
    return min(8, 512 // alloc)


# (G, VPL, U) of the default shapes for dim = 384 (96 float4 per row) and dim = 768 (192)
@pytest.mark.parametrize("g,vpl,u", [(8, 12, 1), (16, 12, 1)])
def test_jobs_scan_streams_like_the_lone_subset_scan(device_asm, g, vpl, u):
    shape = "ILi0ELi%dELi%dELi%dEE" % (g, vpl, u)  # cosine
    jobs_body, jobs_meta = _kernel(device_asm, "18k_scan_subset_jobs" + shape)
    lone_body, lone_meta = _kernel(device_asm, "13k_scan_subset" + shape)
    assert _meta_int(jobs_meta, "private_segment_fixed_size") == 0  # nothing spilled
    nt_jobs = len(re.findall(r"global_load_dwordx4 .* nt", jobs_body))
    nt_lone = len(re.findall(r"global_load_dwordx4 .* nt", lone_body))
    assert nt_lone == vpl * u  # the yardstick is what it is believed to be
    assert nt_jobs == nt_lone
    jobs_waves = _waves_per_simd(_meta_int(jobs_meta, "vgpr_count") + _meta_int("- .agpr_count:" + jobs_meta, "agpr_count"))
    lone_waves = _waves_per_simd(_meta_int(lone_meta, "vgpr_count") + _meta_int("- .agpr_count:" + lone_meta, "agpr_count"))
    assert jobs_waves >= lone_waves, (jobs_waves, lone_waves)

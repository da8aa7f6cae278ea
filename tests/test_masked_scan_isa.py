"""Static checks on the gfx950 ISA of the three masked scans of an exclusion filter (k_scan_masked, k_scan_bf16_masked,
k_scan_i8_masked; CPU only, cross-compiles of kernels.hip and mfma_scan.hip).  The yardstick is the unmasked kernel of
the same shape from the same compile: the masked one must keep everything in registers, stream as many non-temporal
16-byte loads per step, and need at most 2 U more VGPRs -- one keep word and one flag per row group in flight, what a
vector-load implementation of the bitmap read would take (the scalar read the kernels use takes none)."""
import os
import re
import subprocess

import pytest


def _device_asm(tmp_path_factory, source):
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_masked") / (source + ".s")
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
        "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, source), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


@pytest.fixture(scope="module")
def kernels_asm(tmp_path_factory):
    return _device_asm(tmp_path_factory, "kernels.hip")


@pytest.fixture(scope="module")
def mfma_asm(tmp_path_factory):
    return _device_asm(tmp_path_factory, "mfma_scan.hip")


def _kernel(asm, mangled_fragment):
    m = re.search(r"^(_Z\S*%s\S*):[^\n]*\n(.*?)s_endpgm" % re.escape(mangled_fragment), asm, flags=re.S | re.M)
    assert m, mangled_fragment
    name = m.group(1)
    meta = [b for b in asm.split("- .agpr_count:")[1:] if re.search(r"\.name:\s+%s\s" % re.escape(name), b)]
    assert len(meta) == 1, name
    return m.group(2), meta[0]


def _meta_int(meta, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def _vgprs(meta):
    return _meta_int(meta, "vgpr_count") + _meta_int("- .agpr_count:" + meta, "agpr_count")


def _check(asm, masked_name, plain_name, g, vpl, u):
    shape = "ILi0ELi%dELi%dELi%dEE" % (g, vpl, u)  # cosine
    masked_body, masked_meta = _kernel(asm, masked_name + shape)
    plain_body, plain_meta = _kernel(asm, plain_name + shape)
    assert _meta_int(masked_meta, "private_segment_fixed_size") == 0  # nothing spilled
    nt_masked = len(re.findall(r"global_load_dwordx4 .* nt", masked_body))
    nt_plain = len(re.findall(r"global_load_dwordx4 .* nt", plain_body))
    assert nt_plain == vpl * u  # the yardstick is what it is believed to be
    assert nt_masked == nt_plain
    print("%s%s: %d VGPRs, unmasked %d" % (masked_name, shape, _vgprs(masked_meta), _vgprs(plain_meta)))
    assert _vgprs(masked_meta) <= _vgprs(plain_meta) + 2 * u, (_vgprs(masked_meta), _vgprs(plain_meta))


# (G, VPL, U) of the default shapes for dim = 384 and dim = 768 of each stage
@pytest.mark.parametrize("g,vpl,u", [(8, 12, 1), (16, 12, 1)])
def test_masked_f32_scan_streams_like_k_scan(kernels_asm, g, vpl, u):
    _check(kernels_asm, "13k_scan_masked", "6k_scan", g, vpl, u)


@pytest.mark.parametrize("g,vpl,u", [(8, 6, 1), (16, 6, 1)])
def test_masked_bf16_scan_streams_like_k_scan_bf16_qarg(mfma_asm, g, vpl, u):
    _check(mfma_asm, "18k_scan_bf16_masked", "16k_scan_bf16_qarg", g, vpl, u)


@pytest.mark.parametrize("g,vpl,u", [(8, 3, 1), (8, 6, 1)])
def test_masked_i8_scan_streams_like_k_scan_i8_qarg(mfma_asm, g, vpl, u):
    _check(mfma_asm, "16k_scan_i8_masked", "14k_scan_i8_qarg", g, vpl, u)

"""Static checks on the gfx950 ISA of k_mfma_rows_masked, the mask-aware forms of the row-stationary batch filter (CPU only:
one cross-compile of mfma_scan.hip).  The yardstick is k_mfma_rows of the same shape from the same compile -- the two share
one body (rs_rows_body), and the mask must cost the masked kernels nothing where it matters:

  * exactly the 45 shipped shapes have a masked form (5 strides x 3 metrics x {sampling, pass 1, pass 1 streaming});
  * every one fits the 256 registers two waves per SIMD leave, and needs no more scratch than its unmasked twin;
  * pass 1 issues exactly the unmasked kernel's MFMAs: the mask added nothing to the matrix stream."""
import os
import re
import subprocess

import pytest

KSTEPS = (8, 16, 24, 32, 48)
METRICS = (0, 1, 3)  # cosine, Euclidean, dot


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(masked, ksteps, mode, metric, stream): (body, metadata)} of every k_mfma_rows / k_mfma_rows_masked in the default build"""
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_masked_mfma") / "mfma.s"
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
        "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, "mfma_scan.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    asm = out.read_text()
    meta = {}
    for block in asm.split("- .agpr_count:")[1:]:
        meta[re.search(r"\.name:\s+(\S+)", block).group(1)] = "- .agpr_count:" + block
    found = {}
    for m in re.finditer(r"^(_Z\S*?(11k_mfma_rows|18k_mfma_rows_masked)I\S*):[^\n]*\n(.*?)s_endpgm", asm, flags=re.S | re.M):
        name, which, body = m.group(1), m.group(2), m.group(3)
        if which.startswith("18"):
            a = re.search(r"k_mfma_rows_maskedILi(\d+)ELi(\d)ELi(\d)ELb([01])E", name)
            key = (True, int(a.group(1)), int(a.group(2)), int(a.group(3)), a.group(4) == "1")
        else:
            a = re.search(r"k_mfma_rowsILi(\d+)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELb([01])E", name)
            assert (a.group(4), a.group(5)) == ("2", "8"), name  # the default build holds the shipped shape only
            key = (False, int(a.group(1)), int(a.group(2)), int(a.group(3)), a.group(6) == "1")
        assert key not in found, name
        found[key] = (body, meta[name])
    return found


def _int(meta, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def _shapes():
    return [(ks, mode, met, stream) for ks in KSTEPS for met in METRICS for (mode, stream) in ((0, False), (1, False), (1, True))]


def test_exactly_the_shipped_shapes_have_a_masked_form(kernels):
    masked = sorted(k[1:] for k in kernels if k[0])
    assert len(masked) == 45
    assert masked == sorted(_shapes())
    assert not [k for k in masked if k[1] == 0 and k[3]]  # the sampling pass never streams
    assert sorted(k[1:] for k in kernels if not k[0]) == masked  # and the unmasked kernel still ships the same 45


@pytest.mark.parametrize("ks,mode,met,stream", _shapes())
def test_masked_kernel_costs_no_more_than_its_twin(kernels, ks, mode, met, stream):
    body, meta = kernels[(True, ks, mode, met, stream)]
    plain_body, plain_meta = kernels[(False, ks, mode, met, stream)]
    vgprs = _int(meta, "vgpr_count") + _int(meta, "agpr_count")
    scratch, plain_scratch = _int(meta, "private_segment_fixed_size"), _int(plain_meta, "private_segment_fixed_size")
    mfma = len(re.findall(r"^\s*v_mfma_", body, flags=re.M))
    plain_mfma = len(re.findall(r"^\s*v_mfma_", plain_body, flags=re.M))
    print("k_mfma_rows_masked<%d, %d, %d, %d>: %d VGPRs, scratch %d (unmasked %d), %d MFMAs (unmasked %d)"
          % (ks, mode, met, stream, vgprs, scratch, plain_scratch, mfma, plain_mfma))
    assert vgprs <= 256
    assert scratch <= plain_scratch
    assert plain_mfma > 0  # the yardstick is what it is believed to be
    if mode == 1:
        assert mfma == plain_mfma

"""Static checks on the gfx950 ISA of the bulk delete's row-move kernel (CPU only, cross-compile of kernels.hip): no scratch,
and rows move in 16-byte global loads and stores."""
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_move") / "kernels.s"
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


def test_row_move_kernel_uses_no_scratch_and_moves_16_bytes_per_lane(device_asm):
    body, meta = _kernel(device_asm, "11k_move_rowsILi16EE")
    assert "scratch_" not in body
    assert _meta_int(meta, "private_segment_fixed_size") == 0
    assert re.search(r"\bglobal_load_dwordx4\b", body)
    assert re.search(r"\bglobal_store_dwordx4\b", body)
    for frag in ("11k_move_rowsILi8EE", "11k_move_rowsILi4EE", "11k_move_rowsILi1EE"):  # the narrower paths spill nothing either
        body, meta = _kernel(device_asm, frag)
        assert "scratch_" not in body and _meta_int(meta, "private_segment_fixed_size") == 0

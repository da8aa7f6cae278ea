"""The int8 single-query filter on the CPU: VL_SINGLE_FILTER=i8 parsing and the ladder's rules (csrc/single_filter.hpp,
compiled with g++ under AddressSanitizer + UBSan), the Python name of mode 3, and the gfx950 ISA of k_scan_i8_qarg."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_single_filter_i8_parsing_and_ladder(tmp_path):
    exe = tmp_path / "single_filter_i8_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "single_filter_i8_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "passed single_filter i8 checks" in r.stdout


def test_python_i8_mode_maps_to_3():
    import vectorlite_amd as V

    class FakeLib:
        def __init__(self):
            self.seen = []

        def vl_index_set_single_filter(self, h, mode):
            self.seen.append(mode)
            return 0

    idx = object.__new__(V.FlatIndex)  # no device: only the argument mapping is under test
    idx._L, idx._h = FakeLib(), None
    for name in ("i8", "auto", "f32", "bf16"):
        idx.set_single_filter(name)
    assert idx._L.seen == [3, 2, 0, 1]
    with pytest.raises(KeyError):
        idx.set_single_filter("int8")


@pytest.fixture(scope="module")
def mfma_asm(tmp_path_factory):
    """mfma_scan.hip's device assembly (two minutes of hipcc)."""
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_i8") / "mfma.s"
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
        "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, "mfma_scan.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def _body(asm, frag):
    m = re.search(r"^(_ZN\S*" + re.escape(frag) + r"\S*):[^\n]*\n(.*?)\.Lfunc_end", asm, re.S | re.M)
    assert m, frag
    return m.group(1), m.group(2)


# (G, VPL, U) of every listed shape: VL_I8_SCAN_SHAPES in mfma_scan.hip
SHAPES = [(8, 1, 1), (8, 2, 1), (8, 3, 1), (8, 4, 1), (8, 6, 1), (4, 2, 1), (4, 4, 1), (4, 6, 1), (4, 8, 1), (8, 3, 2),
          (4, 6, 2), (2, 12, 1), (8, 6, 2), (4, 12, 1), (16, 3, 1)]


@pytest.mark.parametrize("metric", [0, 3])
def test_i8_scan_streams_16_byte_nontemporal_loads_and_dots_f16_pairs(mfma_asm, metric):
    """Every listed shape: VPL * U 16-byte non-temporal row loads per lane and iteration, no scratch, and the chosen
    arithmetic: per 16 bytes, 8 v_perm_b32 (bytes -> f16 pairs), 8 packed f16 subtracts and 8 f16 pair dots."""
    for g, vpl, u in SHAPES:
        name, body = _body(mfma_asm, f"14k_scan_i8_qargILi{metric}ELi{g}ELi{vpl}ELi{u}E")
        nt = re.findall(r"global_load_dwordx4 [^\n]* nt", body)
        assert len(nt) == vpl * u, (name, len(nt))
        assert "scratch_" not in body, name
        assert len(re.findall(r"\bv_perm_b32\b", body)) == 8 * vpl * u, name
        assert len(re.findall(r"\bv_pk_add_f16\b", body)) == 8 * vpl * u, name
        assert len(re.findall(r"\bv_dot2c?_f32_f16", body)) == 8 * vpl * u, name
        assert "v_cvt_f32_i32" not in body and "v_bfe_i32" not in body, name  # no per-byte widening
        meta = re.search(re.escape(name) + r"\.private_seg_size, (\d+)", mfma_asm)
        if meta:
            assert int(meta.group(1)) == 0, name

"""Static checks on the gfx950 ISA of the reference-navigated walk, k_hnsw_search_ref (hnsw.hip; CPU only,
cross-compile).  Every evaluation of that walk must be the reference's f64 arithmetic: separate multiply and add,
no contraction, one lane per row."""
import os
import re
import subprocess

import pytest

KERNEL = "k_hnsw_search_ref"
METRICS = (0, 1, 2, 3)
SLOTS = (1, 2, 4, 8)
# scratch bytes per lane of the S = 8 instantiations as the build shows them (the beam is 3 x 8 registers per lane)
S8_SCRATCH = 0


@pytest.fixture(scope="module")
def hnsw_asm(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    out = tmp_path_factory.mktemp("isa_hnsw") / "hnsw.s"
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"] + vbuild.COMMON + [
        "--cuda-device-only", "-S", os.path.join(vbuild.CSRC, "hnsw.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def _frag(metric, s):
    return "%d%sILi%dELi%dE" % (len(KERNEL), KERNEL, metric, s)


def _body(asm, frag):
    m = re.search(r"^(_Z\S*%s\S*):[^\n]*\n(.*?)s_endpgm" % re.escape(frag), asm, flags=re.S | re.M)
    assert m, frag
    return m.group(2)


def _meta(asm, frag, key):
    for block in asm.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if frag in name:
            return int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
    raise AssertionError(frag)


def test_every_instantiation_exists(hnsw_asm):
    for metric in METRICS:
        for s in SLOTS:
            _body(hnsw_asm, _frag(metric, s))


def test_accumulation_is_separate_multiply_and_add(hnsw_asm):
    for metric in METRICS:
        for s in SLOTS:
            body = _body(hnsw_asm, _frag(metric, s))
            assert "v_add_f64" in body, (metric, s)
            if metric != 2:  # Manhattan accumulates |x - y|: adds only (its `* 1000.0` is a multiply all the same)
                assert "v_mul_f64" in body, (metric, s)
            first_fma = body.find("v_fma_f64")
            # v_fma_f64 only inside the correctly rounded sqrt / division expansions (rsq / rcp first)
            assert first_fma == -1 or "v_rsq_f64" in body[:first_fma] or "v_rcp_f64" in body[:first_fma], (metric, s)


def test_no_scratch_below_eight_slots_and_eight_pinned(hnsw_asm):
    for metric in METRICS:
        for s in SLOTS:
            frag = _frag(metric, s)
            scratch = _meta(hnsw_asm, frag, "private_segment_fixed_size")
            if s < 8:
                assert scratch == 0, (metric, s, scratch)
                assert "scratch_" not in _body(hnsw_asm, frag), (metric, s)
            else:
                assert scratch == S8_SCRATCH, (metric, s, scratch)

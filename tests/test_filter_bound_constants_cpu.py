"""The in_extra terms of the bf16 filters' exactness bound are named once (mfma_scan.hpp) and the library passes those
names, so the value the filter audit (tests/test_gpu_filter_audit.py) checks is the value the library ships."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorlite_amd", "csrc")


def test_flat_index_passes_the_named_in_extra_constants():
    hpp = open(os.path.join(CSRC, "mfma_scan.hpp")).read()
    assert re.search(r"constexpr double IN_EXTRA_BF16_SINGLE = [0-9.]+;", hpp)
    assert re.search(r"constexpr double IN_EXTRA_MFMA = [0-9.]+;", hpp)
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "flat_index.cpp")).read())  # code only, any layout
    calls = [m.group(0) for m in re.finditer(r"launch_merge_finalize\s*\([^;]*;", src)]
    bf16 = [c for c in calls if "IN_EXTRA_BF16_SINGLE" in c]
    assert len(bf16) == 1 and re.search(r",\s*IN_EXTRA_BF16_SINGLE\s*\)\s*\)\s*;$", bf16[0]), bf16
    assert re.search(r"\bconst\s+double\s+in_extra\s*=\s*IN_EXTRA_MFMA\s*;", src)
    # no other value of in_extra anywhere: no literal, no arithmetic on the constants
    assert not re.search(r"\bin_extra\s*=(?![=\s]*IN_EXTRA_MFMA\s*;)", src)
    assert not re.search(r"IN_EXTRA_\w+\s*[*/+-]|[*/+-]\s*IN_EXTRA_", src)
    assert not re.search(r"\b0\.00392\b|\b0\.0079\b", src)

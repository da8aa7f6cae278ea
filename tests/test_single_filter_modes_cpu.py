"""The single-query filter modes on the CPU: VL_SINGLE_FILTER parsing and the auto mode's window / probe rule
(csrc/single_filter.hpp, compiled with g++ under AddressSanitizer + UBSan), and the Python names of the modes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_single_filter_parsing_and_auto_window(tmp_path):
    exe = tmp_path / "single_filter_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "single_filter_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "passed single_filter checks" in r.stdout


def test_python_modes_map_to_the_c_values():
    import vectorlite_amd as V
    assert V.SINGLE_FILTER_MODES == {"f32": 0, "bf16": 1, "auto": 2}

    class FakeLib:
        def __init__(self):
            self.seen = []

        def vl_index_set_single_filter(self, h, mode):
            self.seen.append(mode)
            return 0

    idx = object.__new__(V.FlatIndex)  # no device: only the argument mapping is under test
    idx._L, idx._h = FakeLib(), None
    for name in ("f32", "bf16", "auto"):
        idx.set_single_filter(name)
    assert idx._L.seen == [0, 1, 2]
    with pytest.raises(KeyError):
        idx.set_single_filter("fp8")

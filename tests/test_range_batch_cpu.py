"""The batched range search on the CPU: the key threshold it hands the MFMA filter (csrc/score_bound.hpp,
range_key_threshold with the bf16 in_extra) against the host build of the shipped bound_for_key, and the surfaces every
binding has to carry."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_threshold_is_the_smallest_key_not_provably_out(tmp_path):
    exe = tmp_path / "range_batch_threshold_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "range_batch_threshold_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "range batch thresholds ok" in r.stdout


def test_the_test_and_the_library_use_the_same_in_extra():
    hpp = open(os.path.join(ROOT, "vectorlite_amd", "csrc", "mfma_scan.hpp")).read()
    cpp = open(os.path.join(ROOT, "tests", "native", "range_batch_threshold_test.cpp")).read()
    lib = re.search(r"constexpr double IN_EXTRA_MFMA = ([0-9.e-]+);", hpp).group(1)
    test = re.search(r"constexpr double IN_EXTRA = ([0-9.e-]+);", cpp).group(1)
    assert float(lib) == float(test)


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vectorlite_amd.h")).read()
    from vectorlite_amd import _lib
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "index", "gpu.rs")).read()
    for sym in ("vl_index_search_range_batch", "vl_index_last_range_batch", "vl_index_last_range_batch_candidates"):
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in _lib.SYMBOLS, sym
        assert re.search(r"\bfn %s\(" % sym, rust), sym
    import vectorlite_amd as V
    for cls in (V.FlatIndex, V.MultiFlatIndex, V.HNSWIndex):
        assert callable(getattr(cls, "search_range_batch_arrays")) and callable(getattr(cls, "search_range_batch"))
    assert callable(V.FlatIndex.last_range_batch)

"""CPU tests of the check / canonicalise gate's host side: the declarations of sapca_check_csr_device_* and
sapca_canonicalize_csr_device_* in include/sapca.h, the layout of sapca_csr_report against its ctypes mirror, the flag
values, the Python methods, and the numpy reference the GPU tests compare with (tests/canonical_ref.py).  The exports, the
sys crate and the C++ mirror are held to the header by tests/test_abi_cpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch  # noqa: F401  (first: one HIP runtime per process)

import canonical_ref as R
from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sapca.h")


def _args_of(name):
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"sapca_status\s+%s\s*\(([^()]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_header_declares_both_pairs():
    for suf, ct in (("f32", "float"), ("f64", "double")):
        csr = ["sapca_handle h", "uint64_t m", "uint64_t n", "uint64_t nnz", "const int64_t* row_offsets",
               "const int32_t* col_indices", f"const {ct}* values"]
        assert _args_of(f"sapca_check_csr_device_{suf}") == csr + ["sapca_csr_report* report"]
        assert _args_of(f"sapca_canonicalize_csr_device_{suf}") == csr + [
            "uint64_t* nnz_out", "const int64_t** d_row_offsets", "const int32_t** d_col_indices", f"{ct}** d_values",
            "sapca_csr_report* report"]
        for name in (f"sapca_check_csr_device_{suf}", f"sapca_canonicalize_csr_device_{suf}"):
            assert name in L.EXPORTED_SYMBOLS and hasattr(L.load(), name)
    text = open(HEADER).read()
    assert re.search(r"#define\s+SAPCA_ABI_VERSION\s+4\b", text)
    assert "additive, ABI 4: sapca_check_csr_device_*, sapca_canonicalize_csr_device_*" in text


def test_the_flag_values_are_the_headers():
    text = open(HEADER).read()
    got = {n: int(v) for n, v in re.findall(r"^#define\s+SAPCA_CSR_(\w+)\s+(\d+)u\b", text, flags=re.M)}
    assert got == {"BAD_OFFSETS": 1, "COL_RANGE": 2, "UNSORTED": 4, "DUPLICATES": 8, "NONFINITE": 16}
    assert (L.CSR_BAD_OFFSETS, L.CSR_COL_RANGE, L.CSR_UNSORTED, L.CSR_DUPLICATES, L.CSR_NONFINITE) == (1, 2, 4, 8, 16)
    assert {v: k for k, v in L.CSR_FLAG_NAMES.items()} == got


def test_the_report_struct_layout_matches_a_compiled_probe(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    fields = [f[0] for f in L.CsrReport._fields_]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "%s"\nint main() {\n  std::printf("%%zu\\n", sizeof(sapca_csr_report));\n%s  return 0;\n}\n'
                   % (HEADER, "".join('  std::printf("%s %%zu\\n", offsetof(sapca_csr_report, %s));\n' % (f, f) for f in fields)))
    exe = tmp_path / "probe"
    r = subprocess.run([cxx, "-std=c++17", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(L.CsrReport) == 88
    got = dict((ln.split()[0], int(ln.split()[1])) for ln in out[1:] if ln.strip())
    assert got == {f: getattr(L.CsrReport, f).offset for f in fields}
    # the header's field order is the mirror's
    hdr = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+sapca_csr_report\s*\{(.*?)\}", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", body) == fields


def test_the_python_methods_exist_and_the_report_decodes():
    for name in ("check", "canonicalize", "from_torch"):
        assert callable(getattr(ops.ResidentCsr, name))
    raw = L.CsrReport()
    for f, _ in L.CsrReport._fields_:
        if f.startswith("first_"):
            setattr(raw, f, 2 ** 64 - 1)
    rep = ops.CsrReport(raw)
    assert rep.canonical and rep.flags == () and rep.bits == 0 and rep.first_unsorted_row is None and rep.unsorted_rows == 0
    raw.flags = L.CSR_UNSORTED | L.CSR_NONFINITE
    raw.unsorted_rows, raw.first_unsorted_row = 2, 7
    rep = ops.CsrReport(raw)
    assert not rep.canonical and rep.flags == ("UNSORTED", "NONFINITE") and (rep.unsorted_rows, rep.first_unsorted_row) == (2, 7)
    raw.flags = L.CSR_NONFINITE
    assert ops.CsrReport(raw).canonical                       # non-finite values are reported, not a defect of the structure


def test_the_reference_on_the_example_of_its_docstring():
    ptr, idx, val = R.canonicalize([0, 4, 4, 6], np.array([3, 1, 3, 0, 4, 4], np.int32), np.array([1, 2, 4, 8, 0.5, 0.25], np.float32))
    assert ptr.tolist() == [0, 3, 3, 4] and ptr.dtype == np.int64
    assert idx.tolist() == [0, 1, 3, 4] and idx.dtype == np.int32
    assert val.tolist() == [8.0, 2.0, 5.0, 0.75] and val.dtype == np.float32


def test_the_reference_sums_left_to_right_in_the_dtype_and_keeps_bit_patterns():
    # (1e8 + 1) + -1e8 in f32 is 0; 1e8 + (-1e8 + 1) would be 1: stored order decides
    ptr, idx, val = R.canonicalize([0, 3], np.array([2, 2, 2], np.int32), np.array([1e8, 1.0, -1e8], np.float32))
    assert idx.tolist() == [2] and val.tolist() == [0.0]
    v = np.array([0.0, -0.0, 1.0], np.float32)
    v.view(np.uint32)[2] = 0x7FC00123                          # a NaN with a payload
    ptr, idx, val = R.canonicalize([0, 3], np.array([5, 3, 1], np.int32), v)
    assert idx.tolist() == [1, 3, 5] and val.view(np.uint32).tolist() == [0x7FC00123, 0x80000000, 0]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_reference_agrees_with_scipy_where_sums_are_exact(dt):
    rng = np.random.default_rng(5)
    m, n, nnz = 40, 30, 900
    lens = rng.multinomial(nnz, np.ones(m) / m)
    lens[3] = 0
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, n, int(ptr[-1])).astype(np.int32)    # unsorted, many duplicates
    val = rng.integers(-8, 9, idx.size).astype(dt)             # small integers: every sum is exact
    got = R.canonicalize(ptr, idx, val)
    A = sp.csr_matrix((val.copy(), idx.copy(), ptr.copy()), shape=(m, n))
    A.sum_duplicates()
    A.sort_indices()
    np.testing.assert_array_equal(got[0], A.indptr)
    np.testing.assert_array_equal(got[1], A.indices)
    np.testing.assert_array_equal(got[2], A.data)
    assert got[2].dtype == dt and got[0][-1] < idx.size

"""CPU tests of the row selection's host side: the argument handling of ResidentCsr.select_rows (ops._row_list, pure numpy)
and the declarations of sapca_select_rows_csr_device_* in include/sapca.h.  The exports, the sys crate and the C++ mirror
are held to the header by tests/test_abi_cpu.py."""
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_mask_becomes_ascending_indices():
    mask = np.array([False, True, True, False, True, False, False, True])
    r = ops._row_list(mask, 8)
    assert r.dtype == np.uint64 and r.flags.c_contiguous
    assert r.tolist() == [1, 2, 4, 7]
    assert ops._row_list([True, False, True], 3).tolist() == [0, 2]          # a list of bools is a mask too
    assert ops._row_list(np.zeros(5, bool), 5).size == 0
    assert ops._row_list(np.ones(5, bool), 5).tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("length", [0, 7, 9])
def test_a_mask_of_the_wrong_length_raises(length):
    with pytest.raises(ValueError, match=rf"Row mask length \({length}\) does not match number of rows \(8\)"):
        ops._row_list(np.ones(length, bool), 8)


def test_a_negative_index_raises():
    with pytest.raises(ValueError, match="negative row index -1 at position 2"):
        ops._row_list([3, 0, -1, 2], 8)
    with pytest.raises(ValueError, match="negative row index -5 at position 0"):
        ops._row_list(np.array([-5], dtype=np.int32), 8)


def test_an_integer_list_passes_through_as_uint64():
    r = ops._row_list([5, 0, 5, 3], 8)                                        # order and repeats are the caller's
    assert r.dtype == np.uint64 and r.flags.c_contiguous and r.tolist() == [5, 0, 5, 3]
    for dt in (np.int32, np.int64, np.uint8, np.uint64):
        r = ops._row_list(np.array([7, 1, 1], dtype=dt), 8)
        assert r.dtype == np.uint64 and r.tolist() == [7, 1, 1]
    assert ops._row_list(np.arange(10)[::3], 10).tolist() == [0, 3, 6, 9]     # a strided view is made contiguous
    assert ops._row_list(np.array([8, 100]), 8).tolist() == [8, 100]          # too large: the library's to refuse, with its message
    e = ops._row_list([], 8)
    assert e.dtype == np.uint64 and e.size == 0


def test_what_is_neither_a_mask_nor_indices_raises():
    with pytest.raises(ValueError, match="boolean mask or integer indices"):
        ops._row_list([0.0, 1.0], 8)
    with pytest.raises(ValueError, match="one-dimensional"):
        ops._row_list(np.zeros((2, 2), dtype=np.int64), 8)


def test_the_header_declares_both_functions():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sapca.h")).read(), flags=re.S)
    for suf, ct in (("f32", "float"), ("f64", "double")):
        m = re.search(r"sapca_status\s+sapca_select_rows_csr_device_%s\s*\(([^()]*)\)\s*;" % suf, text)
        assert m, f"sapca_select_rows_csr_device_{suf} is not declared"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == ["sapca_handle h", "uint64_t m", "uint64_t n", "uint64_t nnz", "const int64_t* row_offsets",
                        "const int32_t* col_indices", f"const {ct}* values", "const uint64_t* rows", "uint64_t n_rows",
                        "uint64_t* nnz_out", "const int64_t** d_row_offsets", "const int32_t** d_col_indices", f"{ct}** d_values"]
        assert f"sapca_select_rows_csr_device_{suf}" in L.EXPORTED_SYMBOLS
        assert hasattr(L.load(), f"sapca_select_rows_csr_device_{suf}")
    assert re.search(r"#define\s+SAPCA_ABI_VERSION\s+4\b", text)
    assert "additive, ABI 4: sapca_select_rows_csr_device_*" in open(os.path.join(ROOT, "include", "sapca.h")).read()


def test_the_python_method_exists():
    assert callable(getattr(ops.ResidentCsr, "select_rows"))

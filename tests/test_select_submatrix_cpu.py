"""CPU tests of the row-and-column selection's host side: ops._col_mask (pure numpy), the numpy reference of the GPU tests
(tests/submatrix_ref.py) against scipy, and the declarations of sapca_select_submatrix_csr_device_* in include/sapca.h.
The sys crate and the C++ mirror are held to the header by tests/test_abi_cpu.py."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch  # noqa: F401  (first: one HIP runtime per process)

import submatrix_ref as SR
from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


# ------------------------------------------------------------------ _col_mask
def test_a_mask_passes_through():
    mask = np.array([False, True, True, False, True])
    got = ops._col_mask(mask, 5)
    assert got.dtype == np.uint8 and got.flags.c_contiguous and got.tolist() == [0, 1, 1, 0, 1]
    assert ops._col_mask([True, False], 2).tolist() == [1, 0]                 # a list of bools is a mask too
    assert ops._col_mask(np.ones(70, bool)[::2], 35).flags.c_contiguous       # a strided view is made contiguous


@pytest.mark.parametrize("length", [0, 4, 6])
def test_a_mask_of_the_wrong_length_raises(length):
    with pytest.raises(ValueError, match=rf"Column mask length \({length}\) does not match number of columns \(5\)"):
        ops._col_mask(np.ones(length, bool), 5)


def test_ascending_indices_become_a_mask():
    for dt in (np.int32, np.int64, np.uint8, np.uint64):
        got = ops._col_mask(np.array([0, 3, 4], dtype=dt), 6)
        assert got.dtype == np.uint8 and got.tolist() == [1, 0, 0, 1, 1, 0]
    assert ops._col_mask([5], 6).tolist() == [0, 0, 0, 0, 0, 1]
    assert ops._col_mask(np.arange(6), 6).tolist() == [1] * 6


def test_an_empty_index_list_is_an_all_false_mask():
    got = ops._col_mask([], 4)
    assert got.dtype == np.uint8 and got.tolist() == [0, 0, 0, 0]
    assert ops._col_mask(np.zeros(0, np.int64), 4).tolist() == [0, 0, 0, 0]


def test_repeated_descending_negative_and_float_indices_raise():
    with pytest.raises(ValueError, match="strictly ascending: 2 at position 2 follows 2"):
        ops._col_mask([1, 2, 2, 3], 6)
    with pytest.raises(ValueError, match="strictly ascending: 1 at position 1 follows 4"):
        ops._col_mask([4, 1], 6)
    with pytest.raises(ValueError, match="negative column index -1 at position 1"):
        ops._col_mask([0, -1, 2], 6)
    with pytest.raises(ValueError, match="boolean mask or integer indices"):
        ops._col_mask([0.0, 1.0], 6)
    with pytest.raises(ValueError, match="out of range"):
        ops._col_mask([0, 6], 6)
    with pytest.raises(ValueError, match="one-dimensional"):
        ops._col_mask(np.zeros((2, 2), bool), 4)


# ------------------------------------------------------------------ the reference of the GPU tests against scipy
def _small_mixed(dt):
    """7 x 9: stored zeros of both signs, a NaN with a payload, an empty row 2, an empty column 4, unsorted nowhere"""
    bits = BITS[np.dtype(dt)]
    ptr = np.array([0, 3, 6, 6, 10, 11, 14, 16], np.int64)
    idx = np.array([0, 2, 8, 1, 2, 3, 0, 3, 5, 7, 6, 1, 5, 8, 2, 7], np.int32)
    val = np.array([1.5, 0.0, -2.0, 3.0, -0.0, 4.0, 5.0, np.nan, 0.0, 6.0, np.inf, 7.0, -8.0, 0.0, 9.0, -0.0], dt)
    val.view(bits)[7] = bits(0x7FC00123) if dt == np.float32 else bits(0x7FF8000000000123)
    return ptr, idx, val, 7, 9


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_reference_agrees_with_scipy(dt):
    ptr, idx, val, m, n = _small_mixed(dt)
    bits = BITS[np.dtype(dt)]
    A = sp.csr_matrix((val, idx, ptr), shape=(m, n))
    assert A.nnz == val.size                                                     # (scipy kept the stored zeros)
    rng = np.random.default_rng(0)
    row_cases = [None, np.arange(m), np.array([6, 2, 2, 0, 3, 3]), np.zeros(0, np.int64), rng.integers(0, m, 20)]
    mask_cases = [None, np.ones(n, bool), np.zeros(n, bool), np.arange(n) == 4, np.arange(n) % 2 == 0, rng.random(n) < 0.5]
    for rows in row_cases:
        for mask in mask_cases:
            for drop in (False, True):
                off, ci, v, nc = SR.select_submatrix(ptr, idx, val, n, rows, mask, drop)
                want = A if rows is None else (A[rows] if len(rows) else sp.csr_matrix((0, n), dtype=dt))
                if mask is not None:
                    want = want[:, np.flatnonzero(mask)]
                want = sp.csr_matrix(want, copy=True)                            # (eliminate_zeros works in place)
                if drop:
                    want.eliminate_zeros()
                assert nc == want.shape[1] and off.dtype == np.int64 and ci.dtype == np.int32 and v.dtype == np.dtype(dt)
                np.testing.assert_array_equal(off, want.indptr)
                np.testing.assert_array_equal(ci, want.indices)
                np.testing.assert_array_equal(v.view(bits), np.ascontiguousarray(want.data).view(bits))
    off, ci, v, nc = SR.select_submatrix(ptr, idx, val, n, None, None, True)
    assert v.size == val.size - 5 and np.isnan(v).sum() == 1                     # five zeros of either sign go, the NaN stays


# ------------------------------------------------------------------ the declarations
def test_the_header_declares_both_functions_and_the_flag():
    raw = open(os.path.join(ROOT, "include", "sapca.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    for suf, ct in (("f32", "float"), ("f64", "double")):
        m = re.search(r"sapca_status\s+sapca_select_submatrix_csr_device_%s\s*\(([^()]*)\)\s*;" % suf, text)
        assert m, f"sapca_select_submatrix_csr_device_{suf} is not declared"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == ["sapca_handle h", "uint64_t m", "uint64_t n", "uint64_t nnz", "const int64_t* row_offsets",
                        "const int32_t* col_indices", f"const {ct}* values", "const uint64_t* rows", "uint64_t n_rows",
                        "const uint8_t* col_mask", "uint64_t mask_len", "uint32_t flags", "uint64_t* n_cols_out",
                        "uint64_t* nnz_out", "const int64_t** d_row_offsets", "const int32_t** d_col_indices", f"{ct}** d_values"]
    assert re.search(r"#define\s+SAPCA_SELECT_DROP_STORED_ZEROS\s+1u\b", text)
    assert re.search(r"#define\s+SAPCA_ABI_VERSION\s+4\b", text)
    assert "additive, ABI 4: sapca_select_submatrix_csr_device_*" in raw


def test_the_library_exports_both_functions():
    for suf in ("f32", "f64"):
        assert f"sapca_select_submatrix_csr_device_{suf}" in L.EXPORTED_SYMBOLS
        assert hasattr(L.load(), f"sapca_select_submatrix_csr_device_{suf}")
    assert L.SELECT_DROP_STORED_ZEROS == 1


def test_the_python_methods_exist():
    assert callable(getattr(ops.ResidentCsr, "select"))
    assert callable(getattr(ops.ResidentCsr, "select_cols"))

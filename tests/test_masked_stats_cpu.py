"""Masked and chunk statistics (MatrixNonZero / MatrixSum / MatrixVariance *_masked and *_chunk, MatrixMinMax *_chunk;
csr.rs:124-252, 394-556, 728-1008): the numpy restatement against literal transliterations of the reference loops, the
Python wrapper's argument checks, the C++ mirror's new members, and the library's exports.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch  # noqa: F401  (first: one HIP runtime per process)

import masked_stats_ref as M
from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_csr(m, n, density, seed):
    """stored explicit zeros, negative values, an empty row and an empty column"""
    rng = np.random.default_rng(seed)
    D = (rng.random((m, n)) < density) * rng.normal(1.0, 3.0, (m, n))
    stored = (D != 0) | (rng.random((m, n)) < 0.05)
    stored[2, :] = False
    stored[:, 1] = False
    r, c = np.nonzero(stored)
    A = sp.csr_matrix((D[r, c], (r, c)), shape=(m, n))
    A.sort_indices()
    assert (A.data == 0).any() and (A.data < 0).any()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data


def _masks(k, rng):
    return {
        "random": rng.random(k) < 0.6,
        "all_true": np.ones(k, bool),
        "all_false": np.zeros(k, bool),
        "longer_false_tail": np.concatenate([rng.random(k) < 0.5, np.zeros(4, bool)]),
    }


def _close(got, want, what):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=1e-12, atol=1e-12, err_msg=what)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_masked_restatement_matches_the_reference_loops(seed):
    m, n = 21, 13
    ptr, idx, val = _random_csr(m, n, 0.4, seed)
    rng = np.random.default_rng(50 + seed)
    for kind, cm in _masks(m, rng).items():       # column statistics: a mask over the rows
        for name in ("nonzero_col_masked", "sum_col_masked", "var_col_masked"):
            _close(getattr(M, name)(ptr, idx, val, m, n, cm), getattr(M, "ref_" + name)(ptr, idx, val, m, n, list(cm)), f"{name} {kind}")
    for kind, rm in _masks(n, rng).items():       # row statistics: a mask over the columns
        for name in ("nonzero_row_masked", "sum_row_masked", "var_row_masked"):
            _close(getattr(M, name)(ptr, idx, val, m, n, rm), getattr(M, "ref_" + name)(ptr, idx, val, m, n, list(rm)), f"{name} {kind}")
    assert not M.sum_col_masked(ptr, idx, val, m, n, np.zeros(m, bool)).any()


def _chunk_refs(name, m, n, rng):
    """initial reference arrays for a chunk method: shorter, exact and longer where the reference accepts them"""
    if name in ("nonzero_col_chunk", "nonzero_row_chunk"):
        k = n if "col" in name else m
        return [rng.integers(0, 9, L_).astype(np.uint64) for L_ in (k - 3, k, k + 2)]
    if name == "sum_col_chunk":
        return [rng.normal(size=L_) for L_ in (n - 3, n, n + 2)]
    if name == "sum_row_chunk":
        return [rng.normal(size=L_) for L_ in (m, m + 2)]
    if name in ("var_col_chunk", "var_row_chunk"):
        return [rng.normal(size=n if "col" in name else m)]
    k = n if "col" in name else m
    return [(rng.normal(0, 2, k), rng.normal(0, 2, k)), (np.full(k, np.inf), np.full(k, -np.inf))]


def _copy(r):
    return tuple(a.copy() for a in r) if isinstance(r, tuple) else r.copy()


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", M.CHUNK)
def test_chunk_restatement_matches_the_reference_loops(name, seed):
    m, n = 19, 14
    ptr, idx, val = _random_csr(m, n, 0.45, 10 + seed)
    rng = np.random.default_rng(seed)
    for ref in _chunk_refs(name, m, n, rng):
        got = getattr(M, name)(ptr, idx, val, m, n, _copy(ref))
        want = getattr(M, "ref_" + name)(ptr, idx, val, m, n, _copy(ref))
        for g, w in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
            if g.dtype.kind == "u":
                np.testing.assert_array_equal(g, w, err_msg=name)
            else:
                _close(g, w, name)


def test_no_mask_is_the_stored_entry_variance_of_the_chunk_family():
    m, n = 17, 9
    ptr, idx, val = _random_csr(m, n, 0.5, 7)
    _close(M.masked_stats(ptr, idx, val, m, n, M.COLUMN)[3], M.ref_var_col_chunk(ptr, idx, val, m, n, [0.0] * n), "col")
    _close(M.masked_stats(ptr, idx, val, m, n, M.ROW)[3], M.ref_var_row_chunk(ptr, idx, val, m, n, [0.0] * m), "row")
    _close(M.masked_stats(ptr, idx, val, m, n, M.ROW, np.ones(n + 3, bool))[3], M.masked_stats(ptr, idx, val, m, n, M.ROW)[3], "tail")


def test_wrapper_checks_before_any_library_call():
    R = ops.ResidentCsr(None, (4, 3), 0, np.float32, 0, 0, 0)   # these checks come before any library call
    for fn, k, msg in ((R.nonzero_col_masked, 3, "Mask length (3) is less than number of rows (4)"),
                       (R.sum_col_masked, 0, "Mask length (0) is less than number of rows (4)"),
                       (R.var_col_masked, 2, "Mask length (2) is less than number of rows (4)"),
                       (R.nonzero_row_masked, 2, "Mask length (2) is less than number of columns (3)"),
                       (R.sum_row_masked, 1, "Mask length (1) is less than number of columns (3)"),
                       (R.var_row_masked, 2, "Mask length (2) is less than number of columns (3)")):
        with pytest.raises(ValueError) as e:
            fn([True] * k)
        assert str(e.value) == msg
    for fn, k, msg in ((R.var_col_chunk, 4, "Reference slice length 4 does not match number of columns 3"),
                       (R.var_col_chunk, 2, "Reference slice length 2 does not match number of columns 3"),
                       (R.var_row_chunk, 3, "Reference slice length 3 does not match number of rows 4")):
        with pytest.raises(ValueError) as e:
            fn(np.zeros(k))
        assert str(e.value) == msg
    with pytest.raises(ValueError, match="less than number of rows 4"):
        R.sum_row_chunk(np.zeros(3))


def test_library_exports_the_masked_statistics_entry_points():
    lib = L.load()
    for suf in ("f32", "f64"):
        name = f"sapca_masked_stats_csr_device_{suf}"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.EXPORTED_SYMBOLS
    assert lib.sapca_abi_version() == 4                 # additive: the ABI version stays


def test_cpp_mirror_masked_and_chunk_members_instantiate():
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    hpp = os.path.join(ROOT, "single-algebra_amd", "host", "cpp", "sapca.hpp")
    src = ('#include "%s"\n'
           'template <typename T> void use(sapca::ResidentCsr<T>& r) {\n'
           '  std::vector<bool> mk{true, false};\n'
           '  std::vector<uint64_t> a = r.nonzero_col_masked(mk), b = r.nonzero_row_masked(mk);\n'
           '  std::vector<double> c = r.sum_col_masked(mk), d = r.sum_row_masked(mk), e = r.var_col_masked(mk), f = r.var_row_masked(mk);\n'
           '  std::vector<uint32_t> u(3); r.nonzero_col_chunk(u); r.nonzero_row_chunk(u);\n'
           '  std::vector<float> x(3), y(3); r.sum_col_chunk(x); r.sum_row_chunk(x); r.var_col_chunk(x); r.var_row_chunk(y);\n'
           '  r.min_max_col_chunk(x, y); r.min_max_row_chunk(x, y); (void)a; (void)b; (void)c; (void)d; (void)e; (void)f; }\n'
           'template void use<float>(sapca::ResidentCsr<float>&);\ntemplate void use<double>(sapca::ResidentCsr<double>&);\n'
           'int main() { return 0; }\n' % hpp)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

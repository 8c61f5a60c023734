"""Per-batch means / variances and top-n row sums (BatchMatrixVariance, BatchMatrixMean, MatrixNTop; csr.rs:1081-1376):
the numpy restatement against literal transliterations of the reference loops, the Python wrapper's label handling and
messages, the C++ mirror's new members, and the library's exports.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch  # noqa: F401  (first: one HIP runtime per process)

import batch_stats_ref as B
from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_csr(m, n, density, seed, integer=False):
    """with stored explicit zeros, negative values, an empty row and an empty column"""
    rng = np.random.default_rng(seed)
    D = (rng.random((m, n)) < density) * (rng.integers(-5, 9, (m, n)) if integer else rng.normal(2.0, 3.0, (m, n)))
    stored = D != 0
    stored |= rng.random((m, n)) < 0.05          # explicit zeros among the stored entries
    D[1, :] = 0
    stored[1, :] = False                        # an empty row
    D[:, 2] = 0
    stored[:, 2] = False                        # an empty column
    r, c = np.nonzero(stored)
    A = sp.csr_matrix((D[r, c].astype(np.float64), (r, c)), shape=(m, n))
    A.sort_indices()
    assert (A.data == 0).any()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data, A


def _same(got, want):
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_allclose(np.asarray(got[k], np.float64), np.asarray(want[k], np.float64), rtol=1e-12, atol=1e-12)


LABELS = {
    "ints": lambda rng, k: rng.integers(0, 3, k).tolist(),
    "strings": lambda rng, k: [["ctrl", "stim", "rep-2"][j] for j in rng.integers(0, 3, k)],
    "one_row_batch": lambda rng, k: ["solo"] + ["many"] * (k - 1),   # a batch of one line: var 0
    "single": lambda rng, k: [7] * k,
}


@pytest.mark.parametrize("labels", sorted(LABELS))
@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_matches_the_reference_loops(labels, seed):
    m, n = 23, 11
    ptr, idx, val, _ = _random_csr(m, n, 0.35, seed)
    rng = np.random.default_rng(100 + seed)
    row_labels, col_labels = LABELS[labels](rng, m), LABELS[labels](rng, n)
    for axis, batches, ref_var, ref_mean in ((0, row_labels, B.ref_var_batch_row, B.ref_mean_batch_col),
                                             (1, col_labels, B.ref_var_batch_col, B.ref_mean_batch_row)):
        names, codes = B.dense_codes(batches)
        mean, var, cnt = B.batch_stats(ptr, idx, val, m, n, axis, codes, len(names))
        _same(B.to_dict(names, var), ref_var(ptr, idx, val, m, n, batches))
        _same(B.to_dict(names, mean), ref_mean(ptr, idx, val, m, n, batches))
        assert cnt.sum() == len(val)                       # every stored entry, explicit zeros included, counted once


def test_unused_codes_give_zeros_and_a_batch_of_one_has_variance_zero():
    ptr, idx, val, A = _random_csr(12, 6, 0.5, 3)
    codes = np.array([0] * 11 + [2], dtype=np.int32)        # code 1 never occurs, code 2 labels one row
    mean, var, cnt = B.batch_stats(ptr, idx, val, 12, 6, 0, codes, 4)
    assert not mean[1].any() and not var[1].any() and not cnt[1].any() and not mean[3].any()
    assert not var[2].any()
    np.testing.assert_allclose(mean[2], A.toarray()[11])


@pytest.mark.parametrize("integer", [False, True])
def test_top_n_restatement_matches_the_reference_loop(integer):
    m, n = 30, 17
    ptr, idx, val, _ = _random_csr(m, n, 0.6, 5, integer=integer)
    lens = np.diff(ptr)
    for k in (0, 1, 2, 5, int(lens.max()), int(lens.max()) + 3):
        np.testing.assert_allclose(B.sum_row_n_top(ptr, val, k), B.ref_sum_row_n_top(ptr, idx, val, m, k), rtol=1e-13, atol=1e-12)
    assert (B.sum_row_n_top(ptr, val, 0) == 0).all()


def test_wrapper_maps_labels_to_codes_in_order_of_first_appearance():
    for batches in ([3, 1, 3, 9, 1], np.array([3, 1, 3, 9, 1]), ["b", "a", "b", "z", "a"], [(1, "x"), (0, "y"), (1, "x"), 5, (0, "y")]):
        names, codes = ops._dense_codes(batches)
        want_names, want_codes = B.dense_codes(list(batches) if not isinstance(batches, np.ndarray) else batches.tolist())
        assert names == want_names and codes.tolist() == want_codes.tolist() and codes.dtype == np.int32


def test_wrapper_raises_the_reference_messages_on_a_length_mismatch():
    R = ops.ResidentCsr(None, (4, 3), 0, np.float32, 0, 0, 0)   # the length check comes before any library call
    cases = ((R.var_batch_row, 3, "Batch vector length (3) doesn't match matrix row count (4)"),
             (R.var_batch_col, 4, "Batch vector length (4) doesn't match matrix column count (3)"),
             (R.mean_batch_row, 2, "Number of batch identifiers (2) must match number of columns (3)"),
             (R.mean_batch_col, 5, "Number of batch identifiers (5) must match number of rows (4)"))
    for fn, k, msg in cases:
        with pytest.raises(ValueError) as e:
            fn(["a"] * k)
        assert str(e.value) == msg
    for bad in (-1, [], [2, -3], 1.5):
        with pytest.raises(ValueError):
            R.sum_row_n_top(bad)


def test_library_exports_the_batch_statistics_entry_points():
    lib = L.load()
    for name in ("sapca_batch_stats_csr_device", "sapca_sum_row_n_top_csr_device"):
        for suf in ("f32", "f64"):
            assert hasattr(lib, f"{name}_{suf}"), f"{name}_{suf} is not exported"
            assert f"{name}_{suf}" in L.EXPORTED_SYMBOLS
    assert lib.sapca_abi_version() == 4                 # additive: the ABI version stays


def test_cpp_mirror_batch_members_instantiate():
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    hpp = os.path.join(ROOT, "single-algebra_amd", "host", "cpp", "sapca.hpp")
    src = ('#include "%s"\n#include <string>\n'
           'template <typename T> void use(sapca::ResidentCsr<T>& r) {\n'
           '  std::unordered_map<std::string, std::vector<double>> a = r.var_batch_row(std::vector<std::string>{"x"});\n'
           '  std::unordered_map<int, std::vector<double>> b = r.var_batch_col(std::vector<int>{1});\n'
           '  auto c = r.mean_batch_row(std::vector<long>{2}); auto d = r.mean_batch_col(std::vector<std::string>{"y"});\n'
           '  std::vector<double> e = r.sum_row_n_top(50); (void)a; (void)b; (void)c; (void)d; (void)e; }\n'
           'template void use<float>(sapca::ResidentCsr<float>&);\ntemplate void use<double>(sapca::ResidentCsr<double>&);\n'
           'int main() { return 0; }\n' % hpp)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

"""CPU tests of the covariate feature's host side: sapca_covariate_basis (pure host code of the library) against the numpy
reference, the Python marshalling errors of set_covariates, and the reference's own consistency (the oracle run on the
densified residual against a dense SVD of it)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import covariates_ref as R
import sapca
import sapca_oracle as O
from sapca import _lib as L
from sapca import ops, synth


def _designs():
    rng = np.random.default_rng(11)
    m = 157
    codes = rng.integers(0, 4, m)
    depth = 1e4 * (1.0 + rng.random(m))
    return {
        "full rank": (rng.standard_normal((m, 5)), True, 6),
        "full rank, no intercept": (rng.standard_normal((m, 5)), False, 5),
        "one-hot + intercept (collinear)": (R.one_hot(codes, 4), True, 4),
        "one-hot, no intercept": (R.one_hot(codes, 4), False, 4),
        "zero column": (np.hstack([rng.standard_normal((m, 2)), np.zeros((m, 1)), rng.standard_normal((m, 1))]), True, 4),
        "repeated column": (np.repeat(rng.standard_normal((m, 2)), 2, axis=1), False, 2),
        "badly scaled": (np.hstack([R.one_hot(codes, 4), depth[:, None]]), True, 5),
        "rank 0": (np.zeros((m, 3)), False, 0),
        "sixteen design columns": (np.hstack([R.one_hot(rng.integers(0, 8, m), 8), rng.standard_normal((m, 7))]), True, 15),
        "more columns than rows": (rng.standard_normal((5, 9)), True, 5),
    }


@pytest.mark.parametrize("name", list(_designs()))
def test_basis_against_the_reference(name):
    Z, center, rank = _designs()[name]
    D = R.design(Z, center)
    Q, W, r = ops.covariate_basis(Z, center)
    Qr, rr = R.basis(D)
    assert r == rr == rank, name
    assert Q.shape == (D.shape[0], r) and W.shape == (D.shape[1], r)
    if r == 0:
        return
    assert np.abs(Q.T @ Q - np.eye(r)).max() <= 1e-13, name
    assert np.abs(Q @ Q.T - Qr @ Qr.T).max() <= 1e-12, name             # the same projector
    assert np.abs(D @ W - Q).max() <= 1e-12, name                        # Q = D W
    assert np.abs(D - Q @ (Q.T @ D)).max() <= 1e-12 * np.abs(D).max(), name   # ... which spans the design
    assert (np.abs(W).sum(axis=1) > 0).sum() == r, name                  # the basic solution: r pivot columns, zero rows elsewhere


def test_basis_padding_and_refusals():
    lib = L.load()
    rng = np.random.default_rng(3)
    z = np.ascontiguousarray(rng.standard_normal((40, 3)))
    q = np.full((40, 16), 7.0)
    w = np.full((4, 16), 7.0)
    rank = C.c_uint64(99)
    dp = C.POINTER(C.c_double)
    st = lib.sapca_covariate_basis(z.ctypes.data_as(dp), 40, 3, 1, q.ctypes.data_as(dp), w.ctypes.data_as(dp), C.byref(rank))
    assert st == L.OK and rank.value == 4
    assert not q[:, 4:].any() and not w[:, 4:].any()                     # zero padded to 16 columns
    for bad in (np.nan, np.inf):
        z2 = z.copy()
        z2[17, 1] = bad
        with pytest.raises(L.SapcaError):
            ops.covariate_basis(z2, True)
    with pytest.raises(L.SapcaError):
        ops.covariate_basis(np.zeros((20, 16)), True)                   # 17 design columns
    assert ops.covariate_basis(np.zeros((20, 16)), False)[2] == 0       # 16 are fine
    assert lib.sapca_covariate_basis(None, 5, 2, 1, q.ctypes.data_as(dp), w.ctypes.data_as(dp), C.byref(rank)) == L.ERR_ARG
    assert ops.covariate_basis(np.zeros((0, 2)), True)[2] == 0          # no rows: rank 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check: with a GPU the estimator exists (tests/test_gpu_covariates.py)")
def test_no_estimator_without_a_gpu():
    with pytest.raises(L.SapcaError, match="no HIP device"):
        sapca.SparsePCABuilder.new().build().set_covariates(np.zeros((3, 1)))


class _NoLibrary(sapca.pca._Estimator):
    """set_covariates' own checks, without a handle: they raise before any library call"""

    def __init__(self, center):
        self.center = center
        self._h = None


@pytest.mark.parametrize("center", [True, False])
def test_python_marshalling_errors(center):
    est = _NoLibrary(center)
    with pytest.raises(ValueError, match="design columns"):
        est.set_covariates(np.zeros((10, 17 - int(center))))
    with pytest.raises(ValueError, match="design columns"):
        est.set_covariates(np.zeros((10, 9)), batch=np.arange(10) % 8)
    z = np.zeros((10, 3))
    z[4, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite value at row 4, column 2"):
        est.set_covariates(z)
    with pytest.raises(ValueError, match="covariates have 10 rows, batch 9 labels"):
        est.set_covariates(np.zeros((10, 2)), batch=list("abcabcabc"))
    with pytest.raises(ValueError, match="one- or two-dimensional"):
        est.set_covariates(np.zeros((4, 2, 2)))
    est._covariates = np.zeros((10, 2))
    with pytest.raises(ValueError, match="covariates have 10 rows, the matrix 12"):
        est._covariate_check(12)
    est._covariate_check(10)


def test_batch_labels_expand_to_one_hot_columns():
    labels, codes = ops._dense_codes(["b", "a", "b", "c", "a"])
    assert labels == ["b", "a", "c"]
    np.testing.assert_array_equal(np.eye(3)[codes], [[1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 1, 0]])


CASES = {   # name: (m, n, batches, continuous covariates, center, stress, rank)
    "320x208": (320, 208, 3, 1, True, False, 4),
    "385x250": (385, 250, 0, 2, True, False, 3),
    "513x257": (513, 257, 8, 7, True, False, 15),
    "385x250 uncentred": (385, 250, 0, 2, False, False, 2),
    "320x208 stress": (320, 208, 3, 1, True, True, 4),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("masked", [False, True])
def test_reference_is_consistent_on_the_planted_cases(name, masked):
    """the oracle on the densified residual finds what a dense SVD of the residual finds; its total variance is
    |R|_F^2 / (m - 1) (center = 1) and the reference's quirk (center = 0); the rank is the design's"""
    m, n, nb, nc, center, stress, rank = CASES[name]
    seed = 4
    A, Z, _ = R.covariate_case(m, n, seed, nb, nc, centred=center, stress=stress)
    mask = synth.bernoulli_mask(n, 0.7, seed).numpy() if masked else None
    n_used = int(mask.sum()) if masked else n
    om = synth.gaussian_panel(n_used, 10, seed + 7).numpy()
    want, Q, r, Res = R.expected_fit(A.toarray(), Z, center=center, n_components=4, n_oversamples=6, n_power_iterations=2,
                                     normalizer="QR", omega=om, mask=mask)
    assert r == rank
    Ru = Res if mask is None else Res[:, mask]
    assert R.gap(Res, 4, mask) >= 2.0
    u, s, vt = np.linalg.svd(Ru, full_matrices=False)
    np.testing.assert_allclose(want.singular_values, s[:4], rtol=2e-3)     # (q = 2 power iterations at a gap of 2)
    assert O.subspace_angle(want.components, vt[:4]) < 5e-2
    if center:
        assert np.abs(Res.mean(axis=0)).max() <= 1e-9 * np.abs(A.toarray()).max()
        np.testing.assert_allclose(want.total_var, (Ru ** 2).sum() / (m - 1), rtol=1e-9)
    else:
        np.testing.assert_allclose(want.total_var, (want.singular_values ** 2).sum() / (m - 1), rtol=1e-12)
    # the implicit algorithm (uncentred sweeps, projection behind every A sweep) is the explicit one
    Qn = om.copy()
    Ad = A.toarray() if mask is None else A.toarray()[:, mask]
    for _ in range(2):
        Y = Ad @ Qn
        Qn = np.linalg.qr(Y - Q @ (Q.T @ Y))[0]
        Qn = np.linalg.qr(Ad.T @ Qn)[0]
    Y = Ad @ Qn
    Qy = np.linalg.qr(Y - Q @ (Q.T @ Y))[0]
    sv = np.linalg.svd(Ad.T @ Qy, compute_uv=False)
    np.testing.assert_allclose(sv[:4], want.singular_values, rtol=1e-10)

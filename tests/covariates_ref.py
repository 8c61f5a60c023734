"""Reference for the implicit regression on per-row covariates (sapca_set_covariates), numpy f64 on dense matrices.

The library fits R = (I - Q Q^T) A without forming it; here R IS formed and handed, as a CSR with every entry present, to the
existing oracle (oracle/sapca_oracle.py) with the same center, normaliser and injected Omega.  The oracle's centring of R is a
no-op for center = 1 (the intercept is a design column, so R's column means are zero) and its total variance is then
|R|_F^2 / (m - 1); for center = 0 nothing is centred on either side."""
import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp
import torch

import sapca_oracle as O
from sapca import synth

BATCH_SHIFTS = np.array([0.0, 3.0, -2.0, 5.0, 1.0, 4.0, 2.5, -1.0])


def design(Z, center):
    """D = [1 | Z] (center) or Z"""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim == 1:
        Z = Z[:, None]
    return np.hstack([np.ones((Z.shape[0], 1)), Z]) if center else Z


def basis(D):
    """(Q, rank): orthonormal basis of the span of D by the library's rule -- columns scaled to unit norm (zero columns
    dropped), QR with column pivoting, rank = #{j : |R_jj| > max(rows, design columns) eps |R_00|}"""
    D = np.asarray(D, dtype=np.float64)
    m, c = D.shape
    if m == 0 or c == 0:
        return np.zeros((m, 0)), 0
    nrm = np.linalg.norm(D, axis=0)
    Ds = D[:, nrm > 0] / nrm[nrm > 0]
    if Ds.shape[1] == 0:
        return np.zeros((m, 0)), 0
    Q, R, _ = sl.qr(Ds, mode="economic", pivoting=True)
    d = np.abs(np.diag(R))
    r = int((d > max(m, c) * np.finfo(np.float64).eps * d[0]).sum())
    return Q[:, :r], r


def one_hot(codes, n_batches=None):
    codes = np.asarray(codes)
    return np.eye(int(codes.max()) + 1 if n_batches is None else n_batches)[codes]


def residual(A, Q):
    """(I - Q Q^T) A, dense"""
    A = np.asarray(A, dtype=np.float64)
    return A - Q @ (Q.T @ A)


def out_of_sample_scores(A_fit, D_fit, A_new, D_new, Vt):
    """(A_new - D_new pinv(D_fit) A_fit) V^T: the new rows minus what the fit's regression predicts for them"""
    return (A_new - D_new @ (np.linalg.pinv(D_fit) @ A_fit)) @ Vt.T


def dense_csr(R):
    """R as the three CSR arrays with EVERY entry present (zeros stored)"""
    m, n = R.shape
    return np.arange(0, m * n + 1, n, dtype=np.int64), np.tile(np.arange(n, dtype=np.int64), m), np.ascontiguousarray(R, dtype=np.float64).reshape(-1)


def expected_fit(A, Z, *, center, n_components, n_oversamples, n_power_iterations, normalizer, omega, mask=None):
    """The oracle's fit of the densified residual.  A: dense m x n (all columns; `mask` keeps a subset as in a masked fit).
    Returns (FitResult, Q, rank, R) with R the full-width residual."""
    Q, r = basis(design(Z, center))
    R = residual(A, Q)
    ptr, idx, val = dense_csr(R)
    m, n = R.shape
    res = O.fit(ptr, idx, val, m, n, n_components=n_components, n_oversamples=n_oversamples, n_power_iterations=n_power_iterations,
                normalizer=normalizer, center=center, omega=omega, mask=mask)
    return res, Q, r, R


def covariate_case(m, n, seed, n_batches, n_cont, *, centred=True, stress=False, dtype=np.float64):
    """The test matrices of the covariate fits: synth.gapped_csr(m, n, 0.3, k = 4, seed) with covariate effects on the stored
    values -- row i scaled by 1 + 0.3 tanh(c_i0), plus a per-batch shift -- batch codes and c ~ N(0, 1) from
    default_rng(seed + 100).  stress: columns 5, 77, 150 overwritten by fully stored 1000 + 0.01 N(0, 1).
    Returns (scipy CSR in f64, Z) with Z = [one-hot of the batches | c] (no one-hot columns for n_batches = 0)."""
    ptr, idx, val = (x.numpy() for x in synth.gapped_csr(m, n, 0.3, 4, seed=seed, centred=centred, dtype=torch.float64))
    rng = np.random.default_rng(seed + 100)
    codes = rng.integers(0, max(n_batches, 1), m)
    c = rng.standard_normal((m, max(n_cont, 1)))
    rows = np.repeat(np.arange(m), np.diff(ptr))
    val = val * (1.0 + 0.3 * np.tanh(c[rows, 0]))
    if n_batches:
        val = val + BATCH_SHIFTS[codes[rows]]
    A = sp.csr_matrix((val, idx.astype(np.int64), ptr), shape=(m, n))
    if stress:
        D = A.toarray()
        stored = A.copy()
        stored.data[:] = 1.0
        S = stored.toarray() > 0
        for j in (5, 77, 150):
            D[:, j] = 1000.0 + 0.01 * rng.standard_normal(m)
            S[:, j] = True
        r_, c_ = np.nonzero(S)
        A = sp.csr_matrix((D[r_, c_], (r_, c_)), shape=(m, n))
    A.sort_indices()
    parts = ([one_hot(codes, n_batches)] if n_batches else []) + ([c[:, :n_cont]] if n_cont else [])
    return A.astype(dtype), np.hstack(parts), codes


def gap(R, k, mask=None):
    """sigma_k / sigma_{k+1} of the dense operator the fit sees"""
    sv = np.linalg.svd(R if mask is None else R[:, mask], compute_uv=False)
    return float(sv[k - 1] / sv[k])

"""The driver of SVDMethod.Lanczos (lanczos_fit, csrc/lanczos.hip) on spectra that are hard for a single-vector Lanczos run
(-m gpu): flat, complete, tiny, rank-deficient, empty, too slow for the iteration cap, repeated and clustered.  The matrices are
those of tests/lanczos_spectra_cases.py (tests/test_lanczos_spectra_cases_cpu.py holds them to what they are for); the reference
is numpy's svd of the dense f64 operator (masked columns dropped, column means subtracted for a centred fit).

Accepted triplets are checked one by one, not by subspace angle (ill-conditioned on a flat spectrum).  With kappa = 1e-5, steps =
timings().lanczos_steps, s the exact singular values, and q_i = s_1 / sigma_i on the wide side (where the iteration runs on
A A^T and v_i = A^T u_i / sigma_i carries u_i's residual times |A| / sigma_i), q_i = 1 on the tall side:
  value     |sigma_i - s_i| <= 1e-5 s_i in f64 (kappa bounds the Ritz value of the Gram matrix), 2e-4 s_i in f32 (the bound of
            test_gpu_parity.py's random configurations).
  residual  |A^T A v_i - sigma_i^2 v_i| <= kappa sigma_i^2 q_i + R: the acceptance bound IS the Ritz residual.  R = 64 steps eps
            s_1^2 (the rounding of `steps` steps and of the Ritz combination, the form of test_gpu_spectral.py's bound); f32 adds
            4 * 2^-24 q_i s_1^2 (v_i, and on the wide side u_i, are rounded once to f32: |A^T A - sigma^2| <= s_1^2 times that).
  rows      |v_i . v_j - delta_ij| <= 64 steps eps (+ 2^-22 in f32) on the tall side: Ritz vectors of one orthonormal basis; the
            wide side adds 2 kappa s_1 / sigma_k, since v_i . v_j = u_i^T A A^T u_j / (sigma_i sigma_j) carries u_j's residual.
  sign      the entry of largest magnitude of every row is positive (svd_flip).
  steps     a run ends at a check: steps is a multiple of its interval (1 up to 64 steps, 2 up to 128, 4 up to 256, then 8) or
            the iteration cap; the interval is the one the restatement predicts wherever its own count is further than a
            tenth of itself from 64, 128 and 256 (its start vector is not the library's)."""
import functools

import numpy as np
import pytest
import torch

import lanczos_spectra_cases as LC
import sapca
from sapca import _lib as L
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KAPPA = LC.KAPPA
BOTH = [np.float64, np.float32]
IDS = dict(ids=["f64", "f32"])
SREL = {np.float64: 1e-5, np.float32: 2e-4}


def _device(A, dt):
    t = torch.float64 if dt == np.float64 else torch.float32
    return sapca.DeviceCsr(torch.from_numpy(A.indptr.astype(np.int64)).cuda(), torch.from_numpy(A.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(A.data.astype(np.float64)).to(t).cuda(), A.shape)


def _build(k, mask=None, centred=False):
    b = sapca.SparsePCABuilder.new() if mask is None else sapca.MaskedSparsePCABuilder.new().mask(mask)
    b = b.n_components(k).svd_method(SVDMethod.Lanczos())
    return (b.lanczos_center() if centred else b).build()


def _operator(A, mask=None, centred=False):
    D = A.toarray().astype(np.float64)
    if mask is not None:
        D = D[:, mask]
    return D - D.mean(0) if centred else D


def _interval(steps):
    return LC.step_class(steps)


def _check_triplets(D, s, est, dt, label, srel=None, exact_index=True, masked=False, interval=None):
    """every triplet of the fitted `est` against the operator D and its exact singular values s (exact_index: sigma_i is s_i;
    otherwise sigma_i is SOME exact value, the nearest); returns (sigma, components, steps)"""
    m, n = D.shape
    wide = n > m
    sigma, c = est.singular_values_(np.float64), est.components_(np.float64)
    steps = int(est.timings().lanczos_steps)
    k = sigma.size
    f32 = dt == np.float32
    srel = SREL[dt] if srel is None else srel
    assert c.shape == (k, n) and np.all(np.isfinite(c)) and np.all(np.isfinite(sigma)), label
    assert np.all(np.diff(sigma) <= 0) and np.all(sigma > 0), (label, sigma)
    want = s[:k] if exact_index else s[np.argmin(np.abs(s[None, :] - sigma[:, None]), axis=1)]
    rel = np.abs(sigma - want) / want
    G = D.T @ D
    worst_r = 0.0
    for i in range(k):
        q = s[0] / sigma[i] if wide else 1.0
        bound = KAPPA * sigma[i] ** 2 * q + 64 * steps * EPS * s[0] ** 2 + (4 * 2.0 ** -24 * q * s[0] ** 2 if f32 else 0.0)
        r = np.linalg.norm(G @ c[i] - sigma[i] ** 2 * c[i])
        worst_r = max(worst_r, r / bound)
        assert r <= bound, (label, i, r, bound)
    ortho = np.max(np.abs(c @ c.T - np.eye(k)))
    ortho_bound = 64 * steps * EPS + (2.0 ** -22 if f32 else 0.0) + (2 * KAPPA * s[0] / sigma[-1] if wide else 0.0)
    print(f"{label}: steps {steps}, sigma rel err {rel.max():.3e} (bound {srel:.0e}), residual / bound {worst_r:.3e}, "
          f"|C C^T - I| {ortho:.3e} (bound {ortho_bound:.3e})")
    assert np.all(rel <= srel), (label, rel.max())
    assert ortho <= ortho_bound, (label, ortho, ortho_bound)
    assert np.all(c[np.arange(k), np.argmax(np.abs(c), 1)] > 0), label
    jmax = LC.pca_jmax(m, n, k, masked)
    assert steps >= k and (steps % (interval or _interval(steps)) == 0 or steps == jmax), (label, steps)
    return sigma, c, steps


@functools.lru_cache(maxsize=None)
def _flat_reference(transposed, centred):
    D = _operator(LC.p_flat(transposed), None, centred)
    return D, np.linalg.svd(D, compute_uv=False)


# ------------------------------------------------------------------ P-flat
@pytest.mark.parametrize("dt", BOTH, **IDS)
@pytest.mark.parametrize("transposed", [False, True], ids=["tall", "wide"])
@pytest.mark.parametrize("k", LC.P_FLAT_KS)
def test_flat_spectrum_across_the_check_intervals(debug_switches, monkeypatch, k, transposed, dt):
    """P-flat: no gap, so k = 8, 30, 60, 100 end in the 2-, 4-, 4- and 8-step check intervals.  The same fit with every step
    checked (SAPCA_LANCZOS_CHECK=1) stops at s1, the first step at which the k triplets pass; the default schedule can only
    see that at its next check: steps in [s1, s1 + interval - 1], and both fits agree to 2 kappa."""
    A = LC.p_flat(transposed)
    D, s = _flat_reference(transposed, False)
    x = _device(A, dt)
    monkeypatch.delenv("SAPCA_LANCZOS_CHECK", raising=False)
    est = _build(k)
    est.fit(x)
    label = f"P-flat {'wide' if transposed else 'tall'} {np.dtype(dt).name} k {k}"
    sigma, _, steps = _check_triplets(D, s, est, dt, label)
    predicted = LC.P_FLAT_STEPS[k]
    if min(abs(predicted - b) for b in (64, 128, 256)) > predicted / 10:
        assert _interval(steps) == _interval(predicted), (label, steps, predicted)
    monkeypatch.setenv("SAPCA_LANCZOS_CHECK", "1")
    every = _build(k)
    every.fit(x)
    sigma1, _, s1 = _check_triplets(D, s, every, dt, label + " every step", interval=1)
    print(f"{label}: default {steps} steps, every step checked {s1} (restatement: {predicted})")
    assert s1 <= steps <= s1 + _interval(steps) - 1, (label, s1, steps)
    np.testing.assert_allclose(sigma, sigma1, rtol=2 * KAPPA)


@pytest.mark.parametrize("dt", BOTH, **IDS)
@pytest.mark.parametrize("transposed", [False, True], ids=["tall", "wide"])
def test_flat_spectrum_centred(transposed, dt):
    A = LC.p_flat(transposed)
    D, s = _flat_reference(transposed, True)
    est = _build(8, centred=True)
    est.fit(_device(A, dt))
    _check_triplets(D, s, est, dt, f"P-flat centred {'wide' if transposed else 'tall'} {np.dtype(dt).name} k 8")


# ------------------------------------------------------------------ P-all, P-tiny
@pytest.mark.parametrize("dt", BOTH, **IDS)
@pytest.mark.parametrize("wide", [False, True], ids=["tall", "wide"])
def test_all_and_all_but_one_triplets(wide, dt):
    """P-all: 30 x 12 and 12 x 30, k = 11 and k = 12 = the length of the Lanczos vectors (the run ends with the whole space: 12
    steps); the same behind a mask that drops two columns (30 x 10: k = 9, 10; 12 x 28: k = 11, 12)"""
    A = LC.p_all(wide)
    n = A.shape[1]
    mask = np.ones(n, dtype=bool)
    mask[[3, 7]] = False
    for m_ in (None, mask):
        D = _operator(A, m_)
        s = np.linalg.svd(D, compute_uv=False)
        full = min(D.shape)
        for k in (full - 1, full):
            est = _build(k, m_)
            est.fit(_device(A, dt))
            _, _, steps = _check_triplets(D, s, est, dt, f"P-all {A.shape} {'masked ' if m_ is not None else ''}{np.dtype(dt).name} k {k}",
                                          masked=m_ is not None)
            if k == full:
                assert steps == full


@pytest.mark.parametrize("dt", BOTH, **IDS)
@pytest.mark.parametrize("shape", LC.P_TINY_SHAPES, ids=[f"{a}x{b}" for a, b in LC.P_TINY_SHAPES])
def test_tiny_shapes(shape, dt):
    """P-tiny: every k of 2 x 2 and 3 x 2 and the single column of 5 x 1; a matrix of one row (1 x 1, 1 x 5) is refused before
    the driver (SAPCA_ERR_ARG, "need at least two samples") and the estimator goes on"""
    A = LC.p_tiny(shape)
    D = _operator(A)
    s = np.linalg.svd(D, compute_uv=False)
    for k in range(1, min(shape) + 1):
        est = _build(k)
        if shape[0] == 1:
            with pytest.raises(L.SapcaError, match="need at least two samples") as e:
                est.fit(_device(A, dt))
            assert e.value.status == 1
            A, D = LC.p_tiny((3, 2)), _operator(LC.p_tiny((3, 2)))
            s = np.linalg.svd(D, compute_uv=False)
        est.fit(_device(A, dt))
        _, _, steps = _check_triplets(D, s, est, dt, f"P-tiny {shape} {np.dtype(dt).name} k {k}")
        assert steps <= min(D.shape)


# ------------------------------------------------------------------ P-rank
def _refused(est, x, match):
    with pytest.raises(L.SapcaError, match=match) as e:
        est.fit(x)
    assert e.value.status == 4       # SAPCA_ERR_SVD
    return str(e.value)


@pytest.mark.parametrize("dt", BOTH, **IDS)
@pytest.mark.parametrize("wide", [False, True], ids=["tall", "wide"])
def test_exact_rank(wide, dt):
    """P-rank: rank 5 with integer entries.  k = 5: the Krylov space is exhausted after 6 steps and the triplets are exact (1e-10
    in f64).  k > 5: the contract of include/sapca.h, deviation 5 -- a Ritz value at or below 1e-12 of the largest (sigma <= 1e-6
    sigma_1) is a zero whatever its sign and is never a triplet, so the call is SAPCA_ERR_SVD with the rank in its message, on
    both sides alike and on every call; the handle then fits k = 5 to the bytes of a fresh one."""
    A = LC.p_rank(wide)
    D = _operator(A)
    s = np.linalg.svd(D, compute_uv=False)
    x = _device(A, dt)
    r = LC.P_RANK
    est = _build(r)
    est.fit(x)
    f64 = dt == np.float64
    sigma, c, steps = _check_triplets(D, s, est, dt, f"P-rank {A.shape} {np.dtype(dt).name} k {r}", srel=1e-10 if f64 else None)
    assert steps == r + 1            # r values and the start vector's share of the null space
    if f64:
        G = D.T @ D
        for i in range(r):
            assert np.linalg.norm(G @ c[i] - sigma[i] ** 2 * c[i]) <= 1e-10 * sigma[i] ** 2, i
    for k in (r + 1, r + 3):
        bad = _build(k)
        msg = "SVD computation failed: the operator has 5 singular values above 1e-6 of the largest, %d singular triplets were asked for" % k
        first = _refused(bad, x, msg)
        assert _refused(bad, x, msg) == first
    # after the refusals the same estimator class fits again, to the same bytes as before
    again = _build(r)
    again.fit(x)
    assert again.components_(np.float64).tobytes() == c.tobytes() and again.singular_values_(np.float64).tobytes() == sigma.tobytes()
    est.fit(x)
    assert est.components_(np.float64).tobytes() == c.tobytes()


# ------------------------------------------------------------------ P-zero, P-cap
@pytest.mark.parametrize("dt", BOTH, **IDS)
def test_zero_matrices_are_refused_and_the_handle_goes_on(dt):
    """P-zero: no entries, and stored zeros only: the operator has no singular value at all"""
    good = LC.p_all(False)
    D = _operator(good)
    s = np.linalg.svd(D, compute_uv=False)
    for stored in (False, True):
        est = _build(3)
        msg = _refused(est, _device(LC.p_zero(stored), dt), "SVD computation failed")
        print(f"P-zero stored={stored} {np.dtype(dt).name}: {msg}")
        assert "0 singular values above 1e-6 of the largest, 3 singular triplets were asked for" in msg
        est.fit(_device(good, dt))
        _check_triplets(D, s, est, dt, f"P-all after P-zero {np.dtype(dt).name}")


def test_iteration_cap_is_reported_and_the_handle_goes_on():
    """P-cap: A^T A = tridiag(1, 2, 1) of order 5000: the largest eigenvalue does not converge to kappa within the 20 k + 600 =
    620 steps of k = 1 (tests/test_lanczos_spectra_cases_cpu.py runs the restatement to the same end)"""
    est = _build(1)
    msg = _refused(est, _device(LC.p_cap(), np.float64), "SVD computation failed: Lanczos did not converge 1 singular triplets within 620 steps")
    print(msg)
    good = LC.p_all(False)
    D = _operator(good)
    est.fit(_device(good, np.float64))
    _check_triplets(D, np.linalg.svd(D, compute_uv=False), est, np.float64, "P-all after P-cap")


# ------------------------------------------------------------------ P-mult, P-cluster
@pytest.mark.parametrize("case,dt", [("mult", np.float64), ("mult", np.float32), ("cluster", np.float64)], ids=["mult-f64", "mult-f32", "cluster-f64"])
def test_repeated_and_clustered_values_are_true_triplets(case, dt):
    """P-mult (every singular value twice) and P-cluster (twice within a relative 1e-7, below kappa): reference behaviour,
    pinned.  A single-vector Lanczos may return fewer copies of a repeated singular value than its multiplicity, as las2 may
    (include/sapca.h, deviation 5): every returned triplet is a true one, the values descend, sigma_1 is exact and the vectors
    are orthonormal; which exact values were skipped is printed, not asserted."""
    A = LC.p_mult(1.0 if case == "mult" else 1.0 + 1e-7)
    D = _operator(A)
    s = np.linalg.svd(D, compute_uv=False)
    for k in LC.P_MULT_KS:
        est = _build(k)
        est.fit(_device(A, dt))
        label = f"P-{case} {np.dtype(dt).name} k {k}"
        sigma, _, _ = _check_triplets(D, s, est, dt, label, exact_index=False)
        assert abs(sigma[0] - s[0]) <= SREL[dt] * s[0]
        taken = np.zeros(len(s), dtype=bool)
        for x in sigma:                                   # each returned value takes the nearest exact one still free
            free = np.flatnonzero(~taken)
            taken[free[np.argmin(np.abs(s[free] - x))]] = True
        last = int(np.flatnonzero(taken).max())
        print(f"{label}: returned {np.array2string(sigma, precision=6)}; exact values skipped above the last returned one: "
              f"{np.array2string(s[:last + 1][~taken[:last + 1]], precision=6)}")

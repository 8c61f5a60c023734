"""GPU tests of the implicit regression on per-row covariates (sapca_set_covariates): the two kernels through
sapca_project_out_panel_*, fit parity against the oracle run on the densified residual (tests/covariates_ref.py), the
projection, the equivalences that tie the feature to the plain fits, and every refusal.

The planted matrices, their designs and seeds are those of covariates_ref.covariate_case; sigma_4 / sigma_5 of every
residual operator is asserted to be at least 2 by a dense SVD, so f32 is held to the project's own figures (1e-4 relative
on the singular values, 1e-4 rad subspace angle) and no tolerance is ever loosened."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import covariates_ref as R
import sapca
import sapca_oracle as O
from sapca import SVDMethod, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import _lib as L
from sapca import ops

pytestmark = pytest.mark.gpu

K = 4
EPS = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}          # unit roundoff
SIGMA_RTOL = {np.float32: 1e-4, np.float64: 1e-7}
ANGLE = {np.float32: 1e-4, np.float64: 1e-5}
MEAN_ATOL = {np.float32: 1e-5, np.float64: 1e-12}
TV_RTOL = {np.float32: 1e-5, np.float64: 1e-12}                 # of the raw second moment (the minuend)
PROJ_ATOL = {np.float32: 2e-4, np.float64: 1e-9}
NORM = {"QR": PIN.QR, "LU": PIN.LU, "NONE": PIN.NONE}

CASES = {   # name: (m, n, batches, continuous covariates, center, stress, rank of the design)
    "320x208": (320, 208, 3, 1, True, False, 4),
    "385x250": (385, 250, 0, 2, True, False, 3),
    "513x257": (513, 257, 8, 7, True, False, 15),
    "385x250-uncentred": (385, 250, 0, 2, False, False, 2),
    "320x208-stress": (320, 208, 3, 1, True, True, 4),
}


@functools.lru_cache(maxsize=None)
def _case(name, seed):
    m, n, nb, nc, center, stress, _ = CASES[name]
    A, Z, codes = R.covariate_case(m, n, seed, nb, nc, centred=center, stress=stress)
    for x in (A.data, A.indices, A.indptr, Z, codes):
        x.setflags(write=False)
    return A, Z, codes


@functools.lru_cache(maxsize=None)
def _expected(name, seed, masked, p, q, norm):
    """the oracle's fit of the densified residual, computed once per configuration and shared (read-only)"""
    m, n, _, _, center, _, _ = CASES[name]
    A, Z, _ = _case(name, seed)
    mask = synth.bernoulli_mask(n, 0.7, seed).numpy() if masked else None
    n_used = int(mask.sum()) if masked else n
    om = synth.gaussian_panel(n_used, K + p, seed + 7).numpy()
    want, Q, r, Res = R.expected_fit(A.toarray(), Z, center=center, n_components=K, n_oversamples=p, n_power_iterations=q,
                                     normalizer=norm, omega=om, mask=mask)
    g = R.gap(Res, K, mask)
    assert g >= 2.0, f"{name} seed {seed} masked {masked}: gap {g:.2f}"
    return want, Q, r, Res, mask, om


def _estimator(center, p, q, norm="QR", mask=None, variant=0, omega=None, centered_transform=True, method=None):
    b = sapca.MaskedSparsePCABuilder.new().mask(mask) if mask is not None else sapca.SparsePCABuilder.new()
    b = b.n_components(K).center(center).spmm_variant(variant).svd_method(method or SVDMethod.Random(p, q, NORM[norm]))
    if centered_transform:
        b = b.transform_semantics(L.TRANSFORM_CENTERED)
    est = b.build()
    return est.set_omega(omega) if omega is not None else est


def _input(A, dtype, entry, keep):
    """the matrix as the entry point wants it: a scipy CSR (host) or a DeviceCsr of a ResidentCsr (resident)"""
    A = A.astype(dtype)
    if entry == "host":
        return A
    s = ops.Session()
    res = s.upload(A.indptr, A.indices, A.data, *A.shape)
    keep.append((s, res))
    return res.as_device_csr()


def _host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("r", [1, 5, 16])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_project_out_panel(dtype, r):
    """P - Q (Q^T P) against numpy, element by element within (r + 3) eps_T (|P_ij| + sum_j |Q_ij| |S_j.|): the rounding of
    one conversion of S and r + 1 operations in T (derived, not measured); two calls give the same bytes.
    The reference sums S = Q^T P in extended precision (np.longdouble): the bound allows S one rounding and nothing for a
    sum over the rows, and a plain f64 sum -- numpy's own included -- carries an error of eps_f64 sum_i |Q_ij P_il| that
    exceeds it for f64 panels wherever |S_jl| is small beside that sum (measured with S = Q64.T @ P64 as the reference and
    plain f64 accumulation in the kernel: up to 2.75 times the bound at rows = 1000).  The kernel sums f64 panels in
    double-double for the same reason."""
    s = ops.Session()
    rng = np.random.default_rng(100 * r + (dtype == np.float64))
    for rows in (1, 63, 64, 65, 1000, 4097):
        Q = rng.standard_normal((rows, r))
        if rows >= r:
            Q = np.linalg.qr(Q)[0]
        Q = Q.astype(dtype)
        Q64, Qx = Q.astype(np.float64), Q.astype(np.longdouble)
        for l in (1, 16, 17, 60, 64, 110, 128, 140):
            P = (rng.standard_normal((rows, l)) + Q64 @ (50.0 * rng.standard_normal((r, l)))).astype(dtype)
            P64 = P.astype(np.float64)
            Sx = Qx.T @ P.astype(np.longdouble)
            want = (P.astype(np.longdouble) - Qx @ Sx).astype(np.float64)
            bound = (r + 3) * EPS[dtype] * (np.abs(P64) + np.abs(Q64) @ np.abs(Sx.astype(np.float64)))
            got = s.project_out_panel(P, Q)
            assert got.dtype == dtype and got.shape == P.shape
            err = np.abs(got.astype(np.float64) - want)
            worst = float((err / np.maximum(bound, 1e-300)).max())
            assert (err <= bound).all(), f"rows {rows} l {l} r {r}: error / bound {worst:.3f}"
            again = s.project_out_panel(P, Q)
            assert got.tobytes() == again.tobytes(), f"rows {rows} l {l} r {r}: two calls differ"


# ------------------------------------------------------------------ 2. fit parity with a shared Omega
def _fit_cases():
    out = []
    for name in CASES:                                            # every matrix: both dtypes, masked and not, host entry
        for dtype in (np.float32, np.float64):
            for masked in (False, True):
                out.append((name, 4, dtype, masked, "host", "QR", 0, 6))
    for name in CASES:                                            # the other seeds
        for seed in ((5,) if name == "385x250-uncentred" else (3, 5)):
            out.append((name, seed, np.float32, False, "host", "QR", 0, 6))
        out.append((name, 5, np.float32, True, "host", "QR", 0, 6))
    for norm in ("LU", "NONE"):
        for dtype in (np.float32, np.float64):
            out.append(("320x208", 4, dtype, False, "host", norm, 0, 6))
    for variant in (1, 2):
        for dtype in (np.float32, np.float64):
            out.append(("320x208", 4, dtype, variant == 2, "host", "QR", variant, 6))
    for p in (106, 136):                                          # l = 110 (ld 128) and l = 140 (the wide path)
        for dtype in (np.float32, np.float64):
            out.append(("320x208", 4, dtype, False, "host", "QR", 0, p))
    for name, dtype, masked in (("320x208", np.float32, False), ("320x208", np.float32, True), ("385x250", np.float64, False),
                                ("513x257", np.float32, True), ("385x250-uncentred", np.float32, False),
                                ("320x208-stress", np.float32, False)):
        out.append((name, 4, dtype, masked, "resident", "QR", 0, 6))
    return out


def _fit_id(c):
    name, seed, dtype, masked, entry, norm, variant, p = c
    return f"{name}-s{seed}-{np.dtype(dtype).name}-{'masked' if masked else 'full'}-{entry}-{norm}-v{variant}-p{p}"


@pytest.mark.parametrize("case", _fit_cases(), ids=_fit_id)
def test_fit_against_the_oracle_on_the_residual(case):
    """sigma, components, explained variance, total variance and rank are those of R = (I - Q Q^T) A; mean_ is A's.
    mean_ is held to 1e-5 (f32) / 1e-12 (f64) as everywhere in the project, except where f32 cannot represent the mean that
    closely: the stress case's three columns of 1000 +- 0.01 have means whose half ulp in f32 is 3e-5, so a column's bound
    is max(1e-5, 2^-24 |mean|) -- 1e-5 for every |mean| < 167."""
    name, seed, dtype, masked, entry, norm, variant, p = case
    m, n, _, _, center, _, rank = CASES[name]
    q = 2
    A, Z, _ = _case(name, seed)
    want, Q, r, Res, mask, om = _expected(name, seed, masked, p, q, norm)
    keep = []
    est = _estimator(center, p, q, norm, mask, variant, om).set_covariates(Z)
    est.fit(_input(A, dtype, entry, keep))
    note = _fit_id(case)
    assert r == rank and est.covariate_rank_ == rank, note
    s_got = est.singular_values_(np.float64)
    print(f"{note}: sigma rel {np.abs(s_got / want.singular_values - 1).max():.2e} "
          f"angle {O.subspace_angle(est.components_(np.float64), want.components):.2e}")
    np.testing.assert_allclose(s_got, want.singular_values, rtol=SIGMA_RTOL[dtype], err_msg=note)
    assert O.subspace_angle(est.components_(np.float64), want.components) < ANGLE[dtype], note
    np.testing.assert_allclose(est.explained_variance_(np.float64), want.singular_values ** 2 / (m - 1), rtol=3 * SIGMA_RTOL[dtype], err_msg=note)
    A64 = A.astype(dtype).astype(np.float64).toarray()
    mean = A64.mean(axis=0) if center else np.zeros(n)
    bound = np.maximum(MEAN_ATOL[dtype], (EPS[dtype] * (1 + 1e-6)) * np.abs(mean))
    assert (np.abs(est.mean_(np.float64) - mean) <= bound).all(), note
    used = slice(None) if mask is None else mask
    if center:
        raw = (A64[:, used] ** 2).sum() / (m - 1)
        tv = ((Res[:, used]) ** 2).sum() / (m - 1)
        print(f"{note}: total variance {est.total_variance_():.6g} want {tv:.6g} raw second moment {raw:.6g}")
        assert abs(est.total_variance_() - tv) <= TV_RTOL[dtype] * raw, note
        np.testing.assert_allclose(want.total_var, tv, rtol=1e-9)
    else:   # the reference's quirk: the sum of the k explained variances
        np.testing.assert_allclose(est.total_variance_(), want.total_var, rtol=3 * SIGMA_RTOL[dtype], err_msg=note)
    ratio = est.explained_variance_ratio(np.float64)
    np.testing.assert_allclose(ratio, O.explained_variance_ratio(want.explained_variance), atol=1e-5 if dtype == np.float32 else 1e-7, err_msg=note)


def test_a_fit_that_ignored_the_covariates_would_fail():
    """the plain centred PCA of the same matrix is a different answer: the tests above cannot pass by accident"""
    A, Z, _ = _case("320x208", 4)
    want, _, _, _, _, om = _expected("320x208", 4, False, 6, 2, "QR")
    est = _estimator(True, 6, 2, omega=om).fit(A)
    assert O.subspace_angle(est.components_(np.float64), want.components) > 0.05
    assert np.abs(est.singular_values_(np.float64) / want.singular_values - 1).max() > 3e-3


# ------------------------------------------------------------------ 3. transform
@pytest.mark.parametrize("entry", ["host", "resident"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["320x208", "385x250-uncentred", "320x208-stress"])
def test_scores_are_the_residuals_projection(name, dtype, masked, entry):
    m, n, _, _, center, _, _ = CASES[name]
    A, Z, _ = _case(name, 4)
    _, Q, _, Res, mask, om = _expected(name, 4, masked, 6, 2, "QR")
    keep = []
    x = _input(A, dtype, entry, keep)
    est = _estimator(center, 6, 2, "QR", mask, 0, om).set_covariates(Z)
    t = _host(est.fit_transform(x))
    two = _estimator(center, 6, 2, "QR", mask, 0, om).set_covariates(Z)
    t2 = _host(two.fit(x).transform(x))
    Vt = est.components_(np.float64)
    Aq = A.astype(dtype).astype(np.float64).toarray()
    Rq = R.residual(Aq, Q)
    want = (Rq if mask is None else Rq[:, mask]) @ Vt.T
    tol = PROJ_ATOL[dtype] * max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(t, want, atol=tol, rtol=0)
    np.testing.assert_allclose(t2, want, atol=tol, rtol=0)
    np.testing.assert_allclose(t2, t, atol=tol, rtol=0)
    assert np.abs(Q.T @ t.astype(np.float64)).max() <= tol


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
def test_out_of_sample_scores(dtype, masked):
    """fit on rows [0, 256), score rows [256, 320) with their own covariates: (A_new - D_new pinv(D) A) V^T"""
    A, Z, _ = _case("320x208", 4)
    n = A.shape[1]
    mask = synth.bernoulli_mask(n, 0.7, 4).numpy() if masked else None
    n_used = int(mask.sum()) if masked else n
    Af, An = A[:256].astype(dtype), A[256:].astype(dtype)
    om = synth.gaussian_panel(n_used, K + 6, 11).numpy()
    est = _estimator(True, 6, 2, "QR", mask, 0, om).set_covariates(Z[:256]).fit(Af)
    t = est.set_covariates(Z[256:]).transform(An)
    Vt = est.components_(np.float64)
    used = slice(None) if mask is None else mask
    want = R.out_of_sample_scores(Af.astype(np.float64).toarray()[:, used], R.design(Z[:256], True),
                                  An.astype(np.float64).toarray()[:, used], R.design(Z[256:], True), Vt)
    np.testing.assert_allclose(t, want, atol=PROJ_ATOL[dtype] * max(1.0, float(np.abs(want).max())), rtol=0)


# ------------------------------------------------------------------ 4. equivalences
def _fitted_bytes(est, t):
    return (est.components_().tobytes(), est.singular_values_(np.float64).tobytes(), est.mean_(np.float64).tobytes(),
            np.float64(est.total_variance_()).tobytes(), _host(t).tobytes())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
def test_set_then_clear_is_a_fresh_handle(dtype, masked):
    """the no-behaviour-change guarantee: covariates set and cleared leave a fit bit-identical to one on a fresh handle"""
    A, Z, _ = _case("320x208", 4)
    A = A.astype(dtype)
    mask = synth.bernoulli_mask(A.shape[1], 0.7, 4).numpy() if masked else None
    om = synth.gaussian_panel(int(mask.sum()) if masked else A.shape[1], K + 6, 3).numpy()
    for centered in (True, False):
        fresh = _estimator(True, 6, 2, "QR", mask, 0, om, centered_transform=centered)
        want = _fitted_bytes(fresh, fresh.fit_transform(A))
        est = _estimator(True, 6, 2, "QR", mask, 0, om, centered_transform=centered).set_covariates(Z).set_covariates()
        assert _fitted_bytes(est, est.fit_transform(A)) == want
        assert est.covariate_rank_ == 0
        if centered:   # ... and after a fit WITH covariates on the same handle
            est.set_covariates(Z).fit(A)
            assert est.covariate_rank_ == 4
            est.set_covariates(None)
            assert _fitted_bytes(est, est.fit_transform(A)) == want


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_column_of_ones_is_the_centring(dtype):
    """center = 0 with the single covariate 1: sigma and components of the plain center = 1 fit"""
    m, n = 320, 208
    ptr, idx, val = (x.numpy() for x in synth.gapped_csr(m, n, 0.3, K, seed=4, dtype=torch.float64))
    import scipy.sparse as sp
    A = sp.csr_matrix((val, idx.astype(np.int64), ptr), shape=(m, n))
    D = A.toarray()
    sv = np.linalg.svd(D - D.mean(axis=0), compute_uv=False)
    assert sv[K - 1] >= 2.0 * sv[K]
    om = synth.gaussian_panel(n, K + 6, 5).numpy()
    plain = _estimator(True, 6, 2, omega=om).fit(A.astype(dtype))
    est = _estimator(False, 6, 2, omega=om).set_covariates(np.ones((m, 1))).fit(A.astype(dtype))
    assert est.covariate_rank_ == 1
    np.testing.assert_allclose(est.singular_values_(np.float64), plain.singular_values_(np.float64), rtol=SIGMA_RTOL[dtype])
    assert O.subspace_angle(est.components_(np.float64), plain.components_(np.float64)) < ANGLE[dtype]
    assert not est.mean_(np.float64).any()      # center = 0: mean_ stays zeros


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_labels_are_per_batch_centring(dtype):
    """set_covariates(batch=...) with center = 1 against the explicitly per-batch column-centred dense matrix: its dense
    SVD certifies the gap, the oracle run on it with the same Omega gives the figures"""
    A, _, codes = _case("513x257", 4)
    m, n = A.shape
    D = A.astype(dtype).astype(np.float64).toarray()
    C_ = D.copy()
    for b in np.unique(codes):
        C_[codes == b] -= C_[codes == b].mean(axis=0)
    sv = np.linalg.svd(C_, compute_uv=False)
    assert sv[K - 1] >= 2.0 * sv[K]
    om = synth.gaussian_panel(n, K + 6, 9).numpy()
    want = O.fit(*R.dense_csr(C_), m, n, n_components=K, n_oversamples=6, n_power_iterations=2, normalizer="QR", center=True, omega=om)
    labels = [f"batch-{c}" for c in codes]
    est = _estimator(True, 6, 2, omega=om).set_covariates(batch=labels).fit(A.astype(dtype))
    assert est.covariate_rank_ == len(np.unique(codes))
    np.testing.assert_allclose(est.singular_values_(np.float64), want.singular_values, rtol=SIGMA_RTOL[dtype])
    assert O.subspace_angle(est.components_(np.float64), want.components) < ANGLE[dtype]
    raw = (D ** 2).sum() / (m - 1)
    assert abs(est.total_variance_() - (C_ ** 2).sum() / (m - 1)) <= TV_RTOL[dtype] * raw


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("variant", [0, 2])
def test_two_covariate_fits_are_bit_identical(dtype, variant):
    A, Z, _ = _case("513x257", 4)
    A = A.astype(dtype)
    om = synth.gaussian_panel(A.shape[1], K + 6, 3).numpy()
    a = _estimator(True, 6, 2, variant=variant, omega=om).set_covariates(Z)
    b = _estimator(True, 6, 2, variant=variant, omega=om).set_covariates(Z)
    first = _fitted_bytes(a, a.fit_transform(A))
    assert _fitted_bytes(b, b.fit_transform(A)) == first
    assert _fitted_bytes(a, a.fit_transform(A)) == first       # ... and on the same handle again


# ------------------------------------------------------------------ 5. refusals
def _raw_set(est, z, rows, cols):
    """sapca_set_covariates itself, past the Python layer's own checks"""
    ptr = None if z is None else np.ascontiguousarray(z, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    est._covariates = None
    L.check(est._h, L.load().sapca_set_covariates(est._h, ptr, C.c_uint64(rows), C.c_uint64(cols)))


def _plain_fit_works(est, A):
    est.set_covariates()
    t = est.fit_transform(A)
    assert np.isfinite(_host(t)).all() and est.covariate_rank_ == 0


def _arg_error(match):
    class _Ctx:
        def __enter__(self):
            self.cm = pytest.raises(L.SapcaError, match=match)
            self.e = self.cm.__enter__()
            return self.e

        def __exit__(self, *a):
            ok = self.cm.__exit__(*a)
            assert self.e.value.status == L.ERR_ARG
            return ok
    return _Ctx()


def test_refusals_of_set_covariates():
    A, Z, _ = _case("320x208", 4)
    A = A.astype(np.float32)
    m = A.shape[0]
    est = _estimator(True, 6, 2)
    with _arg_error("17 design columns"):
        _raw_set(est, np.zeros((m, 16)), m, 16)
    _plain_fit_works(est, A)
    z = np.array(Z)
    z[7, 2] = np.inf
    with _arg_error("non-finite value at row 7, column 2"):
        _raw_set(est, z, *z.shape)
    _plain_fit_works(est, A)
    with _arg_error("null"):
        _raw_set(est, None, m, 2)
    _plain_fit_works(est, A)
    unc = _estimator(False, 6, 2)
    _raw_set(unc, np.zeros((m, 16)), m, 16)                     # 16 columns without the intercept are fine
    with pytest.raises(ValueError, match="design columns"):    # the Python layer says the same before any library call
        est.set_covariates(np.zeros((m, 16)))


def test_refusals_at_fit_and_transform():
    A, Z, _ = _case("320x208", 4)
    A = A.astype(np.float32)
    m = A.shape[0]
    est = _estimator(True, 6, 2)
    with pytest.raises(ValueError, match="covariates have 319 rows, the matrix 320"):
        est.set_covariates(Z[:319]).fit(A)
    _raw_set(est, Z[:319], 319, Z.shape[1])
    for op in (est.fit, est.fit_transform):
        with _arg_error("covariates have 319 rows, the matrix 320"):
            op(A)
    _plain_fit_works(est, A)
    # a fitted model stays fitted through every refused transform
    est.set_covariates(Z).fit(A)
    comps = est.components_()
    _raw_set(est, Z[:300], 300, Z.shape[1])
    with _arg_error("covariates have 300 rows, the matrix 320"):
        est.transform(A)
    est.set_covariates()
    with _arg_error("the model was fitted with covariates, but none are set"):
        est.transform(A)
    est.set_covariates(Z[:, :2])
    with _arg_error("covariates have 2 columns, the fitted model's 4"):
        est.transform(A)
    np.testing.assert_array_equal(est.components_(), comps)
    assert est.covariate_rank_ == 4
    assert np.isfinite(est.set_covariates(Z).transform(A)).all()
    _plain_fit_works(est, A)
    est.set_covariates(Z)
    with _arg_error("covariates are set, but the model was fitted without"):
        est.transform(A)
    _plain_fit_works(est, A)


def test_refusals_of_routes():
    A, Z, _ = _case("320x208", 4)
    A = A.astype(np.float32)
    lz = _estimator(True, 6, 2, method=SVDMethod.Lanczos()).set_covariates(Z)
    for op in (lz.fit, lz.fit_transform):
        with _arg_error("covariates need SVDMethod::Random"):
            op(A)
    _plain_fit_works(lz, A)
    ref = _estimator(True, 6, 2, centered_transform=False).set_covariates(Z)
    with _arg_error("covariates need SAPCA_TRANSFORM_CENTERED"):
        ref.fit_transform(A)
    with pytest.raises(L.SapcaError, match="Model must be fitted first!"):   # refused before the fit
        ref.components_()
    ref.fit(A)                                                               # the fit alone is fine
    with _arg_error("covariates need SAPCA_TRANSFORM_CENTERED"):
        ref.transform(A)
    assert ref.covariate_rank_ == 4
    _plain_fit_works(ref, A)
    calls = []

    def allreduce(sendbuf, recvbuf, count, dtype, user):
        calls.append(count)
        return 0

    comm = _estimator(True, 6, 2).set_covariates(Z)
    comm.comm_set_callback(2, 0, allreduce)                     # rank 0 of 2: the handle belongs to a communicator
    for op in (comm.fit, comm.fit_transform):
        with _arg_error("handle that belongs to a communicator"):
            op(A)
    assert not calls                                            # refused before any collective
    comm.comm_set_callback(1, 0, allreduce)                     # one rank is no communicator: covariates are fine again
    assert comm.fit(A).covariate_rank_ == 4 and not calls
    _plain_fit_works(comm, A)
    k_big = sapca.SparsePCABuilder.new().n_components(318).svd_method(SVDMethod.Random(2, 1)).build().set_covariates(Z)
    with pytest.raises(L.SapcaError, match="n_components exceeds the matrix dimensions") as e:   # 318 > m - rank = 316
        k_big.fit(sp_dense_rows(320, 400))
    assert e.value.status == L.ERR_SVD


def sp_dense_rows(m, n):
    import scipy.sparse as sp
    return sp.csr_matrix(np.random.default_rng(0).standard_normal((m, n)).astype(np.float32))

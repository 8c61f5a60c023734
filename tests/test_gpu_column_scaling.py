"""GPU tests of the implicit column scaling (sapca_set_column_scaling): the row-scaling kernel through
sapca_scale_panel_rows_*, fit parity against the oracle run on the prescaled CSR (tests/column_scaling_ref.py), the projection,
the equivalences that tie the feature to the plain fits, the edge columns, covariates with explicit weights, two members
of a MultiDevice, and every refusal.

The matrices are column_scaling_ref.scaled_case: the planted gapped_csr with its columns spread over four decades.
sigma_4 / sigma_5 of every scaled operator is asserted to be at least 2 by a dense SVD, so the fits are held to the project's
own figures (1e-4 / 1e-7 relative on the singular values, 1e-4 / 1e-5 rad subspace angle) and no tolerance is ever loosened.
UNIT_VARIANCE standardises the columns by the library's own statistics; the WEIGHTS cases pass numpy's factors of the f64
matrix explicitly (for f32 input the library's own come from the rounded values: the two routes differ in more than a flag)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import column_scaling_ref as R
import covariates_ref as CR
import sapca
import sapca_oracle as O
from sapca import SVDMethod, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import _lib as L
from sapca import ops
from test_gpu_covariates import PROJ_ATOL

pytestmark = pytest.mark.gpu

K = R.K
EPS = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
SIGMA_RTOL = {np.float32: 1e-4, np.float64: 1e-7}
ANGLE = {np.float32: 1e-4, np.float64: 1e-5}
MEAN_ATOL = {np.float32: 1e-5, np.float64: 1e-12}
TV_RTOL = {np.float32: 1e-5, np.float64: 1e-12}                 # of the raw second moment of the scaled matrix (the minuend)
NORM = {"QR": PIN.QR, "LU": PIN.LU, "NONE": PIN.NONE}
SHAPES = {"320x208": (320, 208), "385x250": (385, 250), "513x257": (513, 257)}


@functools.lru_cache(maxsize=None)
def _matrix(name, seed, center):
    if name == "edge":
        A = R.edge_case()
    else:
        A = R.scaled_case(*SHAPES[name], seed, centred=center)
    for x in (A.data, A.indices, A.indptr):
        x.setflags(write=False)
    return A


def _mask(name, seed, masked):
    n = _matrix(name, seed, True).shape[1]
    return synth.bernoulli_mask(n, 0.7, seed).numpy() if masked else None


def _weights(name, seed, mode, A):
    """the full-width factors the reference applies: the library's rule in numpy -- derived by the library itself (UNIT_VARIANCE)
    or handed to it as explicit weights"""
    return R.unit_variance_factors(A)[0]


@functools.lru_cache(maxsize=None)
def _expected(name, seed, center, masked, mode, p, q, norm):
    """the oracle's fit of the prescaled CSR, computed once per configuration and shared (read-only)"""
    A = _matrix(name, seed, center)
    mask = _mask(name, seed, masked)
    d = _weights(name, seed, mode, A)
    n_used = int(mask.sum()) if masked else A.shape[1]
    om = synth.gaussian_panel(n_used, K + p, seed + 7).numpy()
    g = R.gap(R.scaled_operator(A, d, center, mask), K)
    assert g >= 2.0, f"{name} seed {seed} center {center} masked {masked} {mode}: gap {g:.2f}"
    want = R.expected_fit(A, d, center=center, n_components=K, n_oversamples=p, n_power_iterations=q, normalizer=norm, omega=om, mask=mask)
    return want, d, mask, om, g


def _estimator(center, p, q, norm="QR", mask=None, variant=0, omega=None, centered_transform=True, method=None):
    b = sapca.MaskedSparsePCABuilder.new().mask(mask) if mask is not None else sapca.SparsePCABuilder.new()
    b = b.n_components(K).center(center).spmm_variant(variant).svd_method(method or SVDMethod.Random(p, q, NORM[norm]))
    if centered_transform:
        b = b.transform_semantics(L.TRANSFORM_CENTERED)
    est = b.build()
    return est.set_omega(omega) if omega is not None else est


def _scaling(mode, d):
    return "unit_variance" if mode == "unit" else d


def _input(A, dtype, entry, keep):
    A = A.astype(dtype)
    if entry == "host":
        return A
    s = ops.Session()
    res = s.upload(A.indptr, A.indices, A.data, *A.shape)
    keep.append((s, res))
    return res.as_device_csr()


def _host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def _used(mask):
    return slice(None) if mask is None else mask


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scale_panel_rows(dtype):
    """panel[r][:] * T(scale[r]) against numpy, bit for bit: the factor is rounded once to T, each product once.  Values and
    factors stay in the normal range of T; a factor of 0 gives zeros."""
    s = ops.Session()
    rng = np.random.default_rng(7 + (dtype == np.float64))
    for rows in (1, 63, 64, 65, 1000, 4097):
        scale = 10.0 ** rng.uniform(-3, 3, rows)
        scale[rng.random(rows) < 0.1] = 0.0
        scale[0] = 0.0 if rows > 1 else scale[0]
        for l in (1, 16, 17, 60, 64, 110, 128, 140):
            P = (rng.standard_normal((rows, l)) * 10.0 ** rng.uniform(-3, 3, (rows, l))).astype(dtype)
            want = P * scale.astype(dtype)[:, None]
            got = s.scale_panel_rows(P, scale)
            assert got.dtype == dtype and got.shape == P.shape
            assert got.tobytes() == want.astype(dtype).tobytes(), f"rows {rows} l {l}"
            assert not got[scale == 0].any()


# ------------------------------------------------------------------ 2. fit parity with a shared Omega
def _fit_cases():
    out = []
    for name in SHAPES:                                           # every shape: both dtypes, masked and not, both modes, host entry
        for dtype in (np.float32, np.float64):
            for masked in (False, True):
                for mode in ("unit", "weights"):
                    out.append((name, 4, dtype, True, masked, mode, "host", "QR", 0, 6))
    for name in SHAPES:                                           # the other seeds
        for seed in (3, 5):
            for mode in ("unit", "weights"):
                out.append((name, seed, np.float32, True, seed == 5, mode, "host", "QR", 0, 6))
    for dtype in (np.float32, np.float64):
        for norm in ("LU", "NONE"):
            out.append(("320x208", 4, dtype, True, False, "unit", "host", norm, 0, 6))
        for variant in (1, 2):
            out.append(("320x208", 4, dtype, True, variant == 2, "unit", "host", "QR", variant, 6))
        for p in (106, 136):                                      # l = 110 (ld 128) and l = 140 (the wide path)
            out.append(("320x208", 4, dtype, True, False, "unit", "host", "QR", 0, p))
        for masked in (False, True):                              # uncentred
            for mode in ("unit", "weights"):
                out.append(("320x208", 4, dtype, False, masked, mode, "host", "QR", 0, 6))
    for dtype, masked, mode in ((np.float32, False, "unit"), (np.float32, True, "weights"), (np.float64, True, "unit"),
                                (np.float64, False, "weights")):
        out.append(("320x208", 4, dtype, True, masked, mode, "resident", "QR", 0, 6))
    return out


def _fit_id(c):
    name, seed, dtype, center, masked, mode, entry, norm, variant, p = c
    return (f"{name}-s{seed}-{np.dtype(dtype).name}-{'centred' if center else 'uncentred'}-{'masked' if masked else 'full'}-{mode}-"
            f"{entry}-{norm}-v{variant}-p{p}")


def _check_factors(est, A, dtype, mode, d_given, mask, note):
    """sapca_get_column_scale against the reference.  WEIGHTS: the weights, compacted, bit for bit.  UNIT_VARIANCE: d of the
    matrix as the library holds it (rounded to dtype), within 2 m eps sumsq / ss + 4 eps; exactly 0 where the reference is."""
    got = est.column_scale_
    used = _used(mask)
    if mode == "weights":
        assert got.tobytes() == np.ascontiguousarray(d_given[used]).tobytes(), note
        return
    d_ref, ss, s2 = R.unit_variance_factors(A.astype(dtype))
    d_ref, ss, s2 = d_ref[used], ss[used], s2[used]
    live = d_ref > 0
    assert not got[~live].any(), note
    rel = np.abs(got[live] / d_ref[live] - 1)
    bound = R.factor_bound(A.shape[0], ss[live], s2[live])
    print(f"{note}: d rel {rel.max():.2e}, worst rel / bound {(rel / bound).max():.3f}")
    assert (rel <= bound).all(), note


@pytest.mark.parametrize("case", _fit_cases(), ids=_fit_id)
def test_fit_against_the_oracle_on_the_prescaled_matrix(case):
    name, seed, dtype, center, masked, mode, entry, norm, variant, p = case
    q = 2
    A = _matrix(name, seed, center)
    m, n = A.shape
    want, d, mask, om, g = _expected(name, seed, center, masked, mode, p, q, norm)
    keep = []
    est = _estimator(center, p, q, norm, mask, variant, om).set_column_scaling(_scaling(mode, d))
    est.fit(_input(A, dtype, entry, keep))
    note = _fit_id(case)
    s_got = est.singular_values_(np.float64)
    ang = O.subspace_angle(est.components_(np.float64), want.components)
    print(f"{note}: gap {g:.2f} sigma rel {np.abs(s_got / want.singular_values - 1).max():.2e} angle {ang:.2e}")
    np.testing.assert_allclose(s_got, want.singular_values, rtol=SIGMA_RTOL[dtype], err_msg=note)
    assert ang < ANGLE[dtype], note
    np.testing.assert_allclose(est.explained_variance_(np.float64), want.singular_values ** 2 / (m - 1), rtol=3 * SIGMA_RTOL[dtype], err_msg=note)
    ratio = est.explained_variance_ratio(np.float64)
    np.testing.assert_allclose(ratio, O.explained_variance_ratio(want.explained_variance), atol=1e-5 if dtype == np.float32 else 1e-7, err_msg=note)
    A64 = A.astype(dtype).astype(np.float64).toarray()
    mean = A64.mean(axis=0) if center else np.zeros(n)            # mean_ is that of A, not of A D
    bound = np.maximum(MEAN_ATOL[dtype], (EPS[dtype] * (1 + 1e-6)) * np.abs(mean))
    assert (np.abs(est.mean_(np.float64) - mean) <= bound).all(), note
    used = _used(mask)
    n_used = int(mask.sum()) if masked else n
    tv = est.total_variance_()
    if center:
        raw = ((A64[:, used] * d[used]) ** 2).sum() / (m - 1)
        print(f"{note}: total variance {tv:.12g} want {want.total_var:.12g}")
        assert abs(tv - want.total_var) <= TV_RTOL[dtype] * raw, note
        if mode == "unit":
            assert abs(tv - np.count_nonzero(d[used])) <= 1e-12 * n_used, note
    else:   # the reference's quirk: the sum of the k explained variances
        np.testing.assert_allclose(tv, want.total_var, rtol=3 * SIGMA_RTOL[dtype], err_msg=note)
    _check_factors(est, A, dtype, mode, d, mask, note)


@pytest.mark.parametrize("mode", ["unit", "weights"])
def test_a_fit_that_ignored_the_scaling_would_fail(mode):
    """the plain fit of the same matrix is a different answer: the tests above cannot pass by accident"""
    A = _matrix("320x208", 4, True)
    want, _, _, om, _ = _expected("320x208", 4, True, False, mode, 6, 2, "QR")
    est = _estimator(True, 6, 2, omega=om).fit(A)
    assert est.column_scale_ is None
    assert O.subspace_angle(est.components_(np.float64), want.components) > 0.05
    assert np.abs(est.singular_values_(np.float64) / want.singular_values - 1).max() > 3e-3


# ------------------------------------------------------------------ 3. transform
@pytest.mark.parametrize("entry", ["host", "resident"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", ["unit", "weights"])
def test_scores_are_the_scaled_projection(mode, dtype, masked, entry):
    """fit_transform, fit + transform and the dense ((A - mu) d) V^T agree"""
    A = _matrix("320x208", 4, True)
    _, d, mask, om, _ = _expected("320x208", 4, True, masked, mode, 6, 2, "QR")
    keep = []
    x = _input(A, dtype, entry, keep)
    est = _estimator(True, 6, 2, "QR", mask, 0, om).set_column_scaling(_scaling(mode, d))
    t = _host(est.fit_transform(x))
    two = _estimator(True, 6, 2, "QR", mask, 0, om).set_column_scaling(_scaling(mode, d))
    t2 = _host(two.fit(x).transform(x))
    Vt = est.components_(np.float64)
    Aq = A.astype(dtype).astype(np.float64).toarray()[:, _used(mask)]
    want = ((Aq - Aq.mean(axis=0)) * est.column_scale_) @ Vt.T
    tol = PROJ_ATOL[dtype] * max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(t, want, atol=tol, rtol=0)
    np.testing.assert_allclose(t2, want, atol=tol, rtol=0)
    np.testing.assert_allclose(t2, t, atol=tol, rtol=0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
def test_out_of_sample_scores(dtype, masked):
    """fit on rows [0, 256), score rows [256, 320) with the fit's d and mu -- whatever is set on the handle by then"""
    A = _matrix("320x208", 4, True)
    n = A.shape[1]
    mask = _mask("320x208", 4, masked)
    n_used = int(mask.sum()) if masked else n
    Af, An = A[:256].astype(dtype), A[256:].astype(dtype)
    om = synth.gaussian_panel(n_used, K + 6, 11).numpy()
    est = _estimator(True, 6, 2, "QR", mask, 0, om).set_column_scaling("unit_variance").fit(Af)
    d = est.column_scale_
    t = est.transform(An)
    est.set_column_scaling(np.ones(n))                          # only concerns the next fit
    t_again = est.transform(An)
    est.set_column_scaling(None)
    t_cleared = est.transform(An)
    assert t.tobytes() == t_again.tobytes() == t_cleared.tobytes()
    used = _used(mask)
    F, N = Af.astype(np.float64).toarray()[:, used], An.astype(np.float64).toarray()[:, used]
    np.testing.assert_allclose(d, R.unit_variance_factors(F)[0], rtol=1e-9)
    want = ((N - F.mean(axis=0)) * d) @ est.components_(np.float64).T
    np.testing.assert_allclose(t, want, atol=PROJ_ATOL[dtype] * max(1.0, float(np.abs(want).max())), rtol=0)


# ------------------------------------------------------------------ 4. equivalences
def _fitted_bytes(est, t):
    return (est.components_().tobytes(), est.singular_values_(np.float64).tobytes(), est.mean_(np.float64).tobytes(),
            np.float64(est.total_variance_()).tobytes(), _host(t).tobytes())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
def test_unit_variance_is_weights_fed_with_its_factors(dtype, masked):
    A = _matrix("320x208", 4, True).astype(dtype)
    n = A.shape[1]
    mask = _mask("320x208", 4, masked)
    om = synth.gaussian_panel(int(mask.sum()) if masked else n, K + 6, 3).numpy()
    a = _estimator(True, 6, 2, "QR", mask, 0, om).set_column_scaling("unit_variance")
    first = _fitted_bytes(a, a.fit_transform(A))
    w = np.zeros(n)
    w[_used(mask)] = a.column_scale_
    b = _estimator(True, 6, 2, "QR", mask, 0, om).set_column_scaling(w)
    assert _fitted_bytes(b, b.fit_transform(A)) == first
    assert b.column_scale_.tobytes() == a.column_scale_.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_unit_variance_does_not_see_column_gains(dtype):
    """UNIT_VARIANCE of A against UNIT_VARIANCE of A with other column gains: the standardised operator is the same"""
    A = _matrix("320x208", 4, True)
    n = A.shape[1]
    other = R.scaled_case(320, 208, 4, gains=R.column_gains(n, 99))
    om = synth.gaussian_panel(n, K + 6, 3).numpy()
    a = _estimator(True, 6, 2, omega=om).set_column_scaling("unit_variance").fit(A.astype(dtype))
    b = _estimator(True, 6, 2, omega=om).set_column_scaling("unit_variance").fit(other.astype(dtype))
    np.testing.assert_allclose(b.singular_values_(np.float64), a.singular_values_(np.float64), rtol=SIGMA_RTOL[dtype])
    assert O.subspace_angle(b.components_(np.float64), a.components_(np.float64)) < ANGLE[dtype]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
def test_weights_of_one_and_host_prescaling(dtype, masked):
    """weights all 1 against the plain fit (on the planted matrix without gains: the plain fit needs its gap), and a scaled fit
    of A against the plain fit of the host-prescaled matrix.  The weights of the second pair are the unit-variance factors
    rounded to powers of two, so the prescaled values are exact in both dtypes."""
    n = 208
    A = R.scaled_case(320, n, 4, gains=np.ones(n)).astype(dtype)
    mask = _mask("320x208", 4, masked)
    om = synth.gaussian_panel(int(mask.sum()) if masked else n, K + 6, 3).numpy()
    S = R.scaled_operator(A, np.ones(n), True, mask)
    assert R.gap(S, K) >= 2.0
    plain = _estimator(True, 6, 2, "QR", mask, 0, om)
    tp = plain.fit_transform(A)
    ones = _estimator(True, 6, 2, "QR", mask, 0, om).set_column_scaling(np.ones(n))
    t1 = ones.fit_transform(A)
    np.testing.assert_allclose(ones.singular_values_(np.float64), plain.singular_values_(np.float64), rtol=SIGMA_RTOL[dtype])
    assert O.subspace_angle(ones.components_(np.float64), plain.components_(np.float64)) < ANGLE[dtype]
    np.testing.assert_allclose(t1, tp, atol=PROJ_ATOL[dtype] * max(1.0, float(np.abs(tp).max())), rtol=0)
    A = _matrix("320x208", 4, True).astype(dtype)
    w = 2.0 ** np.round(np.log2(R.unit_variance_factors(A)[0]))
    assert R.gap(R.scaled_operator(A, w, True, mask), K) >= 2.0
    scaled = _estimator(True, 6, 2, "QR", mask, 0, om).set_column_scaling(w)
    ts = scaled.fit_transform(A)
    pre = _estimator(True, 6, 2, "QR", mask, 0, om)
    tq = pre.fit_transform(R.prescaled(A, w).astype(dtype))
    np.testing.assert_allclose(scaled.singular_values_(np.float64), pre.singular_values_(np.float64), rtol=SIGMA_RTOL[dtype])
    assert O.subspace_angle(scaled.components_(np.float64), pre.components_(np.float64)) < ANGLE[dtype]
    np.testing.assert_allclose(ts, tq, atol=PROJ_ATOL[dtype] * max(1.0, float(np.abs(tq).max())), rtol=0)
    np.testing.assert_allclose(scaled.total_variance_(), pre.total_variance_(), rtol=1e-9)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("variant", [0, 2])
def test_two_scaled_fits_are_bit_identical(dtype, variant):
    A = _matrix("513x257", 4, True).astype(dtype)
    om = synth.gaussian_panel(A.shape[1], K + 6, 3).numpy()
    a = _estimator(True, 6, 2, variant=variant, omega=om).set_column_scaling("unit_variance")
    b = _estimator(True, 6, 2, variant=variant, omega=om).set_column_scaling("unit_variance")
    first = _fitted_bytes(a, a.fit_transform(A))
    assert _fitted_bytes(b, b.fit_transform(A)) == first
    assert _fitted_bytes(a, a.fit_transform(A)) == first       # ... and on the same handle again


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
def test_set_then_clear_is_a_fresh_handle(dtype, masked):
    """the no-behaviour-change guarantee: scaling set and cleared leaves fit and projection bit-identical to a fresh handle's"""
    A = _matrix("320x208", 4, True).astype(dtype)
    n = A.shape[1]
    mask = _mask("320x208", 4, masked)
    om = synth.gaussian_panel(int(mask.sum()) if masked else n, K + 6, 3).numpy()
    for centered in (True, False):
        fresh = _estimator(True, 6, 2, "QR", mask, 0, om, centered_transform=centered)
        want = _fitted_bytes(fresh, fresh.fit_transform(A))
        est = _estimator(True, 6, 2, "QR", mask, 0, om, centered_transform=centered)
        est.set_column_scaling("unit_variance").set_column_scaling(np.ones(n)).set_column_scaling(None)
        assert _fitted_bytes(est, est.fit_transform(A)) == want
        assert est.column_scale_ is None
        if centered:   # ... and after a scaled fit on the same handle
            est.set_column_scaling("unit_variance").fit_transform(A)
            assert est.column_scale_ is not None
            est.set_column_scaling(None)
            assert _fitted_bytes(est, est.fit_transform(A)) == want
            assert _fitted_bytes(est, est.fit(A).transform(A))[:4] == want[:4]


# ------------------------------------------------------------------ 5. the edge matrix
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
def test_edge_columns(dtype, masked):
    """an empty column, two constant ones (3.0; 0.1f, whose numpy ss is negative) and a single-entry column: d is 0, 0, 0
    and finite; nothing is NaN; the dead columns' component entries are exactly 0; the total variance counts the live ones"""
    A = _matrix("edge", 4, True)
    m, n = A.shape
    want, d, mask, om, g = _expected("edge", 4, True, masked, "unit", 6, 2, "QR")
    assert not d[[3, 10, 11]].any() and np.isfinite(d[12]) and d[12] > 0
    assert np.count_nonzero(d) == 205
    assert abs(g - (3.25 if masked else 3.79)) < 0.01
    est = _estimator(True, 6, 2, "QR", mask, 0, om).set_column_scaling("unit_variance")
    t = est.fit_transform(A.astype(dtype))
    got_d = est.column_scale_
    comps = est.components_(np.float64)
    assert np.isfinite(t).all() and np.isfinite(comps).all() and np.isfinite(got_d).all()
    full = np.zeros(n)
    full[_used(mask)] = got_d
    kept = np.ones(n, bool) if mask is None else mask
    for j in (3, 10, 11):
        if kept[j]:
            assert full[j] == 0.0
            assert not comps[:, int(kept[:j].sum())].any()
    if kept[12]:
        assert np.isfinite(full[12]) and full[12] > 0
    _check_factors(est, A, dtype, "unit", d, mask, f"edge-{np.dtype(dtype).name}-{masked}")
    live = np.count_nonzero(d[_used(mask)])
    assert abs(est.total_variance_() - live) <= 1e-12 * int(kept.sum())
    np.testing.assert_allclose(est.singular_values_(np.float64), want.singular_values, rtol=SIGMA_RTOL[dtype])
    assert O.subspace_angle(comps, want.components) < ANGLE[dtype]


# ------------------------------------------------------------------ 6. covariates x explicit weights
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name,nb,nc,rank", [("320x208", 3, 1, 4), ("513x257", 8, 7, 15)])
def test_covariates_with_weights(name, nb, nc, rank, dtype):
    """covariate_case with its columns multiplied by gains g, weights 1 / g: fit and scores against covariates_ref.expected_fit
    of the prescaled matrix -- which is the covariate case itself"""
    m, n = SHAPES[name]
    A0, Z, _ = CR.covariate_case(m, n, 4, nb, nc)
    g = R.column_gains(n, 4)
    A = R.prescaled(A0, g)
    w = 1.0 / g
    B = R.prescaled(A.astype(dtype), w).toarray()               # what the library's operator is made of
    om = synth.gaussian_panel(n, K + 6, 11).numpy()
    want, Q, r, Res = CR.expected_fit(B, Z, center=True, n_components=K, n_oversamples=6, n_power_iterations=2, normalizer="QR", omega=om)
    assert r == rank and CR.gap(Res, K) >= 2.0
    est = _estimator(True, 6, 2, omega=om).set_covariates(Z).set_column_scaling(w)
    t = est.fit_transform(A.astype(dtype))
    assert est.covariate_rank_ == rank
    np.testing.assert_allclose(est.singular_values_(np.float64), want.singular_values, rtol=SIGMA_RTOL[dtype])
    assert O.subspace_angle(est.components_(np.float64), want.components) < ANGLE[dtype]
    raw = (B ** 2).sum() / (m - 1)
    assert abs(est.total_variance_() - (Res ** 2).sum() / (m - 1)) <= TV_RTOL[dtype] * raw
    scores = Res @ est.components_(np.float64).T
    tol = PROJ_ATOL[dtype] * max(1.0, float(np.abs(scores).max()))
    np.testing.assert_allclose(t, scores, atol=tol, rtol=0)
    np.testing.assert_allclose(est.transform(A.astype(dtype)), scores, atol=tol, rtol=0)


# ------------------------------------------------------------------ 7. two members of one MultiDevice
def test_two_members_agree_with_one_handle():
    m, n, p, q = 2000, 400, 6, 2
    ptr, idx, val = (x.numpy() for x in synth.gapped_csr(m, n, 0.3, K, seed=4, dtype=torch.float64))
    import scipy.sparse as sp
    A = sp.csr_matrix((val * R.column_gains(n, 4)[idx], idx.astype(np.int64), ptr), shape=(m, n))
    d = R.unit_variance_factors(A)[0]
    assert R.gap(R.scaled_operator(A, d, True), K) >= 2.0
    A = A.astype(np.float32)
    om = synth.gaussian_panel(n, K + p, 5).numpy()
    make = lambda: (sapca.SparsePCABuilder.new().n_components(K).transform_semantics(L.TRANSFORM_CENTERED)
                    .svd_method(SVDMethod.Random(p, q, PIN.QR)).build())
    one = make().set_omega(om).set_column_scaling("unit_variance")
    t1 = one.fit_transform(A)
    md = sapca.MultiDevice(make(), [0, 0]).set_omega(om).set_column_scaling("unit_variance")
    t = md.fit_transform(A)
    np.testing.assert_allclose(md.singular_values_(np.float64), one.singular_values_(np.float64), rtol=2e-5)
    assert O.subspace_angle(md.components_(np.float64), one.components_(np.float64)) < 2e-5
    np.testing.assert_allclose(md.mean_(np.float64), one.mean_(np.float64), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(t, t1, atol=2e-4 * np.abs(t1).max())
    np.testing.assert_allclose(md.transform(A), t, atol=2e-4 * np.abs(t).max())
    a, b = md.member(0), md.member(1)
    assert np.array_equal(a.components_(np.float32), b.components_(np.float32))
    assert a.column_scale_.tobytes() == b.column_scale_.tobytes()
    assert np.float64(a.total_variance_()).tobytes() == np.float64(b.total_variance_()).tobytes()
    np.testing.assert_allclose(a.column_scale_, one.column_scale_, rtol=1e-12)
    assert abs(a.total_variance_() - np.count_nonzero(d)) <= 1e-12 * n


# ------------------------------------------------------------------ 8. refusals
def _raw_set(est, mode, w, length):
    """sapca_set_column_scaling itself, past the Python layer's own checks"""
    ptr = None if w is None else np.ascontiguousarray(w, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    est._scale_weights = None
    L.check(est._h, L.load().sapca_set_column_scaling(est._h, C.c_int32(mode), ptr, C.c_uint64(length)))


def _plain_fit_works(est, A):
    est.set_column_scaling(None)
    t = est.fit_transform(A)
    assert np.isfinite(_host(t)).all() and est.column_scale_ is None


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


def test_refusals_of_set_column_scaling():
    A = _matrix("320x208", 4, True).astype(np.float32)
    n = A.shape[1]
    est = _estimator(True, 6, 2).set_column_scaling("unit_variance")
    est.fit(A)
    comps, d = est.components_(), est.column_scale_
    with _arg_error("unknown mode 3"):
        _raw_set(est, 3, None, 0)
    with _arg_error("unknown mode -1"):
        _raw_set(est, -1, None, 0)
    with _arg_error(f"null array of {n} weights"):
        _raw_set(est, L.SCALE_WEIGHTS, None, n)
    with _arg_error(f"unit variance takes no weights \\({n} given\\)"):
        _raw_set(est, L.SCALE_UNIT_VARIANCE, np.ones(n), n)
    w = np.ones(n)
    w[17] = -0.5
    with _arg_error("column scaling: weight -0.5 at column 17"):
        _raw_set(est, L.SCALE_WEIGHTS, w, n)
    for bad in (np.inf, np.nan):
        w[17], w[40] = 1.0, bad
        with _arg_error(f"column scaling: weight {bad:g} at column 40"):
            _raw_set(est, L.SCALE_WEIGHTS, w, n)
    # a refused setting changes nothing: the model stays fitted, the earlier setting stays
    np.testing.assert_array_equal(est.components_(), comps)
    assert est.column_scale_.tobytes() == d.tobytes()
    assert est.fit(A).column_scale_.tobytes() == d.tobytes()
    _plain_fit_works(est, A)
    # the Python layer says the same before any library call
    for bad, msg in (("unit", "unknown mode"), (np.ones((2, n)), "one-dimensional"), (w, "weight nan at column 40"),
                     (-np.ones(n), "weight -1 at column 0")):
        with pytest.raises(ValueError, match=msg):
            est.set_column_scaling(bad)
    with pytest.raises(ValueError, match=f"column scaling has {n - 1} weights, the matrix {n} columns"):
        est.set_column_scaling(np.ones(n - 1)).fit(A)
    _plain_fit_works(est, A)


def test_refusals_at_fit_and_transform():
    A = _matrix("320x208", 4, True).astype(np.float32)
    m, n = A.shape
    est = _estimator(True, 6, 2).set_column_scaling("unit_variance").fit(A)
    comps = est.components_()
    _raw_set(est, L.SCALE_WEIGHTS, np.ones(n - 1), n - 1)
    for op in (est.fit, est.fit_transform):
        with _arg_error(f"column scaling has {n - 1} weights, the matrix {n} columns"):
            op(A)
    np.testing.assert_array_equal(est.components_(), comps)     # a refused fit leaves the fitted model
    assert np.isfinite(est.transform(A)).all()
    _plain_fit_works(est, A)
    one_row = _estimator(True, 0, 1).set_column_scaling("unit_variance")
    with _arg_error("unit variance needs at least two rows, the matrix has 1"):
        one_row.fit(A[:1])
    _plain_fit_works(one_row, A)
    _, Z, _ = CR.covariate_case(m, n, 4, 3, 1)
    cov = _estimator(True, 6, 2).set_covariates(Z).set_column_scaling("unit_variance")
    for op in (cov.fit, cov.fit_transform):
        with _arg_error("pass explicit weights"):
            op(A)
    assert np.isfinite(cov.set_column_scaling(np.ones(n)).fit_transform(A)).all()
    cov.set_covariates()
    _plain_fit_works(cov, A)


def test_refusals_of_routes():
    A = _matrix("320x208", 4, True).astype(np.float32)
    lz = _estimator(True, 6, 2, method=SVDMethod.Lanczos()).set_column_scaling("unit_variance")
    for op in (lz.fit, lz.fit_transform):
        with _arg_error("column scaling needs SVDMethod::Random"):
            op(A)
    _plain_fit_works(lz, A)
    ref = _estimator(True, 6, 2, centered_transform=False).set_column_scaling("unit_variance")
    with _arg_error("column scaling needs SAPCA_TRANSFORM_CENTERED"):
        ref.fit_transform(A)
    with pytest.raises(L.SapcaError, match="Model must be fitted first!"):   # refused before the fit
        ref.components_()
    ref.fit(A)                                                               # the fit alone is fine
    comps = ref.components_()
    ref.set_column_scaling(None)                                             # the MODEL is scaled, whatever is set now
    with _arg_error("column scaling needs SAPCA_TRANSFORM_CENTERED"):
        ref.transform(A)
    np.testing.assert_array_equal(ref.components_(), comps)
    assert ref.column_scale_ is not None
    _plain_fit_works(ref, A)
    calls = []

    def allreduce(sendbuf, recvbuf, count, dtype, user):
        calls.append(count)
        return 0

    comm = _estimator(True, 6, 2, method=SVDMethod.Lanczos()).set_column_scaling("unit_variance")
    comm.comm_set_callback(2, 0, allreduce)                     # rank 0 of 2: the handle belongs to a communicator
    for op in (comm.fit, comm.fit_transform):
        with _arg_error("column scaling needs SVDMethod::Random"):
            op(A)
    cw = _estimator(True, 6, 2).set_column_scaling(np.ones(A.shape[1] + 1))
    cw.comm_set_callback(2, 0, allreduce)
    cw._scale_weights = None
    with _arg_error("column scaling has 209 weights, the matrix 208 columns"):
        cw.fit(A)
    assert not calls                                            # refused before any collective

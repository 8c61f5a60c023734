"""Centred Lanczos fits (sapca_options.lanczos_center, opt-in): SVDMethod.Lanczos with center(True) factors A_c = A - 1 mu^T
instead of the raw matrix (the reference's quirk Q1, still the default).

Reference everywhere: numpy.linalg.svd of D - D.mean(0) in f64, D the dense matrix of the values as stored (f32-rounded where
the fit is f32), and scikit-learn's PCA on the same D.  Tolerances are the Lanczos tolerances of tests/test_gpu_parity.py:
f64 sigma rtol 1e-5 (= kappa) and subspace angle < 1e-4; f32 inputs sigma 2e-4 and angle 2e-3."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import sapca
import sapca_oracle as O
from sapca import _lib as L
from sapca import synth
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

TOL = {np.float64: (1e-5, 1e-4), np.float32: (2e-4, 2e-3)}     # dtype -> (sigma rtol, subspace angle)


def _csr_np(t):
    ptr, idx, val = (x.cpu().numpy() for x in t)
    return ptr.astype(np.int64), idx.astype(np.int64), val


def _host(m, n, dens, k, seed, dtype=np.float64, generate_f64=False):
    """synth.gapped_csr(..., centred=True) as a host CSR (generate_f64: drawn in f64 and rounded, as the random
    configurations of test_gpu_parity.py are)"""
    t = torch.float64 if dtype == np.float64 or generate_f64 else torch.float32
    ptr, idx, val = _csr_np(synth.gapped_csr(m, n, dens, k, seed=seed, centred=True, dtype=t))
    return sp.csr_matrix((val.astype(dtype), idx, ptr), shape=(m, n))


def _device(A):
    """a host CSR as the device-resident matrix the estimators take"""
    t = torch.float64 if A.dtype == np.float64 else torch.float32
    return sapca.DeviceCsr(torch.from_numpy(A.indptr.astype(np.int64)).cuda(), torch.from_numpy(A.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(A.data).to(t).cuda(), A.shape)


def _exact(D, k):
    """(sigma, Vt, sigma_k / sigma_k+1) of the centred dense matrix"""
    D = np.asarray(D, dtype=np.float64)
    _, s, vt = np.linalg.svd(D - D.mean(0), full_matrices=False)
    return s, vt, s[k - 1] / s[k]


def _build(k, mask=None, centred=True, **kw):
    b = sapca.SparsePCABuilder.new() if mask is None else sapca.MaskedSparsePCABuilder.new().mask(mask)
    b = b.n_components(k).svd_method(SVDMethod.Lanczos())
    if centred:
        b = b.lanczos_center()
    for name, v in kw.items():
        b = getattr(b, name)(v)
    return b.build()


def _check_against_exact(est, D, k, dtype, label=""):
    srel, ang = TOL[dtype]
    s, vt, gap = _exact(D, k)
    got_s, c = est.singular_values_(np.float64), est.components_(np.float64)
    angle = O.subspace_angle(c, vt[:k])
    print(f"{label}: gap {gap:.3f}  max sigma rel err {np.max(np.abs(got_s - s[:k]) / s[:k]):.3e}  angle {angle:.3e}"
          f"  steps {est.timings().lanczos_steps}")
    np.testing.assert_allclose(got_s, s[:k], rtol=srel)
    assert angle < ang, (label, angle)
    return s, vt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_centred_lanczos_against_the_exact_svd(dtype):
    from sklearn.decomposition import PCA
    m, n, k = 7000, 1100, 6                      # (the scatter route takes it: n <= m, m >= 4096, the columns fit LDS)
    A = _host(m, n, 0.05, k, 17, dtype)
    D = A.toarray().astype(np.float64)
    x = _device(A)
    est = _build(k)
    est.fit(x)
    srel, _ = TOL[dtype]
    s, vt = _check_against_exact(est, D, k, dtype, "scatter route")
    c = est.components_(np.float64)
    np.testing.assert_allclose(np.abs(c @ vt[:k].T), np.eye(k), atol=2e-3)                         # vector by vector
    assert np.all(c[np.arange(k), np.argmax(np.abs(c), 1)] > 0)                                    # svd_flip as ever
    sk = PCA(n_components=k, svd_solver="full").fit(D)
    np.testing.assert_allclose(est.explained_variance_(np.float64), sk.explained_variance_, rtol=2 * srel)   # a variance now
    # the option off: today's uncentred fit (Q1) from the same builder calls, with the same mean_
    raw = _build(k, centred=False)
    raw.fit(x)
    assert np.array_equal(est.mean_(np.float64), raw.mean_(np.float64))
    np.testing.assert_allclose(est.mean_(np.float64), D.mean(0), rtol=1e-5, atol=1e-7)
    assert est.total_variance_() == raw.total_variance_()
    s_raw = np.linalg.svd(D, compute_uv=False)
    np.testing.assert_allclose(raw.singular_values_(np.float64), s_raw[:k], rtol=srel)
    apart = O.subspace_angle(c, raw.components_(np.float64))
    print(f"centred vs uncentred subspace: {apart:.3f} rad")
    assert apart > 0.5                                                                             # (a switch that does something)
    # center(False) and SVDMethod.Random: the option does nothing
    off = _build(k, center=False)
    off.fit(x)
    plain = _build(k, centred=False, center=False)
    plain.fit(x)
    assert np.array_equal(off.components_(np.float64), plain.components_(np.float64))
    assert np.array_equal(off.singular_values_(np.float64), plain.singular_values_(np.float64))


def test_masked_centred_fit():
    m, n, k = 7000, 1100, 6
    A = _host(m, n, 0.05, k, 17)
    mask = synth.bernoulli_mask(n, 0.6, 5).numpy()
    est = _build(k, mask)
    est.fit(_device(A))
    _check_against_exact(est, A.toarray()[:, mask], k, np.float64, "masked, scatter route")
    assert est.components_().shape == (k, int(mask.sum())) and est.mean_().shape == (n,)
    np.testing.assert_allclose(est.mean_(np.float64), A.toarray().mean(0), rtol=1e-12, atol=1e-14)   # full width, all columns


@pytest.mark.parametrize("masked", [False, True])
def test_scatter_route_is_reproducible_and_agrees_with_the_transposed_operator(debug_switches, monkeypatch, masked):
    """the properties of test_lanczos_without_a_transposed_operator for centred fits, at its tolerances"""
    m, n, k = 7000, 1100, 6
    A = _host(m, n, 0.05, k, 17)
    mask = synth.bernoulli_mask(n, 0.6, 5).numpy() if masked else None
    x = _device(A)
    a, b = _build(k, mask), _build(k, mask)
    ta, tb = a.fit_transform(x), b.fit_transform(x)
    assert np.array_equal(a.components_(np.float64), b.components_(np.float64)) and torch.equal(ta, tb)   # bit for bit
    assert np.array_equal(a.singular_values_(np.float64), b.singular_values_(np.float64))
    monkeypatch.setenv("SAPCA_LANCZOS_TRANSPOSE", "1")
    c = _build(k, mask)
    tc = c.fit_transform(x)
    D = A.toarray() if mask is None else A.toarray()[:, mask]
    _check_against_exact(c, D, k, np.float64, "transposed-operator route")
    ds = np.max(np.abs(a.singular_values_(np.float64) / c.singular_values_(np.float64) - 1))
    ang = O.subspace_angle(a.components_(np.float64), c.components_(np.float64))
    print(f"scatter vs transposed: sigma {ds:.3e}  angle {ang:.3e}")
    np.testing.assert_allclose(a.singular_values_(np.float64), c.singular_values_(np.float64), rtol=1e-10)
    assert ang < 1e-8
    np.testing.assert_allclose(ta.cpu().numpy(), tc.cpu().numpy(), atol=1e-8 * float(tc.abs().max()))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fewer_than_4096_rows_take_the_row_kernel(dtype):
    m, n, k = 3500, 700, 6                        # centred gap sigma_6 / sigma_7 = 1.77 (dense SVD, CPU)
    A = _host(m, n, 0.05, k, 11, dtype)
    est = _build(k)
    est.fit(_device(A))
    _check_against_exact(est, A.toarray(), k, dtype, "row kernel")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wide_matrix_iterates_on_the_small_side(dtype):
    """m < n: the iteration runs on A_c A_c^T, where both products and the recovered right vectors carry a correction"""
    m, n, k = 300, 2000, 5
    A = _host(m, n, 0.08, k, 13, dtype)
    est = _build(k)
    est.fit(A)
    _, vt = _check_against_exact(est, A.toarray(), k, dtype, "wide")
    np.testing.assert_allclose(np.abs(est.components_(np.float64) @ vt[:k].T), np.eye(k), atol=2e-3)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_mean_that_dwarfs_the_signal(dtype):
    """twenty dense columns of 1000 (1 + 1e-3 U(-1, 1)): sigma_1(A) = 3.7e5 against sigma_6(A_c) = 403, ||1 mu^T|| / sigma_6 = 927.
    The centring vector has to be f64: rounded to f32 it leaves an operator that is not symmetric to working precision."""
    m, n, k = 7000, 1100, 6
    D = _host(m, n, 0.05, k, 17).toarray()
    D[:, :20] = 1000.0 * (1.0 + 1e-3 * np.random.default_rng(3).uniform(-1.0, 1.0, (m, 20)))
    A = sp.csr_matrix(D.astype(dtype))
    A.sort_indices()
    est = _build(k)
    est.fit(_device(A))
    Ds = A.toarray().astype(np.float64)           # the values as stored
    s, _ = _check_against_exact(est, Ds, k, dtype, "large mean")
    print(f"sigma_1(A) {np.linalg.norm(Ds, 2):.3e}  sigma_k(A_c) {s[k - 1]:.1f}  ||1 mu^T|| / sigma_k {np.sqrt(m) * np.linalg.norm(Ds.mean(0)) / s[k - 1]:.0f}")


def test_sixteen_random_configurations_against_the_exact_svd():
    """the configurations of test_random_lanczos_configurations_against_the_exact_svd drawn anew (rng 900 + seed) on
    matrices with a centred structure: sigma in all of them, the subspace wherever the dense SVD certifies a gap of 1.5
    (fourteen of them; seeds 10 and 13 have gaps of 1.04 and 1.02)"""
    no_angle, kinds = [], set()
    for seed in range(16):
        rng = np.random.default_rng(900 + seed)
        k = int(rng.integers(1, 9))
        m, n = int(rng.integers(60, 1800)), int(rng.integers(40, 1500))
        dens = float(rng.uniform(0.03, 0.25))
        masked, f32 = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        dtype = np.float32 if f32 else np.float64
        A = _host(m, n, dens, k, seed, dtype, generate_f64=True)
        mask = synth.bernoulli_mask(n, 0.7, seed).numpy() if masked else np.ones(n, bool)
        D = A.toarray().astype(np.float64)[:, mask]
        assert min(D.shape) >= k + 2, seed
        est = _build(k, mask if masked else None)
        est.fit(A)
        s, vt, gap = _exact(D, k)
        srel, ang = TOL[dtype]
        got = est.singular_values_(np.float64)
        angle = O.subspace_angle(est.components_(np.float64), vt[:k])
        print(f"seed {seed}: {m} x {D.shape[1]} k {k} {'masked ' if masked else ''}{'f32' if f32 else 'f64'}  gap {gap:.3f}"
              f"  sigma {np.max(np.abs(got - s[:k]) / s[:k]):.3e}  angle {angle:.3e}")
        np.testing.assert_allclose(got, s[:k], rtol=srel, err_msg=f"seed {seed}")
        if gap >= 1.5:
            assert angle < ang, (seed, angle)
        else:
            no_angle.append(seed)
        kinds.add(("tall" if D.shape[1] <= m else "wide", masked, f32))
    assert len(no_angle) <= 2, no_angle
    assert {t[0] for t in kinds} == {"tall", "wide"} and {t[1] for t in kinds} == {True, False} and {t[2] for t in kinds} == {True, False}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fit_through_projection_is_the_textbook_pca(dtype):
    from sklearn.decomposition import PCA
    m, n, k = 7000, 1100, 6
    A = _host(m, n, 0.05, k, 17, dtype)
    D = A.toarray().astype(np.float64)
    est = _build(k, transform_semantics=L.TRANSFORM_CENTERED)
    t = est.fit_transform(_device(A)).cpu().numpy().astype(np.float64)
    want = (D - est.mean_(np.float64)[None, :]) @ est.components_(np.float64).T
    tol = 1e-8 if dtype == np.float64 else 2e-3
    print(f"projection: max err {np.abs(t - want).max():.3e} of {np.abs(want).max():.3e}")
    np.testing.assert_allclose(t, want, atol=tol * np.abs(want).max())
    # scikit-learn's scores, up to the sign of each column.  Bound: the vector-by-vector agreement asked of the components
    # (2e-3, |C V^T| = I above) carried through the projection
    sk = PCA(n_components=k, svd_solver="full").fit_transform(D)
    sign = np.sign(np.sum(t * sk, axis=0))
    print(f"sklearn scores: max err {np.abs(t - sk * sign).max():.3e} of {np.abs(sk).max():.3e}")
    np.testing.assert_allclose(t, sk * sign, atol=2e-3 * np.abs(sk).max())


def test_sharded_centred_fit_agrees_with_one_handle():
    """at the tolerances of test_masked_lanczos_f64_sharded_inside_the_library: mu and v are replicated, the shift is the
    same number on every rank and the step has the one all-reduce it always had"""
    m, n, k = 6000, 900, 6
    A = _host(m, n, 0.06, k, 9)
    mask = synth.bernoulli_mask(n, 0.6, 7).numpy()
    one = _build(k, mask)
    t1 = one.fit_transform(A)
    _check_against_exact(one, A.toarray()[:, mask], k, np.float64, "one handle")
    md = sapca.MultiDevice(_build(k, mask), [0, 0])
    t = md.fit_transform(A)
    ds = np.max(np.abs(md.singular_values_(np.float64) / one.singular_values_(np.float64) - 1))
    ang = O.subspace_angle(md.components_(np.float64), one.components_(np.float64))
    print(f"sharded vs one handle: sigma {ds:.3e}  angle {ang:.3e}  scores {np.abs(t - t1).max() / np.abs(t1).max():.3e}")
    np.testing.assert_allclose(md.singular_values_(np.float64), one.singular_values_(np.float64), rtol=1e-8)
    assert ang < 1e-6
    np.testing.assert_allclose(t, t1, atol=1e-7 * np.abs(t1).max())
    assert np.array_equal(md.member(1).components_(np.float64), md.member(0).components_(np.float64))

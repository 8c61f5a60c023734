"""The product kernels of a Lanczos fit (csrc/lanczos.hip) and the fixed-point scatter route (csrc/scatter.hip) at their edges.

SVDMethod.Lanczos chooses between five product kernels and the scatter route by shape alone; the matrices of
tests/lanczos_cases.py (held to their conditions on the CPU by tests/test_lanczos_cases_cpu.py) send a small fit through each of
them, on rows that are long enough for the four-at-a-time entry loop (193 entries) and that end at every remainder count.

Every fit is checked
  * against the f64 host reference of its operator, at the tolerances of tests/test_gpu_lanczos_centred.py (TOL): sigma rtol
    1e-5 (f64) / 2e-4 (f32), subspace angle 1e-4 / 2e-3, |C V^T| = I to 2e-3;
  * against the same fit on another route, at the bounds of test_lanczos_without_a_transposed_operator (ROUTE): sigma rtol
    1e-10 / 1e-6, angle 1e-8 / 1e-5, fit_transform scores to 1e-8 / 1e-3 of their maximum -- this is the comparison that
    notices a single dropped entry;
  * on a scatter route, two fits give the same bytes;
  * timings().lanczos_steps >= k.
The debug build reads its SAPCA_SPMV_* switches once per fit, so one process can walk the routes."""
import collections

import numpy as np
import pytest
import torch

import lanczos_cases as C
import sapca
import sapca_oracle as O
from sapca import _lib as L
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

TOL = {np.float64: (1e-5, 1e-4), np.float32: (2e-4, 2e-3)}                  # dtype -> (sigma rtol, subspace angle)
ROUTE = {np.float64: (1e-10, 1e-8, 1e-8), np.float32: (1e-6, 1e-5, 1e-3)}   # dtype -> (sigma rtol, angle, scores / max)
SWITCHES = ("SAPCA_SPMV_NO_LDS", "SAPCA_SPMV_NO_SLICE_GRID", "SAPCA_SPMV_IDX32", "SAPCA_LANCZOS_TRANSPOSE")
BOTH = [np.float64, np.float32]

Fit = collections.namedtuple("Fit", "sigma comps scores mean total_var steps label")


def _device(A, dtype):
    t = torch.float64 if dtype == np.float64 else torch.float32
    return sapca.DeviceCsr(torch.from_numpy(A.indptr.astype(np.int64)).cuda(), torch.from_numpy(A.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(A.data).to(t).cuda(), A.shape)


def _estimator(name, centred=False):
    mask = C.mask_of(name)
    b = sapca.SparsePCABuilder.new() if mask is None else sapca.MaskedSparsePCABuilder.new().mask(mask)
    b = b.n_components(C.k_of("LIM" if name == "LIM+1" else name)).svd_method(SVDMethod.Lanczos())
    return (b.lanczos_center() if centred else b).build()


def _fit(monkeypatch, name, dtype, *switches, centred=False, x=None):
    """one fit_transform of the case with exactly the given switches set (they need the debug_switches fixture)"""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s in switches:
        assert s in SWITCHES
        monkeypatch.setenv(s, "1")
    est = _estimator(name, centred)
    t = est.fit_transform(x if x is not None else _device(C.matrix(name, centred, dtype == np.float32), dtype))
    label = f"{name}{' centred' if centred else ''} {np.dtype(dtype).name} [{' '.join(s[6:] for s in switches) or 'default'}]"
    return Fit(est.singular_values_(np.float64), est.components_(np.float64), t.cpu().numpy().astype(np.float64),
               est.mean_(np.float64), est.total_variance_(), int(est.timings().lanczos_steps), label)


def _against_reference(f, name, dtype, centred=False):
    k = f.sigma.size
    s, vt, gap = C.reference(name, centred, dtype == np.float32)
    srel, ang = TOL[dtype]
    angle = O.subspace_angle(f.comps, vt)
    print(f"{f.label}: gap {gap:.3f}  sigma rel err {np.max(np.abs(f.sigma - s[:k]) / s[:k]):.3e}  angle {angle:.3e}"
          f"  |CV^T|-I {np.abs(np.abs(f.comps @ vt.T) - np.eye(k)).max():.3e}  steps {f.steps}")
    assert f.steps >= k
    np.testing.assert_allclose(f.sigma, s[:k], rtol=srel, err_msg=f.label)
    assert angle < ang, (f.label, angle)
    np.testing.assert_allclose(np.abs(f.comps @ vt.T), np.eye(k), atol=2e-3, err_msg=f.label)


def _same_fit(a, b, dtype):
    srel, ang, trel = ROUTE[dtype]
    angle = O.subspace_angle(a.comps, b.comps)
    tmax = np.abs(b.scores).max()
    print(f"{a.label} vs {b.label}: sigma {np.max(np.abs(a.sigma / b.sigma - 1)):.3e}  angle {angle:.3e}"
          f"  scores {np.abs(a.scores - b.scores).max() / tmax:.3e} of their maximum")
    np.testing.assert_allclose(a.sigma, b.sigma, rtol=srel, err_msg=f"{a.label} vs {b.label}")
    assert angle < ang, (a.label, b.label, angle)
    np.testing.assert_allclose(a.scores, b.scores, atol=trel * tmax, err_msg=f"{a.label} vs {b.label}")


def _same_bytes(a, b):
    assert np.array_equal(a.comps, b.comps) and np.array_equal(a.sigma, b.sigma) and np.array_equal(a.scores, b.scores), a.label
    assert np.array_equal(a.mean, b.mean) and a.total_var == b.total_var, a.label


def _routes(monkeypatch, name, dtype, variants, centred=False, scatter=False):
    """the default fit against its reference, then every variant (a tuple of switches) against its reference and the default"""
    x = _device(C.matrix(name, centred, dtype == np.float32), dtype)
    base = _fit(monkeypatch, name, dtype, centred=centred, x=x)
    _against_reference(base, name, dtype, centred)
    if scatter:
        _same_bytes(base, _fit(monkeypatch, name, dtype, centred=centred, x=x))
    for sw in variants:
        f = _fit(monkeypatch, name, dtype, *sw, centred=centred, x=x)
        _against_reference(f, name, dtype, centred)
        _same_fit(f, base, dtype)
    return base


@pytest.mark.parametrize("dtype", BOTH)
def test_long_rows_with_x_in_lds_and_a_scattered_second_product(debug_switches, monkeypatch, dtype):
    """L (4200 x 1500, 247-352 entries a row and the edited lengths 0 .. 513, 1500), default: spmv_ldsx_kernel<T, uint16_t>, then
    spmvt_scatter_kernel<T, uint16_t> + spmvt_reduce_kernel, the four-wide loop and its (a0 + a1) + (a2 + a3) fold in both.
    IDX32: the int32_t instantiations of both.  NO_LDS: spmv_kernel, then the scatter with 4-byte columns.  LANCZOS_TRANSPOSE:
    spmv_ldsx_kernel on A, spmv_sliced_kernel with one slice on A^T (1500 x 4200, 840 entries a row)."""
    _routes(monkeypatch, "L", dtype, [("SAPCA_SPMV_IDX32",), ("SAPCA_SPMV_NO_LDS",), ("SAPCA_LANCZOS_TRANSPOSE",)], scatter=True)


@pytest.mark.parametrize("dtype", BOTH)
def test_fewer_than_4096_rows_take_the_sliced_kernel_with_one_slice(debug_switches, monkeypatch, dtype):
    """S (3000 x 1200, 218-312 entries a row and the edited lengths): no LDS-x kernel and no scatter below 4096 rows; both
    products take spmv_sliced_kernel with one slice and one row per wave (A^T: 1200 x 3000, 660 entries a row).
    NO_LDS: spmv_kernel for both, the route-independent reference of the long-row loops."""
    _routes(monkeypatch, "S", dtype, [("SAPCA_SPMV_NO_LDS",)])


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("dtype", BOTH)
def test_wide_matrix_on_the_slice_grid(debug_switches, monkeypatch, dtype, centred):
    """W2 (4200 x 20000, 213-329 entries a row, the edited lengths, a row with entries at columns 9999 | 10000), iteration on
    A A^T: A^T v on spmv_ldsx_kernel<T, uint16_t> (20000 x 4200; centred: with shift and rowscale = mu), A t on
    spmv_slice_grid_kernel<T, true> with two slices of 10000 + slice_sum_kernel (centred: with its shift).
    IDX32: spmv_ldsx_kernel<T, int32_t> and spmv_slice_grid_kernel<T, false>.  NO_SLICE_GRID: spmv_sliced_kernel with two slices
    and two rows per wave.  NO_LDS: spmv_kernel for both."""
    assert C.spmv_kind(4200, 20000, C.matrix("W2", centred).nnz, True) == "slice_grid" and C.sliced_rpw(4200) == 2
    _routes(monkeypatch, "W2", dtype, [("SAPCA_SPMV_IDX32",), ("SAPCA_SPMV_NO_SLICE_GRID",), ("SAPCA_SPMV_NO_LDS",)], centred=centred)


def test_three_slices_the_last_one_shorter(debug_switches, monkeypatch):
    """W3 (4200 x 40000): spmv_slice_grid_kernel<double, true> with slices of 13334, 13334 and 13332 columns.  NO_SLICE_GRID:
    spmv_sliced_kernel with three slices (a table of 2 x 4 run limits per wave)."""
    assert C.slices_of(40000) == (13334, 3)
    _routes(monkeypatch, "W3", np.float64, [("SAPCA_SPMV_NO_SLICE_GRID",), ("SAPCA_SPMV_NO_LDS",)])


def test_tall_matrix_on_the_scatter_route_and_with_a_sliced_transposed_operator(debug_switches, monkeypatch):
    """T (20000 x 5000, 225-366 entries a row and the edited lengths), default: spmv_ldsx_kernel + the scatter at about five rows
    per wave of the 4096.  LANCZOS_TRANSPOSE: A^T is 5000 x 20000 (1200 entries a row): spmv_slice_grid_kernel<double, true>
    with two slices on an operator of more rows; with NO_SLICE_GRID as well: spmv_sliced_kernel, two rows per wave, 2 x 3 limits."""
    _routes(monkeypatch, "T", np.float64, [("SAPCA_LANCZOS_TRANSPOSE",), ("SAPCA_LANCZOS_TRANSPOSE", "SAPCA_SPMV_NO_SLICE_GRID"),
                                           ("SAPCA_LANCZOS_TRANSPOSE", "SAPCA_SPMV_NO_LDS")], scatter=True)


# ------------------------------------------------------------------ the statistics of the scatter route
def _statistics_bounds(A, dtype, used_cols=None):
    """(exact mean, bound), (exact total variance, bound), exact counts -- see test_scatter_statistics_against_exact_sums"""
    m, n = A.shape
    S, Q, cnt, _ = C.exact_column_sums(A)
    amax = np.abs(A.data).max()
    u, slack = 2.0 ** -53, 1.0 + 2.0 ** -50
    Es = (cnt * (m * amax * 2.0 ** -61) * slack + u * np.abs(S))
    Eq = (cnt * (m * amax * amax * 2.0 ** -61) * slack + 2 * u * Q)
    uT = 0.0 if dtype == np.float64 else 2.0 ** -24
    mean = S / m
    mean_bound = ((1 + uT) * (Es + u * (np.abs(S) + Es)) + (uT + u) * np.abs(S)) / m
    ms = S * S / m
    Ems = (2 * np.abs(S) * Es + Es * Es) / m + 2 * u * slack * (np.abs(S) + Es) ** 2 / m
    var = (Q - ms) / (m - 1)
    var_bound = (Eq + Ems + 2 * u * (Q + Eq + ms + Ems)) / (m - 1) * slack + 4 * u * (Q + ms) / (m - 1)
    if used_cols is not None:
        var, var_bound = var[used_cols], var_bound[used_cols]
    total = float(np.sum(var))
    total_bound = float(np.sum(var_bound) + 2 * (var.size + 1) * u * np.sum(np.abs(var) + var_bound))
    return (mean, mean_bound), (total, total_bound), cnt


def _check_statistics(f, A, dtype, used_cols=None):
    (mean, mb), (tv, tb), cnt = _statistics_bounds(A, dtype, used_cols)
    err = np.abs(f.mean - mean)
    worst = float(np.max(err / np.where(mb > 0, mb, 1.0)))
    print(f"{f.label}: mean: largest error / bound {worst:.3f} (largest error {err.max():.3e})"
          f"  total variance {f.total_var!r}: error / bound {abs(f.total_var - tv) / tb:.3f} (bound {tb:.3e}, relative {tb / tv:.2e})")
    assert np.all(err <= mb), (f.label, int(np.argmax(err - mb)), worst)
    assert np.all(f.mean[cnt == 0] == 0.0)
    assert abs(f.total_var - tv) <= tb, (f.label, f.total_var, tv, tb)
    return err, mb, cnt


@pytest.mark.parametrize("name,dtype", [("P2", np.float64), ("P2", np.float32), ("P3m", np.float64), ("P3m", np.float32),
                                        ("L", np.float64), ("L", np.float32)])
def test_scatter_statistics_against_exact_sums(debug_switches, monkeypatch, name, dtype):
    """mean_ and total_variance_() of a fit on the scatter route against exact host sums (math.fsum per column) of the CSR arrays.
    P2 (8192 x 7700): colstats_scatter_kernel in two passes of 3850 columns cut by colrange_bounds_kernel; P3m (4200 x 16000 under
    a mask that keeps 4013): three passes of 5334 over ALL columns while the fit sees the kept ones; L: one pass.  Entries sit in
    the columns either side of every pass boundary and in column n - 1; column 1234 and one row are empty.

    The bound, from scatter.hip (not measured).  fixed_scale puts rows * amax * scale in [2^60, 2^61): one unit is at most
    rows * amax * 2^-60, every term is rounded to nearest (half a unit), the integer total is converted once.  With cnt_c the
    stored entries of column c, S_c and Q_c its exact sum and sum of squares, u = 2^-53:
        |sum_c - S_c|   <= Es_c = cnt_c rows amax 2^-61 + u |S_c|
        |sumsq_c - Q_c| <= Eq_c = cnt_c rows amax^2 2^-61 + 2u Q_c          (u more: the rounding of v * v)
    and through finish_statistics (mean = T(sum / m); var_c = (sumsq - (sum / m) sum) / (m - 1), summed over the used columns):
        |mean_c - S_c / m| <= ((1 + uT)(Es_c + u (|S_c| + Es_c)) + (uT + u) |S_c|) / m       uT = 2^-24 for f32 fits, 0 for f64
        |(sum / m) sum - S_c^2 / m| <= Ems_c = (2 |S_c| Es_c + Es_c^2) / m + 2u (|S_c| + Es_c)^2 / m
        |var_c - (Q_c - S_c^2 / m) / (m - 1)| <= (Eq_c + Ems_c + 2u (Q_c + Eq_c + S_c^2 / m + Ems_c)) / (m - 1)
                                                 + 4u (Q_c + S_c^2 / m) / (m - 1)             (the last: this reference in f64)
        |total - sum_c var_c| <= sum_c of the above + 2 (n_used + 1) u sum_c (|var_c| + bound_c)   (two f64 summations)
    each with a factor 1 + 2^-50 for the rounding of rows * amax itself.  An empty column is exactly 0.  The per-column entry
    counts have no accessor; the unmasked projection reads them (t = sum over stored entries of (a - mean_c) V_c), so P2's and L's
    scores are held to that sum at the 1e-8 / 1e-3 of test_g6_lanczos_uncentred: one entry miscounted in one column moves a score
    by mean_c |V_c|, 1e-5 of their maximum here."""
    A = C.matrix(name, False, dtype == np.float32)
    mask = C.mask_of(name)
    m, n = A.shape
    assert C.scatter_route(m, C.used(name).shape[1], C.used(name).nnz)
    f = _fit(monkeypatch, name, dtype)
    _against_reference(f, name, dtype)
    _same_bytes(f, _fit(monkeypatch, name, dtype))
    _check_statistics(f, A, dtype, None if mask is None else np.flatnonzero(mask))
    if name != "L":     # (L's other routes: test_long_rows_with_x_in_lds_and_a_scattered_second_product)
        g = _fit(monkeypatch, name, dtype, "SAPCA_LANCZOS_TRANSPOSE")
        _against_reference(g, name, dtype)
        _same_fit(f, g, dtype)
    if mask is None:
        want = O.transform_sparse(A.indptr, A.indices.astype(np.int64), A.data, m, n, f.comps, f.mean, True)
        terr = np.abs(f.scores - want).max() / np.abs(want).max()
        print(f"{f.label}: scores against the entry-wise sum: {terr:.3e} of their maximum")
        assert terr <= ROUTE[dtype][2]


def test_scatter_statistics_resolution_is_absolute(debug_switches, monkeypatch):
    """What the route promises (include/sapca.h): L with columns 0..9 scaled by 1e-9 and one entry of 1e3.  The sums of the small
    columns meet the same ABSOLUTE bound, cnt_c rows amax 2^-61 = 1.8e-12 a column at sums near 5e-8: far looser in relative
    terms (printed) than the f64 sums of the transposed route, which are held to 2^-53 cnt_c sum |a| on the same matrix."""
    A = C.matrix("Lsmall")
    m, n = A.shape
    f = _fit(monkeypatch, "Lsmall", np.float64)
    err, mb, cnt = _check_statistics(f, A, np.float64)
    S, _, _, sabs = C.exact_column_sums(A)
    small = np.arange(10)
    print(f"small columns: mean error relative to the mean {np.max(err[small] / np.abs(S[small] / m)):.3e}"
          f"  (bound, relative {np.max(mb[small] / np.abs(S[small] / m)):.3e})")
    g = _fit(monkeypatch, "Lsmall", np.float64, "SAPCA_LANCZOS_TRANSPOSE")
    gerr = np.abs(g.mean * m - S)
    gb = 2.0 ** -53 * cnt * sabs + 2.0 ** -52 * np.abs(S)      # (the sum; then the division by m and the product above)
    print(f"transposed route: largest sum error / bound {np.max(gerr / np.where(gb > 0, gb, 1.0)):.3e}"
          f"  small columns relative {np.max(gerr[small] / np.abs(S[small])):.3e}")
    assert np.all(gerr <= gb)


def test_x_exactly_at_the_lds_limit(debug_switches, monkeypatch):
    """LIM (19264 x 19200, k = 2): n_used * 8 is exactly the 150 KiB of spmv_ldsx_kernel and of the scatter's output copy, the
    statistics take three passes of 6400.  Sigma against svds and against the transposed route; the statistics as above.
    Its neighbour (the same matrix and a 19201st column holding one entry of 2^-20: by Weyl's inequality sigma^2 moves by at most
    2^-40, 1e-16 of it) no longer fits: spmv_sliced_kernel with two slices and five rows per wave on A, spmv_slice_grid_kernel on
    A^T, and the same sigma to the route-vs-route bound."""
    A = C.matrix("LIM")
    m, n = A.shape
    assert n == C.LDS_X_COLS and C.scatter_route(m, n, A.nnz) and not C.scatter_route(m, n + 1, A.nnz + 1)
    assert C.products(m, n + 1, A.nnz + 1) == ("sliced", "slice_grid") and C.sliced_rpw(m) == 5
    f = _fit(monkeypatch, "LIM", np.float64)
    _against_reference(f, "LIM", np.float64)
    _same_bytes(f, _fit(monkeypatch, "LIM", np.float64))
    _check_statistics(f, A, np.float64)
    g = _fit(monkeypatch, "LIM", np.float64, "SAPCA_LANCZOS_TRANSPOSE")
    _same_fit(g, f, np.float64)
    h = _fit(monkeypatch, "LIM+1", np.float64)
    print(f"{h.label}: sigma against the 19200-column fit {np.max(np.abs(h.sigma / f.sigma - 1)):.3e}  steps {h.steps}")
    assert h.steps >= 2
    np.testing.assert_allclose(h.sigma, f.sigma, rtol=ROUTE[np.float64][0])
    assert O.subspace_angle(h.comps[:, :n], f.comps) < ROUTE[np.float64][1]


def test_unsorted_rows_on_the_multi_pass_statistics_give_numbers_not_stray_accesses():
    """include/sapca.h: rows whose columns do not ascend give wrong numbers, not stray accesses.  P2 with three rows reversed end
    to end: with two statistics passes the run limits of colrange_bounds_kernel then enclose columns of the other pass, which
    colstats_scatter_kernel skips (they would index LDS outside the workgroup's arrays).  The fit returns or refuses, and the same
    handle then fits the sound matrix to the bytes of a fresh handle."""
    A = C.matrix("P2")
    m, n = A.shape
    idx, val = A.indices.astype(np.int32).copy(), A.data.copy()
    for r in (17, 4242, m - 1):
        lo, hi = A.indptr[r], A.indptr[r + 1]
        assert hi - lo > 8
        idx[lo:hi], val[lo:hi] = idx[lo:hi][::-1].copy(), val[lo:hi][::-1].copy()
    ptr = torch.from_numpy(A.indptr.astype(np.int64)).cuda()
    bad = sapca.DeviceCsr(ptr, torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda(), (m, n))
    good = _device(A, np.float64)
    est = _estimator("P2")
    try:
        t_bad = est.fit_transform(bad)
        assert t_bad.shape == (m, C.K)
        torch.cuda.synchronize()
    except L.SapcaError as e:   # (a refusal would be fine too)
        assert e.status in (L.ERR_ARG, L.ERR_SVD)
    fresh = _estimator("P2")
    t_ref = fresh.fit_transform(good)
    t_again = est.fit_transform(good)
    assert torch.equal(t_again, t_ref)
    assert np.array_equal(est.components_(np.float64), fresh.components_(np.float64))
    assert np.array_equal(est.mean_(np.float64), fresh.mean_(np.float64)) and est.total_variance_() == fresh.total_variance_()

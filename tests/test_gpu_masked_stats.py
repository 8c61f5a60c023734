"""Masked and chunk statistics on a device-resident matrix (-m gpu): sapca_masked_stats_csr_device_* and the Python
ResidentCsr methods (nonzero_/sum_/var_{col,row}_masked, the *_chunk family) against the host restatement in
masked_stats_ref.py.

Bars: counts exact; sums within 1e-12 relative; variances within 1e-12 relative to max(1, sumsq / count) (the column
formula cancels); COLUMN sums bit-identical from call to call and equal to a per-column math.fsum of the kept entries."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import masked_stats_ref as M
import sapca
import sapca_oracle as O
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu


def _resident(A, sess=None):
    sess = sess or ops.Session()
    A = A.tocsr()
    A.sort_indices()
    return sess, sess.upload(A.indptr, A.indices, A.data, A.shape[0], A.shape[1])


def _mixed(m, n, density, seed, dtype):
    """stored explicit zeros, negative values, an empty row and an empty column"""
    rng = np.random.default_rng(seed)
    D = (rng.random((m, n)) < density) * rng.normal(1.5, 4.0, (m, n))
    stored = (D != 0) | (rng.random((m, n)) < 0.01)
    stored[7, :] = False
    stored[:, 3] = False
    r, c = np.nonzero(stored)
    A = sp.csr_matrix((D[r, c].astype(dtype), (r, c)), shape=(m, n))
    A.sort_indices()
    return A


def _arrays(A):
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data


def _check(got, want, what):
    """got / want: (sum, sum_squared, count, var)"""
    s, q, c, v = want
    np.testing.assert_array_equal(got[2], c, err_msg=f"{what}: count")
    np.testing.assert_allclose(got[0], s, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(s).max(initial=0))), err_msg=f"{what}: sum")
    np.testing.assert_allclose(got[1], q, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(q).max(initial=0))), err_msg=f"{what}: sumsq")
    scale = np.maximum(1.0, np.divide(q, c.astype(np.float64), out=np.zeros_like(q), where=c > 0))
    err = np.abs(got[3] - v) / scale
    assert err.max(initial=0) <= 1e-12, f"{what}: var off by {err.max()} (relative to max(1, sumsq / count))"


def _fsum_cols(ptr, idx, val, n, row_mask):
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    keep = row_mask[rows] if row_mask is not None else np.ones(len(val), bool)
    cols, x = idx[keep], np.asarray(val, np.float64)[keep]
    order = np.argsort(cols, kind="stable")
    cols, x = cols[order], x[order]
    bounds = np.searchsorted(cols, np.arange(n + 1))
    sums = np.array([math.fsum(x[bounds[j]:bounds[j + 1]]) for j in range(n)])
    # the squares are summed exactly and rounded once (in f64, x * x itself would round): a rational sum, finite columns
    sq = np.array([float(sum(Fraction(v) ** 2 for v in x[bounds[j]:bounds[j + 1]])) if np.isfinite(sums[j]) else np.inf
                   for j in range(n)])
    return sums, sq


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_every_masked_method_against_the_restatement(dt):
    m, n = 2600, 900
    A = _mixed(m, n, 0.05, 11, dt)
    ptr, idx, val = _arrays(A)
    rng = np.random.default_rng(3)
    row_mask, col_mask = rng.random(m) < 0.5, rng.random(n) < 0.7
    sess, R = _resident(A)
    for direction, mk in ((M.COLUMN, row_mask), (M.ROW, col_mask), (M.COLUMN, None), (M.ROW, None),
                          (M.COLUMN, np.zeros(m, bool)), (M.ROW, np.concatenate([col_mask, np.zeros(5, bool)]))):
        _check(R.masked_stats(direction, mk), M.masked_stats(ptr, idx, val, m, n, direction, mk),
               f"direction {direction}, mask {None if mk is None else int(mk.sum())}")
    for name in M.MASKED:
        mk = row_mask if "_col_" in name else col_mask
        got, want = getattr(R, name)(list(mk)), getattr(M, name)(ptr, idx, val, m, n, mk)
        if "nonzero" in name:
            np.testing.assert_array_equal(got, want, err_msg=name)
        else:
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(want).max())), err_msg=name)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_column_sums_are_exact_and_reproducible(dt):
    m, n = 3000, 1500     # (more than one 1,280-column tile of the accumulators)
    A = _mixed(m, n, 0.04, 5, dt)
    mk = np.random.default_rng(4).random(m) < 0.5
    if dt == np.float64:
        # one more column, whose kept squares sum to 2.5 * 2^-1074 + 2^-1200: the correctly rounded sum is 3 * 2^-1074; rounding
        # the long accumulator to 53 bits first and again into the subnormal range would give 2 * 2^-1074.  A dropped row
        # holds a large value in it.
        tiny = [2.0 ** -537, 2.0 ** -537, 2.0 ** -538, 2.0 ** -538, 2.0 ** -600, 1e100]
        A = sp.hstack([A, sp.csr_matrix((tiny, (np.arange(6), np.zeros(6, int))), shape=(m, 1))], format="csr")
        A.sort_indices()
        mk[:5], mk[5], n = True, False, n + 1
    ptr, idx, val = _arrays(A)
    sess, R = _resident(A)
    a, b = R.masked_stats(M.COLUMN, mk), R.masked_stats(M.COLUMN, mk)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    fs, fq = _fsum_cols(ptr, idx, val, n, mk)
    np.testing.assert_array_equal(a[0], fs)
    np.testing.assert_array_equal(a[1], fq)
    if dt == np.float64:
        ulp = 2.0 ** -1074
        assert fq[-1] == 3 * ulp and a[2][-1] == 5
        np.testing.assert_array_equal(R.sum_col_masked(mk), fs)
        # sumsq / count - mean^2 in f64: 3 ulp / 5 rounds to 1 ulp (2 ulp / 5 would round to 0); mean^2 underflows to 0
        assert R.var_col_masked(mk)[-1] == fq[-1] / 5 - (fs[-1] / 5) ** 2 == ulp


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_row_longer_than_the_register_tile(dt):
    """one row of 110,000 entries: the ROW kernel's second pass re-reads it"""
    n = 120_000
    rng = np.random.default_rng(9)
    lens = [110_000, 0, 5, 1024, 1025, 3000]
    rows = np.concatenate([np.full(k, r) for r, k in enumerate(lens)])
    cols = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens])
    A = sp.csr_matrix((rng.normal(3.0, 2.0, len(cols)).astype(dt), (rows, cols)), shape=(len(lens), n))
    A.sort_indices()
    ptr, idx, val = _arrays(A)
    sess, R = _resident(A)
    col_mask = rng.random(n) < 0.6
    for mk in (col_mask, None):
        _check(R.masked_stats(M.ROW, mk), M.masked_stats(ptr, idx, val, len(lens), n, M.ROW, mk), "long row")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_two_million_columns(dt):
    """a bitset of 2,000,000 columns (250 KB) read from global memory; in f64 the column accumulators would pass 1 GiB,
    so the column direction takes the transposition route"""
    m, n, per_row = 400, 2_000_000, 50
    rng = np.random.default_rng(12)
    rows = np.repeat(np.arange(m), per_row)
    cols = np.concatenate([np.sort(rng.choice(n, per_row, replace=False)) for _ in range(m)])
    A = sp.csr_matrix((rng.normal(0.5, 2.0, len(cols)).astype(dt), (rows, cols)), shape=(m, n))
    A.sort_indices()
    ptr, idx, val = _arrays(A)
    sess, R = _resident(A)
    col_mask, row_mask = rng.random(n) < 0.5, rng.random(m) < 0.5
    _check(R.masked_stats(M.ROW, col_mask), M.masked_stats(ptr, idx, val, m, n, M.ROW, col_mask), "ROW, 2M columns")
    _check(R.masked_stats(M.COLUMN, row_mask), M.masked_stats(ptr, idx, val, m, n, M.COLUMN, row_mask), "COLUMN, 2M columns")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_non_finite_values_kept_propagate_and_dropped_change_nothing(dt):
    m, n = 300, 200
    A = _mixed(m, n, 0.1, 21, dt).tolil()
    A[10, 5], A[11, 6], A[12, 7] = np.inf, np.nan, 1.0       # row 10 kept (inf in column 5), row 11 dropped (nan in 6)
    A[13, 6] = 2.0
    A = A.tocsr()
    A.sort_indices()
    ptr, idx, val = _arrays(A)
    row_mask = np.ones(m, bool)
    row_mask[11] = False
    sess, R = _resident(A)
    s, q, c, v = R.masked_stats(M.COLUMN, row_mask)
    assert s[5] == np.inf and q[5] == np.inf and np.isnan(v[5])
    assert np.isfinite(s[6]) and np.isfinite(v[6])
    fs, fq = _fsum_cols(ptr, idx, val, n, row_mask)
    finite = np.isfinite(fs)
    assert finite.sum() == n - 1
    np.testing.assert_array_equal(s[finite], fs[finite])                 # the other columns keep their exact sums
    np.testing.assert_array_equal(q[finite], fq[finite])
    np.testing.assert_array_equal(c, M.masked_stats(ptr, idx, val, m, n, M.COLUMN, row_mask)[2])
    # ROW: an inf in a kept column, a nan in a dropped one
    col_mask = np.ones(n, bool)
    col_mask[6] = False
    s, q, c, v = R.masked_stats(M.ROW, col_mask)
    assert s[10] == np.inf and np.isnan(v[10])
    w = M.masked_stats(ptr, idx, val, m, n, M.ROW, col_mask)
    ok = np.arange(m) != 10
    _check(tuple(x[ok] for x in (s, q, c, v)), tuple(x[ok] for x in w), "ROW with non-finite values")


def test_no_mask_equals_an_all_true_mask():
    A = _mixed(1200, 700, 0.06, 2, np.float32)
    sess, R = _resident(A)
    for direction, k in ((M.COLUMN, 1200), (M.ROW, 700)):
        a, b = R.masked_stats(direction), R.masked_stats(direction, np.ones(k, bool))
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def test_errors():
    A = _mixed(40, 30, 0.2, 1, np.float64)
    sess, R = _resident(A)
    for direction, k, msg in ((M.COLUMN, 39, "Mask length (39) is less than number of rows (40)"),
                              (M.ROW, 29, "Mask length (29) is less than number of columns (30)")):
        with pytest.raises(L.SapcaError) as e:
            R.masked_stats(direction, np.ones(k, bool))
        assert str(e.value) == msg and e.value.status == L.ERR_ARG
    with pytest.raises(L.SapcaError, match="direction") as e:
        R.masked_stats(2)
    assert e.value.status == L.ERR_ARG
    with pytest.raises(ValueError, match="less than number of rows"):
        R.sum_col_masked([True] * 39)
    with pytest.raises(ValueError, match="column 29"):
        R.min_max_col_chunk((np.zeros(29), np.zeros(30)))
    np.testing.assert_array_equal(R.masked_stats(M.COLUMN)[2], np.bincount(A.indices, minlength=30))   # the handle still works


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_every_chunk_method_against_the_restatement(dt):
    m, n = 900, 400
    A = _mixed(m, n, 0.08, 8, dt)
    ptr, idx, val = _arrays(A)
    sess, R = _resident(A)
    rng = np.random.default_rng(1)
    refs = {"nonzero_col_chunk": rng.integers(0, 9, n - 5).astype(np.uint64), "nonzero_row_chunk": rng.integers(0, 9, m + 3).astype(np.uint64),
            "sum_col_chunk": rng.normal(size=n + 4), "sum_row_chunk": rng.normal(size=m + 2), "var_col_chunk": np.zeros(n),
            "var_row_chunk": np.zeros(m), "min_max_col_chunk": (rng.normal(0, 3, n).astype(dt), rng.normal(0, 3, n).astype(dt)),
            "min_max_row_chunk": (rng.normal(0, 3, m).astype(dt), rng.normal(0, 3, m).astype(dt))}
    for name in M.CHUNK:
        ref = refs[name]
        mine = tuple(a.copy() for a in ref) if isinstance(ref, tuple) else ref.copy()
        want = tuple(a.copy() for a in ref) if isinstance(ref, tuple) else ref.copy()
        got = getattr(R, name)(mine)
        assert got is mine
        getattr(M, name)(ptr, idx, val, m, n, want)
        for g, w in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
            if g.dtype.kind == "u" or "min_max" in name:
                np.testing.assert_array_equal(g, w, err_msg=name)
            else:
                np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(w).max())), err_msg=name)


def test_chunk_accumulation_over_row_blocks_equals_the_whole_matrix():
    m, n = 3000, 800
    A = _mixed(m, n, 0.05, 30, np.float32)
    sess, W = _resident(A)
    want_cnt, want_sum = W.nonzero_col_chunk(np.zeros(n, np.uint64)), W.sum_col_chunk(np.zeros(n))
    want_mm = W.min_max_col_chunk((np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)))
    cnt, sm = np.zeros(n, np.uint64), np.zeros(n)
    mm = (np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32))
    for lo, hi in ((0, 1000), (1000, 1700), (1700, m)):
        s2, B = _resident(A[lo:hi], ops.Session())
        B.nonzero_col_chunk(cnt)
        B.sum_col_chunk(sm)
        B.min_max_col_chunk(mm)
    np.testing.assert_array_equal(cnt, want_cnt)
    np.testing.assert_allclose(sm, want_sum, rtol=1e-14, atol=1e-12)
    np.testing.assert_array_equal(mm[0], want_mm[0])
    np.testing.assert_array_equal(mm[1], want_mm[1])


def test_a_following_fit_is_unchanged():
    m, n = 3000, 600
    A = _mixed(m, n, 0.08, 6, np.float32)
    sess, R = _resident(A)
    out = [torch.empty((m, 50), dtype=torch.float32, device="cuda") for _ in range(2)]

    def fit_transform(o):
        L.check(sess._h, L.load().sapca_fit_transform_csr_device_f32(*R._args(), C.c_void_p(o.data_ptr())))
        torch.cuda.synchronize()

    fit_transform(out[0])
    rm, cm = np.random.default_rng(0).random(m) < 0.5, np.random.default_rng(1).random(n) < 0.5
    for direction, mk in ((M.COLUMN, rm), (M.ROW, cm), (M.COLUMN, None), (M.ROW, None)):
        R.masked_stats(direction, mk)
    R.var_col_chunk(np.zeros(n))
    fit_transform(out[1])
    a, b = out[0].cpu().numpy(), out[1].cpu().numpy()
    np.testing.assert_allclose(b, a, rtol=0, atol=1e-5 * float(np.abs(a).max()))


def test_end_to_end_mito_fraction_then_gene_filter_then_masked_pca():
    """upload -> normalize -> log1p -> mito fraction (sum_row_masked / sum_row) -> cell mask -> var_col_masked over the kept
    cells -> gene mask -> MaskedSparsePCA on the resident arrays; masks against the host restatement, fit against O.fit"""
    m, n, k, p, q, top = 4000, 900, 8, 6, 2, 300
    ptr, idx, val = (x.cpu().numpy() for x in synth.gapped_csr(m, n, 0.05, k, seed=21, dtype=torch.float32))
    ptr, idx = ptr.astype(np.int64), idx.astype(np.int64)
    sess, R = _resident(sp.csr_matrix((val, idx, ptr), shape=(m, n)))
    R.normalize(R.stats(ops.ROW)[0], 1e3, ops.ROW).log1p()
    mito = np.zeros(n, bool)
    mito[:40] = True                                               # the "mitochondrial genes"
    frac = R.sum_row_masked(mito) / np.maximum(R.stats(ops.ROW)[0], 1e-30)
    thr = np.quantile(frac, 0.8)
    assert np.abs(frac - thr).min() > 1e-9 * thr                      # no cell sits on the cut
    cells = frac < thr
    gvar = R.var_col_masked(cells)
    genes = np.zeros(n, bool)
    genes[np.argsort(-gvar, kind="stable")[:top]] = True
    # the same on the host, on the values as they are on the device
    v2 = R.values().astype(np.float64)
    rows = np.repeat(np.arange(m), np.diff(ptr))
    rs = np.bincount(rows, weights=v2, minlength=m)
    hfrac = M.sum_row_masked(ptr, idx, v2, m, n, mito) / np.maximum(rs, 1e-30)
    np.testing.assert_allclose(frac, hfrac, rtol=1e-12, atol=1e-15)
    hcells = hfrac < thr
    np.testing.assert_array_equal(cells, hcells)
    hvar = M.var_col_masked(ptr, idx, v2, m, n, hcells)
    order = np.argsort(-hvar, kind="stable")
    assert hvar[order[top - 1]] > hvar[order[top]] * (1 + 1e-6)         # the cut is not a near tie
    want = np.zeros(n, bool)
    want[order[:top]] = True
    np.testing.assert_array_equal(genes, want)
    om = synth.gaussian_panel(top, k + p, 5).numpy()
    est = (sapca.MaskedSparsePCABuilder.new().n_components(k).mask(genes)
           .svd_method(SVDMethod.Random(p, q, PIN.QR)).build().set_omega(om))
    est.fit(R.as_device_csr())
    ref = O.fit(ptr, idx, v2, m, n, n_components=k, n_oversamples=p, n_power_iterations=q, omega=om, mask=genes)
    assert O.subspace_angle(est.components_(np.float64), ref.components) < 1e-4
    np.testing.assert_allclose(est.singular_values_(np.float64), ref.singular_values, rtol=1e-4)

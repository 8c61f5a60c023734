"""Variable genes on the GPU (-m gpu): sapca_hvg_moments_csr_device_*, sapca_loess_f64 and sapca_hvg_csr_device_* against the
host restatement tests/hvg_ref.py.

Bars.
  Moments: n_clipped EQUAL; sum and sum_squared within 1e-12 relative of a per-column math.fsum of the transformed f64 values
  (the bar of test_gpu_masked_stats.py); the same bytes from two calls.
  Loess: the restatement against itself with every window summed in reversed order, per case, measured on the CPU (absolute):
  0 (n5), 5.3e-15 (n64), 1.2e-14 (n65), 3.2e-13 (n4000), 1.42e-12 (half_tied, whose fitted values reach 418), 3.5e-18
  (all_equal).  The device contracts FMAs and reduces in a tree, so every case is allowed 1000 x ITS OWN spread, the spread
  taken as at least one ulp of the case's largest |y| (a spread of 0 at five points says nothing about rounding): 9.5e-13,
  5.3e-12, 1.2e-11, 3.2e-10, 1.42e-9, 1.7e-13.  The spread is measured again where the test runs and the bound is taken from
  that measurement.
  Chain: means and variances 1e-12 relative.  variances_norm: the restatement's reversed-order spread of norm_var, relative,
  measured on the CPU: 5.4e-14 (n = 700), 2.5e-14 (n = 1300) unbatched, 1.6e-13 and 1.3e-13 with three batches; 1000 x the
  spread measured where the test runs is allowed (about 1.6e-10).  dispersions_norm: spread |a - b| / max(1, |a|) 1.9e-14
  (n = 700, f32) .. 1.7e-14 (n = 1300); 1000 x is allowed.  highly_variable, rank and n_batches_hv are EQUAL, at values of
  n_top where the restatement's own order is safe: the relative gap between every two neighbours of the descending norm_var
  order down to the cut, in every batch, is at least 1000 x the bound, or the two columns tie exactly for a reason that holds
  on the device as well (the same stored values in the same rows; or small whole counts of which none is clipped, with equal
  sums and sums of squares: such sums are exact in any order, and everything behind them is a function of the two).  Measured on the CPU: gaps across the cut 1.9e-4 .. 5.8e-3
  unbatched and 3.5e-5 .. 4.3e-3 batched at n_top = 50, 100, 150; smallest neighbour gap 2.4e-6.  The test computes and
  asserts them, so a change of the fixture cannot hide a mismatch.  n_top = 200 is not among the values: in the third batch of
  the 700-column fixture the columns at positions 200 and 201 of the order tie exactly (gap across the cut 0), so the cut there
  rests on the index alone and shows nothing; 150 takes its place and no value is skipped."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import hvg_ref as R
import sapca
from sapca import _lib as L
from sapca import ops
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

M = 1500
SEEDS = {700: 131, 1300: 132}
K = 3
SPAN = 0.3
CASES = [(700, np.float32), (700, np.float64), (1300, np.float32), (1300, np.float64)]
IDS = ["700-f32", "700-f64", "1300-f32", "1300-f64"]


@functools.lru_cache(maxsize=None)
def _counts(n):
    ptr, idx, val = R.fixture(M, n, SEEDS[n], np.float32)
    return ptr, idx, val, R.batch_labels(M, K, SEEDS[n] + 10), R.columns(ptr, idx, val, M, n)


@functools.lru_cache(maxsize=None)
def _v3(n, batched, reverse=False):
    ptr, idx, val, labels, _ = _counts(n)
    return R.hvg(ptr, idx, val, M, n, labels=labels if batched else None, K=K, n_top=100, span=SPAN, reverse=reverse)


@functools.lru_cache(maxsize=None)
def _logged(n, dt):
    ptr, idx, val, _, _ = _counts(n)
    return R.log1p_normalized(ptr, val.astype(dt))


@functools.lru_cache(maxsize=None)
def _seurat(n, dt, n_top, reverse=False):
    ptr, idx, _, _, _ = _counts(n)
    return R.hvg(ptr, idx, _logged(n, dt), M, n, flavor=R.SEURAT, n_top=n_top, reverse=reverse)


def _upload(n, dt, values=None, sess=None):
    ptr, idx, val, _, _ = _counts(n)
    sess = sess or ops.Session()
    v = (val if values is None else values).astype(dt)
    return sess, sess.upload(ptr, idx.astype(np.int64), v, M, n)


def _fsum_moments(cols, mask, transform, clip):
    n = len(cols)
    s, q, c = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint64)
    for j, (r, v) in enumerate(cols):
        v = v[mask[r]]
        f = R.transformed(v, transform, None if clip is None else clip[j])
        s[j], q[j] = math.fsum(f), math.fsum(f * f)
        if transform == R.CLIP:
            c[j] = int((v.astype(np.float64) > clip[j]).sum())
    return s, q, c


def _close(got, want, rel, what):
    err = np.abs(got - want)
    worst = float(np.max(err / np.where(want != 0, np.abs(want), 1.0)))
    print(f"{what}: worst relative error {worst:.3g} (allowed {rel:.3g})")
    assert (err <= rel * np.abs(want)).all(), (what, worst)


# ---- moments --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [False, True], ids=["all-rows", "one-batch"])
@pytest.mark.parametrize("n,dt", CASES, ids=IDS)
def test_clip_moments(n, dt, batched):
    ptr, idx, val, labels, cols = _counts(n)
    b = _v3(n, batched)["batches"][1 if batched else 0]
    clip = b["clip"]
    # the fixture is only accepted if it clips in at least 20 columns, leaves at least 20 alone, and excludes rows on both sides
    assert (b["n_clipped"] > 0).sum() >= 20 and (b["n_clipped"] == 0).sum() >= 20
    assert (labels == -1).any() and (labels == K).any()
    mask = R.included_rows(M, labels, 1, K) if batched else R.included_rows(M)
    s, q, c = _fsum_moments(cols, mask, R.CLIP, clip)
    sess, X = _upload(n, dt)
    got = X.hvg_moments("clip", clip=clip, batch=labels if batched else None, code=1)
    assert np.array_equal(got["n_clipped"], c) and np.array_equal(c, b["n_clipped"].astype(np.uint64))
    _close(got["sum"], s, 1e-12, "clip sum")
    _close(got["sum_squared"], q, 1e-12, "clip sum_squared")
    again = X.hvg_moments("clip", clip=clip, batch=labels if batched else None, code=1)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


@pytest.mark.parametrize("n,dt", CASES, ids=IDS)
def test_expm1_moments(n, dt):
    ptr, idx, val, labels, _ = _counts(n)
    x = _logged(n, dt)
    cols = R.columns(ptr, idx, x, M, n)
    sess, X = _upload(n, dt, x)
    for batch, code, mask in ((None, 0, R.included_rows(M)), (labels, 2, R.included_rows(M, labels, 2, K))):
        s, q, _ = _fsum_moments(cols, mask, R.EXPM1, None)
        got = X.hvg_moments("expm1", batch=batch, code=code)
        assert not got["n_clipped"].any()
        _close(got["sum"], s, 1e-12, "expm1 sum")
        _close(got["sum_squared"], q, 1e-12, "expm1 sum_squared")
        again = X.hvg_moments("expm1", batch=batch, code=code)
        assert all(got[k].tobytes() == again[k].tobytes() for k in got)


# ---- loess ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loess_ref(kind):
    x, y = R.loess_fixture(kind)
    return x, y, R.loess(x, y, SPAN), R.loess(x, y, SPAN, reverse=True)


def _loess_bound(kind):
    """1000 x the case's own reversed-order spread, the spread taken as at least one ulp of its largest |y|"""
    _, y, a, b = _loess_ref(kind)
    spread = float(np.abs(a - b).max())
    floor = float(np.finfo(np.float64).eps * np.abs(y).max())
    print(f"loess {kind}: reversed-order spread {spread:.3g}, one ulp of max |y| {floor:.3g}")
    return 1000.0 * max(spread, floor)


@pytest.mark.parametrize("kind", R.LOESS_CASES)
def test_loess_against_the_restatement(kind):
    """Measured on the CPU: spread 0 (n5), 5.3e-15 (n64), 1.2e-14 (n65), 3.2e-13 (n4000), 1.42e-12 (half_tied), 3.5e-18
    (all_equal); every case is allowed 1000 x its own, at least 1000 ulp of its largest |y| (the module's docstring)."""
    x, y, want, _ = _loess_ref(kind)
    q = R.loess_window(SPAN, x.size)
    degrees = {R.loess_degree(x, i, q) for i in range(0, x.size, max(1, x.size // 200))}
    if kind == "half_tied":
        assert degrees == {0, 1, 2}          # the h == 0 mean, the line through two abscissae, the parabola
    if kind == "all_equal":
        assert degrees == {0}
    if kind == "n5":
        assert q == 3
    bound = _loess_bound(kind)
    got = ops.Session().loess(x, y, SPAN)
    err = float(np.abs(got - want).max())
    print(f"loess {kind}: worst absolute error {err:.3g} (allowed {bound:.3g})")
    assert err <= bound
    assert got.tobytes() == ops.Session().loess(x, y, SPAN).tobytes()


# ---- the chain ------------------------------------------------------------------------------------------------------------
def _norm_var_bound(n, batched):
    a, b = _v3(n, batched), _v3(n, batched, True)
    spread = max(float(np.max(np.abs(x["norm_var"] - y["norm_var"]) / np.where(x["norm_var"] != 0, np.abs(x["norm_var"]), 1.0)))
                 for x, y in zip(a["batches"], b["batches"]))
    print(f"norm_var reversed-order spread (n = {n}, batched = {batched}): {spread:.3g}")
    return 1000.0 * spread


def _order_is_safe(cols, mask, batch, n_top, threshold):
    """(safe, the gap across the cut, the smallest neighbour gap that is not an exact tie of identical columns)"""
    nv = batch["norm_var"]
    order = np.argsort(-nv, kind="stable")[:n_top + 1]
    smallest, cut = np.inf, None
    for r in range(order.size - 1):
        a, b = order[r], order[r + 1]
        gap = float((nv[a] - nv[b]) / abs(nv[a]))
        if r == n_top - 1:
            cut = gap
        if gap == 0.0:
            (ra, va), (rb, vb) = cols[a], cols[b]
            ka, kb = mask[ra], mask[rb]
            if np.array_equal(ra[ka], rb[kb]) and np.array_equal(va[ka], vb[kb]):
                continue   # the same entries in the same rows: the same bytes on the device too, the index breaks the tie
            whole = all((v == np.rint(v)).all() and np.abs(v).max(initial=0) < 2 ** 20 for v in (va[ka], vb[kb]))
            if whole and not batch["n_clipped"][a] and not batch["n_clipped"][b] and batch["s"][a] == batch["s"][b] \
                    and batch["ss"][a] == batch["ss"][b]:
                continue   # small whole numbers, nothing clipped: both sums are exact in any order and equal, so is all that follows
        smallest = min(smallest, gap)
    return smallest >= threshold, cut, smallest


@pytest.mark.parametrize("n_top", [50, 100, 150])
@pytest.mark.parametrize("batched", [False, True], ids=["unbatched", "k3"])
@pytest.mark.parametrize("n,dt", CASES, ids=IDS)
def test_seurat_v3_against_the_restatement(n, dt, batched, n_top):
    ptr, idx, val, labels, cols = _counts(n)
    ref = _v3(n, batched)
    bound = _norm_var_bound(n, batched)
    masks = [R.included_rows(M, labels, b, K) for b in range(K)] if batched else [R.included_rows(M)]
    for b, mask in zip(ref["batches"], masks):
        safe, cut, smallest = _order_is_safe(cols, mask, b, n_top, 1000.0 * bound)
        print(f"n_top = {n_top}: gap across the cut {cut:.3g}, smallest neighbour gap {smallest:.3g}, needed {1000.0 * bound:.3g}")
        assert safe
    rank, nhv, vnorm, hv = R.combine_v3([b["norm_var"] for b in ref["batches"]], n_top)
    sess, X = _upload(n, dt)
    got = X.highly_variable(n_top, "seurat_v3", batch=labels if batched else None, n_batches=K if batched else None, span=SPAN)
    _close(got.means, ref["means"], 1e-12, "means")
    _close(got.variances, ref["variances"], 1e-12, "variances")
    _close(got.variances_norm, vnorm, bound, "variances_norm")
    assert np.array_equal(got.rank, rank, equal_nan=True)
    assert np.array_equal(got.n_batches_hv, nhv)
    assert np.array_equal(got.highly_variable, hv.astype(bool)) and got.n_selected == n_top
    assert np.isnan(got.dispersions).all() and np.isnan(got.dispersions_norm).all()
    again = X.highly_variable(n_top, "seurat_v3", batch=labels if batched else None, n_batches=K if batched else None, span=SPAN)
    assert again.variances_norm.tobytes() == got.variances_norm.tobytes()


def _disp_bound(n, dt, n_top):
    a, b = _seurat(n, dt, n_top)["dispersions_norm"], _seurat(n, dt, n_top, True)["dispersions_norm"]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    spread = float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(a))))
    print(f"dispersions_norm reversed-order spread (n = {n}): {spread:.3g}")
    return 1000.0 * spread


def _norm_close(got, want, bound):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    print(f"dispersions_norm: worst error {float(err.max()):.3g} (allowed {bound:.3g})")
    assert (err <= bound).all()


@pytest.mark.parametrize("n_top", [50, 100, 150])
@pytest.mark.parametrize("n,dt", CASES, ids=IDS)
def test_seurat_with_n_top(n, dt, n_top):
    ref = _seurat(n, dt, n_top)
    b = ref["batches"][0]
    # a one-gene bin, an empty bin and a bin whose std is 0 (the two identical columns)
    assert (b["bin_count"] == 1).any() and (b["bin_count"] == 0).any() and ((b["bin_count"] >= 2) & (b["bin_std"] == 0)).any()
    bound = _disp_bound(n, dt, n_top)
    gap = R.cut_gap(ref["dispersions_norm"], n_top)
    print(f"n_top = {n_top}: gap across the cut {gap:.3g}, needed {1000.0 * bound:.3g}")
    assert gap >= 1000.0 * bound
    sess, X = _upload(n, dt, _logged(n, dt))
    got = X.highly_variable(n_top, "seurat")
    _close(got.means, ref["means"], 1e-12, "means")
    _close(got.variances, ref["variances"], 1e-12, "variances")
    _norm_close(got.dispersions_norm, ref["dispersions_norm"], bound)
    assert np.array_equal(got.highly_variable, ref["highly_variable"].astype(bool))
    assert np.array_equal(got.n_batches_hv, ref["highly_variable"].astype(np.uint32))
    assert np.isnan(got.rank).all() and np.isnan(got.variances_norm).all()


@pytest.mark.parametrize("n,dt", CASES, ids=IDS)
def test_seurat_with_cutoffs(n, dt):
    ref = _seurat(n, dt, 0)
    bound = _disp_bound(n, dt, 0)
    mn, mx, dmin, _ = R.DEFAULT_CUTOFFS
    norm = np.where(np.isnan(ref["dispersions_norm"]), 0.0, ref["dispersions_norm"])
    margin = min(float(np.min(np.abs(ref["means"] - mn) / mn)), float(np.min(np.abs(ref["means"] - mx) / mx)),
                 float(np.min(np.abs(norm - dmin))))
    print(f"cutoffs: smallest margin {margin:.3g}, needed {1000.0 * bound:.3g}")
    assert margin >= 1000.0 * bound
    sess, X = _upload(n, dt, _logged(n, dt))
    got = X.highly_variable(None, "seurat")
    _norm_close(got.dispersions_norm, ref["dispersions_norm"], bound)
    ok = ~np.isnan(ref["dispersions"])
    assert np.array_equal(np.isnan(got.dispersions), ~ok) and np.abs(got.dispersions[ok] - ref["dispersions"][ok]).max() <= 1e-11
    assert np.array_equal(got.highly_variable, ref["highly_variable"].astype(bool)) and 0 < got.n_selected < n


def test_seurat_with_batches_runs_and_counts():
    """the batched combination of the seurat flavour against the restatement (means 1e-12, the counts and the selection equal
    where the cut is safe: asserted)"""
    n, dt, n_top = 700, np.float32, 100
    ptr, idx, _, labels, _ = _counts(n)
    x = _logged(n, dt)
    ref = R.hvg(ptr, idx, x, M, n, labels=labels, K=K, flavor=R.SEURAT, n_top=n_top)
    rev = R.hvg(ptr, idx, x, M, n, labels=labels, K=K, flavor=R.SEURAT, n_top=n_top, reverse=True)
    spread = max(float(np.nanmax(np.abs(a["norm"] - b["norm"]) / np.maximum(1.0, np.abs(a["norm"]))))
                 for a, b in zip(ref["batches"], rev["batches"]))
    bound = 1000.0 * spread
    gaps = [R.cut_gap(b["norm"], n_top) for b in ref["batches"]]
    print(f"seurat k3: spread {spread:.3g}, gaps across the batch cuts {gaps}")
    assert min(gaps) >= 1000.0 * bound
    sess, X = _upload(n, dt, x)
    got = X.highly_variable(n_top, "seurat", batch=labels, n_batches=K)
    _close(got.means, ref["means"], 1e-12, "means")
    assert np.array_equal(got.n_batches_hv, ref["n_batches_hv"])
    _norm_close(got.dispersions_norm, ref["dispersions_norm"], bound)
    order = np.lexsort((np.arange(n), np.where(np.isnan(ref["dispersions_norm"]), np.inf, -ref["dispersions_norm"]),
                        -ref["n_batches_hv"].astype(np.int64)))
    a, b = order[n_top - 1], order[n_top]
    if ref["n_batches_hv"][a] == ref["n_batches_hv"][b]:   # the final cut falls inside a class of equal counts: its gap decides
        g = abs(ref["dispersions_norm"][a] - ref["dispersions_norm"][b]) / max(1.0, abs(ref["dispersions_norm"][a]))
        assert g >= 1000.0 * bound
    assert np.array_equal(got.highly_variable, ref["highly_variable"].astype(bool)) and got.n_selected == n_top


# ---- consumers and handle state ----------------------------------------------------------------------------------------------
def test_the_selection_feeds_a_masked_fit_and_a_column_selection():
    n, n_top = 700, 100
    sess, X = _upload(n, np.float32)
    hv = X.highly_variable(n_top).highly_variable
    assert hv.dtype == np.bool_ and hv.sum() == n_top
    S = X.select(cols=hv)
    assert S.shape == (M, n_top)
    mask8 = hv.view(np.uint8)
    est = (sapca.MaskedSparsePCABuilder.new().n_components(4).mask(hv).svd_method(SVDMethod.Random(4, 1, PIN.QR)).build())
    L.check(est._h, L.load().sapca_set_mask(est._h, ops._p(mask8, C.c_uint8), C.c_size_t(mask8.size)))   # the library's bytes, as they are
    est.fit(X.as_device_csr())
    assert est._dims()[1] == n_top


def test_a_fitted_estimator_is_untouched():
    n, k = 700, 5
    ptr, idx, val, labels, _ = _counts(n)
    dev = (torch.as_tensor(ptr, device="cuda"), torch.as_tensor(idx, device="cuda"), torch.as_tensor(val, device="cuda"))
    est = sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Random(4, 2, PIN.QR)).build()
    csr = sapca.DeviceCsr(*dev, (M, n))
    est.fit_transform(csr)
    before = est.transform(csr).cpu().numpy()
    comps = est.components_(np.float64).copy()
    sess = ops.Session.borrow(est._h)
    X = ops.ResidentCsr(sess, (M, n), dev[2].numel(), np.float32, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr())
    got = X.highly_variable(100, batch=labels, n_batches=K)
    assert got.n_selected == 100
    sess.loess(np.arange(50.0), np.arange(50.0) ** 2, 0.5)
    assert est.transform(csr).cpu().numpy().tobytes() == before.tobytes()
    np.testing.assert_array_equal(est.components_(np.float64), comps)


def test_refusals_name_the_number_and_leave_the_handle_usable():
    n = 700
    ptr, idx, val, labels, _ = _counts(n)
    sess, X = _upload(n, np.float64)
    want = X.highly_variable(50).highly_variable
    lib = L.load()
    h, m, n_, nnz, p, i, v = X._args()
    d = torch.as_tensor(labels, device="cuda")
    lone = labels.copy()
    lone[lone == 2] = 0
    lone[5] = 2                                     # batch 2 holds one row
    d_lone = torch.as_tensor(lone, device="cuda")
    hv = np.zeros(n, dtype=np.uint8)
    s = np.zeros(n)

    def run(m_=m, p_=p, batch=None, nb=1, **kw):
        o = L.default_hvg_options()
        o.n_top = 50
        for key, value in kw.items():
            setattr(o, key, value)
        return lib.sapca_hvg_csr_device_f64(h, m_, n_, nnz, p_, i, v, batch, C.c_uint32(nb), C.byref(o), None, None, None, None, None,
                                            None, None, ops._p(hv, C.c_uint8))

    def moments(transform, clip, batch=None, code=0):
        return lib.sapca_hvg_moments_csr_device_f64(h, m, n_, nnz, p, i, v, batch, C.c_int32(code), C.c_int32(transform), clip,
                                                    ops._p(s, C.c_double), None, None)

    def last():
        return lib.sapca_last_error(h).decode()

    dp, dl = C.c_void_p(d.data_ptr()), C.c_void_p(d_lone.data_ptr())
    for call, words in ((lambda: run(flavor=7), ("flavor = 7",)),
                        (lambda: run(n_top=0), ("n_top = 0", "SEURAT_V3")),
                        (lambda: run(n_top=n + 1), (f"n_top = {n + 1}", f"n = {n}")),
                        (lambda: run(span=0.0), ("span = 0",)),
                        (lambda: run(span=1.5), ("span = 1.5",)),
                        (lambda: run(flavor=L.HVG_SEURAT, n_bins=0), ("n_bins = 0",)),
                        (lambda: run(nb=0), ("n_batches = 0",)),
                        (lambda: run(batch=dp, nb=1025), ("n_batches = 1025", "SAPCA_HVG_MAX_BATCHES = 1024")),
                        (lambda: run(batch=dl, nb=3), ("batch 2 has 1 rows",)),
                        (lambda: run(m_=C.c_uint64(2 ** 31)), (str(2 ** 31), "rows")),
                        (lambda: run(p_=None), ("null CSR array",)),
                        (lambda: run(struct_size=8), ("struct_size is 8",)),
                        (lambda: moments(5, None), ("transform = 5",)),
                        (lambda: moments(L.HVG_CLIP, None), ("clip is NULL", f"n = {n}")),
                        (lambda: moments(L.HVG_EXPM1, None, dp, -3), ("batch = -3",)),
                        (lambda: lib.sapca_loess_f64(h, C.c_uint64(4), ops._p(s, C.c_double), ops._p(s, C.c_double), C.c_double(2.0),
                                                     ops._p(s, C.c_double)), ("span = 2",)),
                        (lambda: lib.sapca_loess_f64(h, C.c_uint64(2 ** 31), ops._p(s, C.c_double), ops._p(s, C.c_double),
                                                     C.c_double(0.3), ops._p(s, C.c_double)), (str(2 ** 31), "points"))):
        assert call() == L.ERR_ARG
        assert all(w in last() for w in words), last()
        assert np.array_equal(X.highly_variable(50).highly_variable, want)   # a checked call on the same handle
    # empty shapes are valid
    zeros = torch.zeros(8, dtype=torch.int64, device="cuda")
    E = ops.ResidentCsr(sess, (0, 4), 0, np.float64, zeros.data_ptr(), 0, 0)
    e = E.highly_variable(2)
    assert not e.highly_variable.any() and np.isnan(e.rank).all() and not e.means.any()
    E2 = ops.ResidentCsr(sess, (5, 0), 0, np.float64, zeros.data_ptr(), 0, 0)
    assert E2.highly_variable(1).highly_variable.size == 0 and E2.hvg_moments("expm1")["sum"].size == 0
    assert sess.loess(np.zeros(0), np.zeros(0)).size == 0
    assert np.array_equal(X.highly_variable(50).highly_variable, want)

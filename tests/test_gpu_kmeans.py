"""K-means of device-resident rows (-m gpu): sapca_kmeans_* through Session.kmeans_seed / kmeans_assign / kmeans_update / kmeans
and sapca.KMeans.  The reference is tests/kmeans_ref.py (numpy, f64; held to scikit-learn by tests/test_kmeans_cpu.py).

Every comparison that a rounding could turn is guarded on the reference first, before the GPU result is looked at: labels are
compared where the reference's relative margin exceeds the header's 64 d eps_f64 (and the test shows that to be every row of
its fixture), seeding where u_t S lies more than 1e-9 S from every prefix boundary, whole runs where the smallest margin
along the reference's run exceeds 8 eps_T (a one-ulp difference in a stored centroid, propagated to a distance).

Centroids are held element by element to 2 ulp_T of the reference's value plus the one thing no order of summation can avoid:
a mean of n_c rows is an f64 sum of n_c terms, and any order of adding them is within n_c eps_f64 / 2 sum |x| of the exact
sum, so the mean is within n_c eps_f64 mean_i |x_it| of the exact mean of cluster c's column t (_centroid_tolerance).  The
term is in eps_f64 whatever T is: for f32 it is seven orders below an ulp.  The reference sums in extended precision, so its
own error is far below either term.

The issue lists "the returned centroids are the update of the returned labels" without a condition.  It holds where a run ends
on the strict test; a run that ends on tol or max_iter returns, by the loop the issue states, the update of the labels BEFORE
its closing assignment, so there the check is made against those labels (the reference reports them as update_labels)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kmeans_ref as KR
import sapca
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
IDS = dict(ids=["f32", "f64"])
DTYPES = [np.float32, np.float64]
EPS64 = np.finfo(np.float64).eps


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def sess():
    return ops.Session()


# ------------------------------------------------------------------ 1. the exact grid: assign and update on integers
# a design over m, d and k (not their product): every listed value of each occurs, k <= m
GRID = [(1, 1, 1), (15, 3, 2), (16, 4, 15), (17, 5, 16), (63, 50, 17), (64, 64, 64), (65, 127, 65), (129, 128, 2), (1000, 50, 256),
        (2049, 5, 65), (2049, 64, 17), (1000, 127, 1), (129, 1, 64), (1500, 8, 1024)]


@functools.lru_cache(maxsize=None)
def _integer_reference(m, d, k):
    X, Cn = KR.integer_case(m, d, k, 1000 * m + 10 * d + k)
    labels, d2, margin = KR.assign(X, Cn)
    return X, Cn, labels, d2, margin


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("m,d,k", GRID, ids=[f"m{m}-d{d}-k{k}" for m, d, k in GRID])
def test_assign_and_update_are_exact_on_integers(sess, m, d, k, dt):
    """coordinates in [-3, 3], d <= 128: every score, distance and sum is an integer below 2^24, so nothing rounds in either
    precision and labels (ties to the lower index included), distances, counts and means must be the reference's bit for bit"""
    X, Cn, labels, d2, margin = _integer_reference(m, d, k)
    if k >= 4 and m >= 15:
        assert (margin == 0).any()                                   # exact ties occur: duplicated centroids are in play
    x, cen = _dev(X.astype(dt)), _dev(Cn.astype(dt))
    got_l, got_d, inertia, n_amb = sess.kmeans_assign(x, cen)
    np.testing.assert_array_equal(_host(got_l), labels)
    np.testing.assert_array_equal(_host(got_d), d2.astype(dt))
    assert inertia == d2.sum()
    assert n_amb >= (margin == 0).sum()                              # a tie is always left to the f64 pass
    want_c, want_n = KR.update(X, labels, Cn, dt)
    got_c, got_n = sess.kmeans_update(x, got_l, cen)
    np.testing.assert_array_equal(_host(got_n), want_n)
    assert _host(got_c).tobytes() == want_c.tobytes()


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_a_row_stride_beyond_d_is_not_read(sess, dt):
    m, d, k = 129, 50, 17
    X, Cn, labels, d2, _ = _integer_reference(m, d, k)
    wide = np.full((m, d + 7), np.nan, dtype=dt)
    wide[:, :d] = X
    x = _dev(wide)[:, :d]
    assert x.stride(0) == d + 7
    cen = _dev(Cn.astype(dt))
    got_l, got_d, inertia, _ = sess.kmeans_assign(x, cen)
    np.testing.assert_array_equal(_host(got_l), labels)
    np.testing.assert_array_equal(_host(got_d), d2.astype(dt))
    assert inertia == d2.sum()
    got_c, got_n = sess.kmeans_update(x, got_l, cen)
    want_c, want_n = KR.update(X, labels, Cn, dt)
    assert _host(got_c).tobytes() == want_c.tobytes() and (_host(got_n) == want_n).all()
    cs, rows = sess.kmeans_seed(x, 5, seed=3)
    assert np.isfinite(_host(cs)).all() and (_host(cs) == X[_host(rows)].astype(dt)).all()


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_update_keeps_an_empty_cluster_and_skips_labels_outside_the_range(sess, dt):
    m, d, k = 1000, 50, 17
    X, Cn, labels, _, _ = _integer_reference(m, d, k)
    lab = labels.copy()
    victim = int(np.bincount(labels, minlength=k).argmax())
    out = np.flatnonzero(lab == victim)
    lab[out] = np.resize(np.array([-1, k, k + 5, 2 ** 31 - 1, -2 ** 31], dtype=np.int64), out.size).astype(np.int32)
    got_c, got_n = sess.kmeans_update(_dev(X.astype(dt)), _dev(lab), _dev(Cn.astype(dt)))
    want_c, want_n = KR.update(X, lab, Cn, dt)
    assert want_n[victim] == 0 and want_n.sum() == m - out.size
    np.testing.assert_array_equal(_host(got_n), want_n)
    assert _host(got_c).tobytes() == want_c.tobytes()
    assert (_host(got_c)[victim] == Cn[victim].astype(dt)).all()     # kept


# ------------------------------------------------------------------ 2. real-valued assignment
BLOBS = {8: (2.0, 1), 17: (4.0, 1)}      # k: (spread, seed) of the 2000 x 50 blobs, chosen on the CPU (see the test's guards)


@functools.lru_cache(maxsize=None)
def _blob_reference(k, dt):
    spread, seed = BLOBS[k]
    X = KR.blobs(2000, 50, k, spread, seed)[0].astype(dt)
    Cn = X[:k].copy()
    return (X, Cn) + KR.assign(X, Cn)


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("k", sorted(BLOBS))
def test_assign_on_gaussian_blobs(sess, k, dt):
    X, Cn, labels, d2, margin = _blob_reference(k, dt)
    m, d = X.shape
    assert (margin > 64 * d * EPS64).all()                            # every row's label is pinned by the contract
    eps = float(np.finfo(dt).eps)
    bound = 4 * d * eps
    if dt == np.float32:
        # a score is an FMA chain of length d (d eps / 2 |x| |c|, doubled) plus the bias: two of them differ from the exact
        # difference by about a quarter of the bound, so a margin under half the bound is always flagged, one over twice never
        assert (margin < bound / 2).sum() >= 1 and (margin < 2 * bound).mean() < 0.05
    got_l, got_d, inertia, n_amb = sess.kmeans_assign(_dev(X), _dev(Cn))
    np.testing.assert_array_equal(_host(got_l), labels)
    want_d = d2.astype(dt)
    assert (np.abs(_host(got_d).astype(np.float64) - want_d) <= 2 * np.spacing(want_d).astype(np.float64)).all()
    assert abs(inertia - d2.sum()) <= m * EPS64 * d2.sum()
    print(f"k = {k} {np.dtype(dt).name}: n_ambiguous {n_amb} of {m}, reference rows under the bound {(margin < bound).sum()}")
    if dt == np.float32:
        assert 0 < n_amb < 0.05 * m
    assert n_amb <= (margin < 2 * bound).sum()


# ------------------------------------------------------------------ 3. seeding
SEEDINGS = [(2000, 50, 8, 1), (1500, 8, 64, 2), (3000, 50, 17, 3)]


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("m,d,k,seed", SEEDINGS, ids=[f"m{m}-k{k}" for m, d, k, s in SEEDINGS])
def test_seeding_picks_the_reference_rows(sess, m, d, k, seed, dt):
    X = KR.blobs(m, d, min(k, 8), 0.5, seed)[0].astype(dt)
    rows, boundary = KR.seed(X, k, seed)
    assert boundary.min() > 1e-9
    cen, got = sess.kmeans_seed(_dev(X), k, seed=seed)
    np.testing.assert_array_equal(_host(got), rows)
    assert _host(cen).tobytes() == X[rows].tobytes()
    cen2, got2 = ops.Session(seed=seed).kmeans_seed(_dev(X), k)       # the Session's seed is the default
    assert _host(got2).tobytes() == _host(got).tobytes() and _host(cen2).tobytes() == _host(cen).tobytes()


def test_seeding_over_more_than_1024_blocks(sess):
    """1.1 million rows: the block sums themselves take two chunks of 1024"""
    m, k, seed = 1_100_000, 3, 4
    X = np.random.default_rng(seed).normal(size=(m, 1)).astype(np.float32)
    rows, boundary = KR.seed(X, k, seed)
    assert boundary.min() > 1e-9 and m * EPS64 < 1e-9
    cen, got = sess.kmeans_seed(_dev(X), k, seed=seed)
    np.testing.assert_array_equal(_host(got), rows)
    assert _host(cen).tobytes() == X[rows].tobytes()


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_seeding_falls_back_when_every_row_is_a_centre(sess, dt):
    X = np.tile(np.arange(1, 7, dtype=dt), (1500, 1))
    rows, _ = KR.seed(X, 5, 9)
    np.testing.assert_array_equal(rows, np.floor(KR.uniforms(9, 5) * 1500).astype(np.int64))
    cen, got = sess.kmeans_seed(_dev(X), 5, seed=9)
    np.testing.assert_array_equal(_host(got), rows)
    assert (_host(cen) == X[:5]).all()


# ------------------------------------------------------------------ 4. whole runs
RUNS = {8: (2000, 1), 17: (3000, 1)}      # k: (m, seed) of the m x 50 blobs of spread 0.5, seeds chosen on the CPU


@functools.lru_cache(maxsize=None)
def _run_reference(k, dt, tol=0.0, max_iter=300):
    m, seed = RUNS[k]
    X = KR.blobs(m, 50, k, 0.5, seed)[0].astype(dt)
    return X, KR.lloyd(X, X[:k], max_iter, tol, dt)


def _centroid_tolerance(X, labels, want, dt):
    """k x d: 2 ulp_T of the reference's centroid, plus n_c eps_f64 mean |x| over the cluster's rows, column by column"""
    X64 = np.abs(np.asarray(X, dtype=np.float64))
    tol = 2 * np.spacing(np.abs(want).astype(dt)).astype(np.float64)
    for c in range(want.shape[0]):
        rows = X64[labels == c]
        if len(rows):
            tol[c] += len(rows) * EPS64 * rows.mean(axis=0)
    return tol


def _assert_centroids(X, update_labels, got, want, dt):
    """got against the reference's centroids `want`, which are the update of update_labels (None: no update ran, the given
    centroids come back bit for bit)"""
    if update_labels is None:
        assert got.tobytes() == np.ascontiguousarray(want).tobytes()
        return
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (diff <= _centroid_tolerance(X, update_labels, want, dt)).all(), f"largest excess {(diff - _centroid_tolerance(X, update_labels, want, dt)).max():.3e}"


def _check_fixed_point(X, labels, cen, n_iter, max_iter, dt, update_labels):
    """whatever the margins: the labels are the assignment to the returned centroids (on the rows the contract pins), the
    centroids are the update of update_labels -- the returned labels themselves where the run ended on the strict test -- and
    the loop stayed inside max_iter"""
    want_l, _, margin = KR.assign(X, cen)
    pinned = margin > 64 * X.shape[1] * EPS64
    np.testing.assert_array_equal(labels[pinned], want_l[pinned])
    if update_labels is not None:
        want_c, _ = KR.update(X, update_labels, cen, dt)
        _assert_centroids(X, update_labels, cen, want_c, dt)
    assert n_iter <= max_iter


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("k", sorted(RUNS))
def test_whole_runs_equal_the_reference(sess, k, dt):
    X, ref = _run_reference(k, dt)
    assert ref["min_margin"] > 8 * float(np.finfo(np.float32).eps) and ref["strict"] and 9 <= ref["n_iter"] <= 28
    labels, cen, inertia, n_iter = sess.kmeans(_dev(X), n_clusters=k, init=_dev(X[:k]), max_iter=300, tol=0.0)
    labels, cen = _host(labels), _host(cen)
    print(f"k = {k} {np.dtype(dt).name}: n_iter {n_iter} (reference {ref['n_iter']}), inertia {inertia!r} (reference {ref['inertia']!r}), "
          f"largest centroid difference {np.abs(cen.astype(np.float64) - ref['centroids']).max():.3e}")
    _check_fixed_point(X, labels, cen, n_iter, 300, dt, labels)
    assert n_iter == ref["n_iter"]
    np.testing.assert_array_equal(labels, ref["labels"])
    _assert_centroids(X, ref["update_labels"], cen, ref["centroids"], dt)
    assert abs(inertia - ref["inertia"]) <= (1e-6 if dt == np.float32 else 1e-12) * ref["inertia"]


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("tol", [1e-4, 1e-2])
def test_runs_under_a_tolerance(sess, tol, dt):
    """tol = 1e-4: the strict test still ends this run; tol = 1e-2: the shift does, three iterations earlier"""
    X, ref = _run_reference(8, dt, tol)
    assert ref["tol_gap"] > 1e-6 and ref["min_margin"] > 8 * float(np.finfo(np.float32).eps)
    assert ref["strict"] == (tol == 1e-4)
    labels, cen, inertia, n_iter = sess.kmeans(_dev(X), n_clusters=8, init=_dev(X[:8]), max_iter=300, tol=tol)
    labels, cen = _host(labels), _host(cen)
    _check_fixed_point(X, labels, cen, n_iter, 300, dt, labels if ref["strict"] else ref["update_labels"])
    assert n_iter == ref["n_iter"]
    np.testing.assert_array_equal(labels, ref["labels"])
    _assert_centroids(X, ref["update_labels"], cen, ref["centroids"], dt)
    assert abs(inertia - ref["inertia"]) <= (1e-6 if dt == np.float32 else 1e-12) * ref["inertia"]


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("max_iter", [0, 1, 9])
def test_runs_cut_short_by_max_iter(sess, max_iter, dt):
    """9: the host looks at the convergence flag after 8 iterations and finds it clear"""
    X, ref = _run_reference(8, dt, 0.0, max_iter)
    assert ref["n_iter"] == max_iter and not ref["strict"] and ref["min_margin"] > 8 * float(np.finfo(np.float32).eps)
    labels, cen, inertia, n_iter = sess.kmeans(_dev(X), n_clusters=8, init=_dev(X[:8]), max_iter=max_iter, tol=0.0)
    labels, cen = _host(labels), _host(cen)
    _check_fixed_point(X, labels, cen, n_iter, max_iter, dt, ref["update_labels"])
    assert n_iter == max_iter
    if max_iter == 0:
        assert cen.tobytes() == X[:8].tobytes()
    np.testing.assert_array_equal(labels, ref["labels"])
    _assert_centroids(X, ref["update_labels"], cen, ref["centroids"], dt)
    assert abs(inertia - ref["inertia"]) <= (1e-6 if dt == np.float32 else 1e-12) * ref["inertia"]


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_one_cluster_and_as_many_clusters_as_rows(sess, dt):
    X = KR.blobs(2000, 50, 8, 0.5, 1)[0].astype(dt)
    for rows, k in ((X[:300], 1), (X[:40], 40)):
        ref = KR.lloyd(rows, rows[:k], 300, 0.0, dt)
        labels, cen, inertia, n_iter = sess.kmeans(_dev(rows), n_clusters=k, init=_dev(rows[:k]), max_iter=300, tol=0.0)
        labels, cen = _host(labels), _host(cen)
        assert n_iter == ref["n_iter"] == (2 if k == 1 else 1) and ref["strict"] == (k == 1)
        _check_fixed_point(rows, labels, cen, n_iter, 300, dt, labels if ref["strict"] else ref["update_labels"])
        np.testing.assert_array_equal(labels, ref["labels"])
        _assert_centroids(rows, ref["update_labels"], cen, ref["centroids"], dt)
        assert abs(inertia - ref["inertia"]) <= (1e-6 if dt == np.float32 else 1e-12) * ref["inertia"]
    assert inertia == 0.0                                             # k = m: every row is its own centroid


# ------------------------------------------------------------------ 5. contract
@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_two_calls_return_the_same_bytes_and_the_host_route_equals_the_device_route(sess, dt):
    X = KR.blobs(3000, 50, 17, 0.5, 2)[0].astype(dt)
    a = sess.kmeans(_dev(X), n_clusters=17, seed=5)
    b = sess.kmeans(_dev(X), n_clusters=17, seed=5)
    c = ops.Session().kmeans(X, n_clusters=17, seed=5)                # numpy in, numpy out: sapca_kmeans_*
    rows, boundary = KR.seed(X, 17, 5)
    assert boundary.min() > 1e-9
    d = sess.kmeans(_dev(X), n_clusters=17, init=_dev(X[rows]))       # the run started from the seeding's centres
    for other in (b, d):
        assert _host(a[0]).tobytes() == _host(other[0]).tobytes() and _host(a[1]).tobytes() == _host(other[1]).tobytes()
        assert a[2:] == other[2:]
    assert _host(a[0]).tobytes() == c[0].tobytes() and _host(a[1]).tobytes() == c[1].tobytes() and a[2:] == c[2:]
    _check_fixed_point(X, _host(a[0]), _host(a[1]), a[3], 300, dt, None)        # (how the run ended is not known here: labels only)
    assert a[3] >= 2


def test_the_estimator(sess):
    X = KR.blobs(2000, 50, 8, 0.5, 1)[0].astype(np.float32)
    km = sapca.KMeans(n_clusters=8, seed=11).fit(_dev(X))
    want = sess.kmeans(_dev(X), n_clusters=8, seed=11)
    assert _host(km.labels_).tobytes() == _host(want[0]).tobytes() and km.inertia_ == want[2] and km.n_iter_ == want[3]
    assert _host(km.cluster_centers_).tobytes() == _host(want[1]).tobytes()
    assert _host(km.predict(_dev(X))).tobytes() == _host(km.labels_).tobytes()      # a converged run: predict is the last assignment
    assert (km.predict(X[:100]) == _host(km.labels_)[:100]).all()                   # numpy rows in, numpy labels out
    assert (_host(sapca.KMeans(n_clusters=8, seed=11).fit_predict(_dev(X))) == _host(km.labels_)).all()
    mixed = sapca.KMeans(n_clusters=8, init=X[:8], max_iter=3, tol=0.0).fit(_dev(X))  # device rows, a host array of centres
    given = sapca.KMeans(n_clusters=8, init=X[:8], max_iter=3, tol=0.0).fit(X)        # the host route with given centres
    assert _host(mixed.labels_).tobytes() == given.labels_.tobytes() and _host(mixed.cluster_centers_).tobytes() == given.cluster_centers_.tobytes()
    ref = KR.lloyd(X, X[:8], 3, 0.0, np.float32)
    assert given.n_iter_ == 3 and (given.labels_ == ref["labels"]).all()


def _estimator(k, omega):
    return (sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Random(4, 2, PIN.QR))
            .transform_semantics(L.TRANSFORM_CENTERED).build().set_omega(omega))


def test_a_fitted_estimator_is_untouched_by_a_clustering_of_its_scores(sess):
    m, n, k = 1200, 300, 8
    ptr, idx, val = (x.cpu().numpy() for x in synth.gapped_csr(m, n, 0.08, k, seed=5, dtype=torch.float32))
    est = _estimator(k, synth.gaussian_panel(n, k + 4, 3).numpy())
    dev = sapca.DeviceCsr(_dev(ptr.astype(np.int64)), _dev(idx.astype(np.int32)), _dev(val), (m, n))
    scores = est.fit_transform(dev)
    before = _host(est.transform(dev))
    getters = [est.components_(np.float64).copy(), est.explained_variance_ratio(np.float64).copy(), est.mean_(np.float64).copy(),
               est.singular_values_(np.float64).copy()]
    got = est.session().kmeans(scores, n_clusters=6, seed=42)
    want = sess.kmeans(scores.clone(), n_clusters=6, seed=42)        # the same rows on a bare handle
    assert _host(got[0]).tobytes() == _host(want[0]).tobytes() and got[2:] == want[2:]
    sliced = est.session().kmeans(scores[:, :4], n_clusters=3)         # a column slice, clustered in place
    assert sliced[3] >= 1 and np.isfinite(sliced[2])
    assert _host(est.transform(dev)).tobytes() == before.tobytes()
    after = [est.components_(np.float64), est.explained_variance_ratio(np.float64), est.mean_(np.float64), est.singular_values_(np.float64)]
    for a, b in zip(getters, after):
        assert a.tobytes() == b.tobytes()


def test_a_handle_in_a_communicator_clusters_locally(sess):
    calls = []

    def allreduce(sendbuf, recvbuf, count, dtype, user):
        calls.append(count)
        return 0

    est = _estimator(4, synth.gaussian_panel(50, 8, 1).numpy())
    est.comm_set_callback(2, 0, allreduce)                       # rank 0 of 2: the handle belongs to a communicator
    X = _dev(KR.blobs(500, 7, 4, 0.5, 9)[0].astype(np.float32))
    got = est.session().kmeans(X, n_clusters=4, seed=42)
    want = sess.kmeans(X, n_clusters=4, seed=42)
    assert _host(got[0]).tobytes() == _host(want[0]).tobytes() and got[2:] == want[2:]
    assert calls == []


def _options(**changes):
    o = L.default_kmeans_options()
    o.n_clusters, o.init, o.max_iter = 4, L.KMEANS_GIVEN, 20
    for name, value in changes.items():
        setattr(o, name, value)
    return o


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _raw_kmeans(sess, dt, o, m, x, ldx, d, cen, labels):
    fn = getattr(L.load(), f"sapca_kmeans_device_{'f32' if dt == np.float32 else 'f64'}")
    inertia, n_iter = C.c_double(-1.0), C.c_uint64(77)
    torch.cuda.synchronize()      # (what torch queued for the arrays is complete before the handle's stream touches them)
    st = fn(sess._h, C.c_uint64(m), _ptr(x), C.c_uint64(ldx), C.c_uint64(d), C.byref(o), _ptr(cen), _ptr(labels), C.byref(inertia),
            C.byref(n_iter))
    return st, (L.load().sapca_last_error(sess._h) or b"").decode(), inertia.value, n_iter.value


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_refusals_leave_the_handle_usable(dt):
    sess = ops.Session()
    X = KR.blobs(40, 6, 4, 0.5, 2)[0].astype(dt)
    x, start = _dev(X), _dev(X[:4])
    cen = start.clone()
    labels = torch.full((40,), -7, dtype=torch.int32, device="cuda")
    ok = dict(m=40, x=x, ldx=6, d=6, cen=cen, labels=labels)
    st, msg, inertia_ok, n_iter_ok = _raw_kmeans(sess, dt, o=_options(), **ok)
    assert st == L.OK, msg
    good = _host(labels).tobytes() + _host(cen).tobytes()
    cases = [
        (dict(), dict(struct_size=24), "options->struct_size is 24"),
        (dict(), dict(n_clusters=0), "n_clusters is 0"),
        (dict(), dict(n_clusters=1025), "n_clusters = 1025 exceeds SAPCA_KMEANS_MAX_CLUSTERS = 1024"),
        (dict(), dict(n_clusters=41), "n_clusters = 41 exceeds the m = 40 rows"),
        (dict(), dict(init=2), "unknown init 2"),
        (dict(), dict(tol=-1.0), "tol = -1 must be finite and not negative"),
        (dict(), dict(tol=float("nan")), "tol = nan must be finite and not negative"),
        (dict(), dict(tol=float("inf")), "tol = inf must be finite and not negative"),
        (dict(d=0), dict(), "d is 0"),
        (dict(d=1025, ldx=2000), dict(), "d = 1025 exceeds 1024"),
        (dict(ldx=5), dict(), "ldx = 5 is less than d = 6"),
        (dict(ldx=2 ** 28), dict(), f"a row stride of {2 ** 28} elements; 2^28 or more are not supported"),
        (dict(m=2 ** 31), dict(), f"m = {2 ** 31} rows"),
        (dict(x=None), dict(), "a NULL array with m = 40"),
        (dict(cen=None), dict(), "a NULL array with m = 40"),
        (dict(labels=None), dict(), "a NULL array with m = 40"),
    ]
    for change, opt, message in cases:
        cen.copy_(start)
        labels.fill_(-7)
        st, msg, inertia, n_iter = _raw_kmeans(sess, dt, o=_options(**opt), **{**ok, **change})
        assert st == L.ERR_ARG and message in msg, f"{change} {opt}: status {st}, message {msg!r}"
        assert (labels == -7).all() and (cen == start).all() and inertia == -1.0 and n_iter == 77, f"{change} {opt}: an output was written"
        st, msg, inertia, n_iter = _raw_kmeans(sess, dt, o=_options(), **ok)       # the same handle, straight after
        assert st == L.OK, msg
        assert _host(labels).tobytes() + _host(cen).tobytes() == good and inertia == inertia_ok and n_iter == n_iter_ok
    # the stage calls refuse the same way
    lib, suf = L.load(), "f32" if dt == np.float32 else "f64"
    panel = [sess._h, C.c_uint64(40), _ptr(x), C.c_uint64(6), C.c_uint64(6)]
    stage = [
        (getattr(lib, f"sapca_kmeans_seed_device_{suf}"), [C.c_uint32(41), C.c_uint32(1), _ptr(cen), None], "n_clusters = 41 exceeds the m = 40 rows"),
        (getattr(lib, f"sapca_kmeans_assign_device_{suf}"), [C.c_uint32(0), _ptr(cen), _ptr(labels), None, None, None], "n_clusters is 0"),
        (getattr(lib, f"sapca_kmeans_assign_device_{suf}"), [C.c_uint32(4), _ptr(cen), None, None, None, None], "a NULL array with m = 40"),
        (getattr(lib, f"sapca_kmeans_update_device_{suf}"), [C.c_uint32(1025), _ptr(labels), _ptr(cen), None], "n_clusters = 1025 exceeds"),
        (getattr(lib, f"sapca_kmeans_update_device_{suf}"), [C.c_uint32(4), None, _ptr(cen), None], "a NULL array with m = 40"),
    ]
    cen.copy_(start)
    labels.fill_(-7)
    for fn, rest, message in stage:
        st = fn(*panel, *rest)
        msg = (lib.sapca_last_error(sess._h) or b"").decode()
        assert st == L.ERR_ARG and message in msg, msg
        assert (labels == -7).all() and (cen == start).all()
    st, msg, inertia, n_iter = _raw_kmeans(sess, dt, o=_options(), **ok)
    assert st == L.OK and _host(labels).tobytes() + _host(cen).tobytes() == good


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_no_rows_is_valid_and_writes_nothing(sess, dt):
    empty = torch.zeros((0, 5), dtype=DT[np.dtype(dt)], device="cuda")
    cen = torch.full((3, 5), 2.5, dtype=DT[np.dtype(dt)], device="cuda")
    labels, out, inertia, n_iter = sess.kmeans(empty, n_clusters=3, init=cen)
    assert labels.numel() == 0 and (out == 2.5).all() and inertia == 0.0 and n_iter == 0
    labels, dist2, inertia, n_amb = sess.kmeans_assign(empty, cen)
    assert labels.numel() == 0 and dist2.numel() == 0 and inertia == 0.0 and n_amb == 0
    out, counts = sess.kmeans_update(empty, labels, cen)
    assert (out == 2.5).all() and (counts == 0).all()
    seeded = torch.full((3, 5), -1.0, dtype=DT[np.dtype(dt)], device="cuda")
    fn = getattr(L.load(), f"sapca_kmeans_seed_device_{'f32' if dt == np.float32 else 'f64'}")
    assert fn(sess._h, C.c_uint64(0), None, C.c_uint64(5), C.c_uint64(5), C.c_uint32(3), C.c_uint32(1), _ptr(seeded), None) == L.OK
    assert (seeded == -1.0).all()
    labels, out, inertia, n_iter = ops.Session().kmeans(np.zeros((0, 5), dtype=dt), n_clusters=3)     # the host route
    assert labels.size == 0 and inertia == 0.0 and n_iter == 0

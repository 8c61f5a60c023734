"""Exact k-nearest neighbours of device-resident rows (-m gpu): sapca_knn_device_* through Session.knn.

The reference is tests/knn_ref.py (numpy brute force in f64; held to cKDTree, scikit-learn and the reference's own loops by
tests/test_knn_cpu.py).

Exact cases: coordinates are integers in [-3, 3] and d <= 128, so every inner product, norm and squared distance is an
integer below 2^24, exact in f32 whatever the summation order: the selection cannot round, ties are everywhere, and the
indices must equal the reference's exactly, the Euclidean values sqrt(exact integer) rounded once to T.  The grid is
covered by a design, not a product: every size pair below meets two widths, and with each every admissible list length,
with and without EXCLUDE_SELF, in both dtypes.  (The similarity metrics scale rows to unit norm, which is not exact on
integers; they run on the same integer data under the bars of the real-valued cases.)

Real-valued cases (Gaussian clusters with offsets, 1500 x 3000, d = 50): returned values within 2 ulp of T of the direct
formula in extended precision at the returned indices; lists sorted by (value, index); the j-th returned squared distance
(1 - similarity on unit rows) exceeds the reference's j-th by at most 4 d eps_T (|a| + max |b|)^2 -- the rounding of an FMA
chain of length d on both sides of a swap, derived, not tuned; in f64 the indices equal the reference's wherever the
reference's gaps exceed that bound, which the test first shows to be at least 99 % of the lists.
Largest excess seen on an MI355X, as a fraction of the bound: see DESIGN.md, "Neighbour search"."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import knn_ref as KR
import sapca
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
SIZES = [1, 15, 16, 17, 63, 64, 65, 129, 1000]
WIDTHS = [1, 3, 4, 5, 50, 64, 127, 128]
LENGTHS = [1, 2, 15, 16, 17, 64, 128]          # and mc - 1, mc
# every size as mq and as mc, equal and unequal, small against large both ways
PAIRS = [(s, s) for s in SIZES] + [(1, 1000), (1000, 1), (17, 129), (129, 17), (65, 1000), (1000, 65), (15, 64), (63, 16),
                                   (16, 63), (64, 15), (129, 1000), (1000, 129)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(sess, Q, Cm, k, metric, exclude_self, dt):
    """(indices, values) on the host; Cm None: self-search on one tensor"""
    q = _dev(Q.astype(dt))
    c = None if Cm is None else _dev(Cm.astype(dt))
    idx, val = sess.knn(q, c, k, metric=metric, exclude_self=exclude_self)
    assert idx.dtype == torch.int32 and val.dtype == DT[np.dtype(dt)] and tuple(idx.shape) == tuple(val.shape) == (Q.shape[0], k)
    return idx.cpu().numpy(), val.cpu().numpy()


def _integers(rows, d, seed, dup_of=None):
    """integer coordinates in [-3, 3]; a fifth of the rows are exact copies of other rows (of `dup_of`, if given)"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, (rows, d)).astype(np.float64)
    src = X if dup_of is None else dup_of
    for r in rng.choice(rows, rows // 5, replace=False):
        X[r] = src[rng.integers(0, src.shape[0])]
    return X


@pytest.fixture(scope="module")
def sess():
    return ops.Session()


# ------------------------------------------------------------------ 1. exact cases
_EXACT = {}


def _exact_case(case, d):
    """(Q, corpus, squared distances as exact integers, {exclude_self: full order}) of one grid point, computed once and shared
    by the two dtypes"""
    if (case, d) not in _EXACT:
        mq, mc = PAIRS[case]
        Cm = _integers(mc, d, 100 + case)
        Q = Cm if mq == mc else _integers(mq, d, 200 + case, dup_of=Cm)
        sq = np.rint(KR.pairwise(Q, Cm, "euclidean") ** 2)                     # the exact integers
        assert sq.max() < 2 ** 24
        _EXACT[(case, d)] = (Q, Cm, sq, {e: KR.full_order(np.sqrt(sq), "euclidean", e)[0] for e in (False, True)})
    return _EXACT[(case, d)]


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(PAIRS)), ids=[f"{a}x{b}" for a, b in PAIRS])
def test_exact_integer_grid(sess, case, dt):
    mq, mc = PAIRS[case]
    for d in (WIDTHS[case % 8], WIDTHS[(case + 3) % 8]):
        Q, Cm, sq, orders = _exact_case(case, d)
        for excl in (False, True):
            order = orders[excl]
            for k in sorted({k for k in LENGTHS + [mc - 1, mc] if 1 <= k <= min(128, mc - int(excl))}):
                gi, gv = _run(sess, Q, None if mq == mc else Cm, k, "euclidean", excl, dt)
                what = f"mq {mq} mc {mc} d {d} k {k} exclude_self {excl} {np.dtype(dt).name}"
                np.testing.assert_array_equal(gi, order[:, :k], err_msg=f"{what}: indices")
                want = np.sqrt(np.take_along_axis(sq, order[:, :k], axis=1)).astype(dt)
                np.testing.assert_array_equal(gv, want, err_msg=f"{what}: values")


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("metric", KR.METRICS)
def test_strided_panels_with_nan_in_the_padding(sess, metric, dt):
    """ldq, ldc > d: slices of wider buffers whose other columns hold NaN give the bytes of the contiguous call"""
    tdt = DT[np.dtype(dt)]
    for (mq, mc, d, k, excl) in [(65, 129, 5, 17, False), (129, 129, 50, 16, True), (17, 1000, 127, 64, False), (64, 65, 3, 2, False)]:
        Cm = _integers(mc, d, 300 + d)
        Q = Cm if mq == mc else _integers(mq, d, 400 + d, dup_of=Cm)
        wide_c = torch.full((mc, d + 7), float("nan"), dtype=tdt, device="cuda")
        wide_c[:, 3:3 + d] = _dev(Cm.astype(dt))
        if mq == mc:
            wide_q, qv = wide_c, wide_c[:, 3:3 + d]
        else:
            wide_q = torch.full((mq, d + 1), float("nan"), dtype=tdt, device="cuda")
            wide_q[:, :d] = _dev(Q.astype(dt))
            qv = wide_q[:, :d]
        gi, gv = sess.knn(qv, None if mq == mc else wide_c[:, 3:3 + d], k, metric=metric, exclude_self=excl)
        wi, wv = _run(sess, Q, None if mq == mc else Cm, k, metric, excl, dt)
        what = f"{metric} mq {mq} mc {mc} d {d}"
        np.testing.assert_array_equal(gi.cpu().numpy(), wi, err_msg=what)
        assert gv.cpu().numpy().tobytes() == wv.tobytes(), what
        assert not np.isnan(wv).any() and wi.min() >= 0
        assert torch.isnan(wide_c[:, :3]).all() and torch.isnan(wide_c[:, 3 + d:]).all()      # the padding is untouched


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_corpus_split_over_workgroups_gives_the_same_bytes(sess, dt):
    """mq = 3 against mc = 20 000 runs with the corpus dealt to many workgroups per query block and a merge; the same rows
    inside a run of 2 000 queries are split differently, inside a run of 40 000 not at all: same bytes"""
    mc, d, k = 20_000, 5, 17
    Cm = _integers(mc, d, 7)
    Q = _integers(40_000, d, 8, dup_of=Cm)
    c = _dev(Cm.astype(dt))
    q = _dev(Q.astype(dt))
    for metric in ("euclidean", "pearson"):
        small = [t.cpu().numpy() for t in sess.knn(q[:3], c, k, metric=metric)]
        for rows in (2_000, 40_000):
            big = [t[:3].cpu().numpy() for t in sess.knn(q[:rows], c, k, metric=metric)]
            assert small[0].tobytes() == big[0].tobytes() and small[1].tobytes() == big[1].tobytes(), f"{metric}, {rows} queries"
        if metric == "euclidean":
            wi, wv = KR.knn(Q[:3], Cm, k, metric)
            np.testing.assert_array_equal(small[0], wi)
            np.testing.assert_array_equal(small[1], wv.astype(dt))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_many_queries_take_the_128_row_workgroups(sess, dt):
    """70 000 queries are enough workgroups of 128 rows to fill an MI355X twice over, so the selection runs two 16-row blocks
    per wave (the geometry of the C2 score shape); against a small corpus that is cheap.  Exact integers: the whole result
    equals the reference, and slices run as small calls (64-row workgroups) give the same bytes"""
    mq, mc, d, k = 70_000, 129, 5, 15
    Cm = _integers(mc, d, 61)
    Q = _integers(mq, d, 62, dup_of=Cm)
    sq = np.rint(KR.pairwise(Q, Cm, "euclidean", chunk=4096) ** 2)
    c, q = _dev(Cm.astype(dt)), _dev(Q.astype(dt))
    for excl in (False, True):
        order = KR.full_order(np.sqrt(sq), "euclidean", excl)[0][:, :k]
        gi, gv = sess.knn(q, c, k, exclude_self=excl)
        gi, gv = gi.cpu().numpy(), gv.cpu().numpy()
        np.testing.assert_array_equal(gi, order, err_msg=f"exclude_self {excl}: indices")
        np.testing.assert_array_equal(gv, np.sqrt(np.take_along_axis(sq, order, axis=1)).astype(dt), err_msg=f"exclude_self {excl}: values")
    for metric in KR.METRICS:
        bi, bv = (t.cpu().numpy() for t in sess.knn(q, c, k, metric=metric))
        assert KR.is_sorted(bi, bv, metric) and bi.min() >= 0 and bi.max() < mc
        for lo in (0, 100, 33_333, mq - 300):                     # a slice starts its own numbering of blocks and waves
            si, sv = (t.cpu().numpy() for t in sess.knn(q[lo:lo + 300], c, k, metric=metric))
            assert si.tobytes() == bi[lo:lo + 300].tobytes() and sv.tobytes() == bv[lo:lo + 300].tobytes(), f"{metric}, rows from {lo}"


# ------------------------------------------------------------------ 2. real-valued cases
def _clusters(rows, d, seed, centres):
    rng = np.random.default_rng(seed)
    X = centres[rng.integers(0, centres.shape[0], rows)] + rng.normal(0.0, 1.0, (rows, d))
    return X.astype(np.float32).astype(np.float64)            # representable in both dtypes: one reference serves both


@pytest.fixture(scope="module")
def real():
    d, k = 50, 30
    centres = np.random.default_rng(11).normal(0.0, 3.0, (12, d)) + 2.0       # clusters, and an offset from the origin
    Q, Cm = _clusters(1500, d, 12, centres), _clusters(3000, d, 13, centres)
    out = {"Q": Q, "C": Cm, "k": k}
    for metric in KR.METRICS:
        vals = KR.pairwise(Q, Cm, metric)
        order, sv = KR.full_order(vals, metric)
        out[metric] = (order[:, :k + 1], sv[:, :k + 1])                       # one more: the gap behind the list
    return out


def _loss(Q, Cm, idx, metric):
    """what the ranking minimises, f64 from the returned indices: squared distance, or 1 - similarity"""
    v = np.asarray(KR.values_at(Q, Cm, idx, metric), dtype=np.float64)
    return v * v if metric == "euclidean" else 1.0 - v


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("metric", KR.METRICS)
def test_real_valued_clusters(sess, real, metric, dt):
    Q, Cm, k = real["Q"], real["C"], real["k"]
    order, sv = real[metric]
    gi, gv = _run(sess, Q, Cm, k, metric, False, dt)
    assert gi.min() >= 0 and gi.max() < Cm.shape[0]
    assert all(np.unique(r).size == k for r in gi), "a corpus row twice in one list"
    # values: the direct formula at the returned indices, to 2 ulp of T
    want = KR.values_at(Q, Cm, gi, metric, dt)
    ulp = np.spacing(np.abs(np.asarray(want, dtype=np.float64)).astype(dt)).astype(np.longdouble)
    err = np.abs(gv.astype(np.longdouble) - want) / ulp
    print(f"\n{metric} {np.dtype(dt).name}: values off by at most {float(err.max()):.3f} ulp")
    assert err.max() <= 2.0
    assert KR.is_sorted(gi, gv, metric), "a list is not sorted by (value, index)"
    # the j-th returned against the reference's j-th
    bound = KR.swap_bound(Q, Cm, dt) if metric == "euclidean" else np.full(Q.shape[0], 4.0 * Q.shape[1] * np.finfo(dt).eps * 4.0)
    ref_loss = sv[:, :k] ** 2 if metric == "euclidean" else 1.0 - sv[:, :k]
    excess = (_loss(Q, Cm, gi, metric) - ref_loss) / bound[:, None]
    print(f"{metric} {np.dtype(dt).name}: largest excess over the reference's j-th value: {float(excess.max()):.3e} of the bound")
    assert excess.max() <= 1.0
    if dt == np.float64:
        full_loss = sv ** 2 if metric == "euclidean" else 1.0 - sv
        clear = (np.diff(full_loss, axis=1) > bound[:, None]).all(axis=1)     # every gap, the one behind the list included
        assert clear.mean() >= 0.99, f"only {clear.mean():.3f} of the reference's lists have clear gaps"
        np.testing.assert_array_equal(gi[clear], order[clear, :k])


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("metric", ["cosine", "pearson"])
def test_similarities_on_integer_data_with_ties(sess, metric, dt):
    """the similarity metrics on the tie-ridden integer data, self-search: values, order and the bound as above"""
    X = _integers(1000, 5, 21)
    k = 64
    gi, gv = _run(sess, X, None, k, metric, True, dt)
    assert (gi != np.arange(1000)[:, None]).all() and gi.min() >= 0
    want = KR.values_at(X, X, gi, metric, dt)
    ulp = np.spacing(np.maximum(np.abs(np.asarray(want, dtype=np.float64)), np.finfo(dt).tiny).astype(dt)).astype(np.longdouble)
    assert (np.abs(gv.astype(np.longdouble) - want) <= 2.0 * ulp).all()
    assert KR.is_sorted(gi, gv, metric)
    _, sv = KR.knn(X, X, k, metric, exclude_self=True, T=dt)
    excess = (1.0 - np.asarray(want, dtype=np.float64)) - (1.0 - sv)
    assert excess.max() <= 4.0 * 5 * np.finfo(dt).eps * 4.0


# ------------------------------------------------------------------ 3. edges and lifecycle
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_zero_and_constant_rows(sess, dt):
    rng = np.random.default_rng(31)
    X = rng.normal(1.0, 2.0, (200, 6)).astype(np.float32).astype(np.float64)
    X[[0, 17, 64, 199]] = 0.0                                   # zero rows
    X[[5, 130]] = 2.5                                           # constant rows: zero once centred
    X[77] = 0.0
    X[77, 2] = 1e-5                                             # below sqrt(eps_f32), above sqrt(eps_f64)
    for metric in ("cosine", "pearson"):
        gi, gv = _run(sess, X, None, 20, metric, True, dt)
        wi, wv = KR.knn(X, X, 20, metric, exclude_self=True, T=dt)
        zero = [0, 17, 64, 199] + ([5, 130] if metric == "pearson" else []) + ([77] if dt == np.float32 and metric == "cosine" else [])
        for r in zero:                                          # similarity 0 to everything: index order
            assert gi[r].tolist() == [j for j in range(21) if j != r][:20], f"{metric} row {r}"
            assert (gv[r] == 0).all()
        assert KR.is_sorted(gi, gv, metric)
        bound = 4.0 * 6 * np.finfo(dt).eps * 4.0                 # the selection's rounding on unit rows, as above
        np.testing.assert_allclose(gv, wv, rtol=0, atol=bound + 2 * np.finfo(dt).eps)
        clear = (np.abs(np.diff(wv, axis=1)) > 2 * bound).all(axis=1)                      # lists without near-ties
        np.testing.assert_array_equal(gi[clear], wi[clear])
    gi, gv = _run(sess, X, None, 5, "euclidean", True, dt)      # a duplicate of a point is a neighbour at distance 0
    assert gi[0].tolist()[:3] == [17, 64, 199] and (gv[0][:3] == 0).all()


def test_call_to_call_byte_identity(sess, real):
    Q, Cm = _dev(real["Q"].astype(np.float32)), _dev(real["C"].astype(np.float32))
    for metric in KR.METRICS:
        a = [t.cpu().numpy().tobytes() for t in sess.knn(Q, Cm, 30, metric=metric)]
        b = [t.cpu().numpy().tobytes() for t in sess.knn(Q, Cm, 30, metric=metric)]
        fresh = [t.cpu().numpy().tobytes() for t in ops.Session().knn(Q, Cm, 30, metric=metric)]
        assert a == b == fresh, metric


def _raw(sess, dt, mq, q, ldq, mc, c, ldc, d, metric, k, flags, idx, val):
    import ctypes as C
    fn = getattr(L.load(), f"sapca_knn_device_{'f32' if dt == np.float32 else 'f64'}")
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)   # noqa: E731
    torch.cuda.synchronize()
    st = fn(sess._h, C.c_uint64(mq), p(q), C.c_uint64(ldq), C.c_uint64(mc), p(c), C.c_uint64(ldc), C.c_uint64(d), C.c_int32(metric),
            C.c_uint32(k), C.c_uint32(flags), p(idx), p(val))
    return st, (L.load().sapca_last_error(sess._h) or b"").decode()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_refusals_leave_the_handle_usable(dt):
    sess = ops.Session()
    X = _integers(40, 6, 41)
    x = _dev(X.astype(dt))
    idx = torch.full((40, 8), -7, dtype=torch.int32, device="cuda")
    val = torch.full((40, 8), -7.0, dtype=DT[np.dtype(dt)], device="cuda")
    ok = dict(mq=40, q=x, ldq=6, mc=40, c=x, ldc=6, d=6, metric=0, k=8, flags=1, idx=idx, val=val)
    cases = [
        (dict(k=0), "n_neighbors is 0"),
        (dict(k=129), "n_neighbors = 129 exceeds SAPCA_KNN_MAX_NEIGHBORS = 128"),
        (dict(k=40), "n_neighbors = 40 exceeds the 39 corpus rows"),
        (dict(k=41, flags=0), "n_neighbors = 41 exceeds the 40 corpus rows"),
        (dict(d=0), "d is 0"),
        (dict(d=1025, ldq=2000, ldc=2000), "d = 1025 exceeds 1024"),
        (dict(ldq=5), "ldq = 5 is less than d = 6"),
        (dict(ldc=3), "ldc = 3 is less than d = 6"),
        (dict(mc=2 ** 31), f"mc = {2 ** 31} corpus rows"),
        (dict(metric=3), "unknown metric 3"),
        (dict(metric=-1), "unknown metric -1"),
        (dict(flags=6), "unknown flag bits 6"),
        (dict(q=None), "d_queries is NULL with mq = 40"),
        (dict(c=None), "d_corpus is NULL with mc = 40"),
        (dict(idx=None), "a NULL output with mq = 40"),
        (dict(val=None), "a NULL output with mq = 40"),
    ]
    for change, message in cases:
        st, msg = _raw(sess, dt, **{**ok, **change})
        assert st == L.ERR_ARG and message in msg, f"{change}: status {st}, message {msg!r}"
        assert (idx == -7).all() and (val == -7).all(), f"{change}: an output was written"
        st, msg = _raw(sess, dt, **ok)                                          # the same handle, straight after
        assert st == L.OK, msg
        wi, wv = KR.knn(X, X, 8, "euclidean", exclude_self=True)
        np.testing.assert_array_equal(idx.cpu().numpy(), wi)
        np.testing.assert_array_equal(val.cpu().numpy(), wv.astype(dt))
        idx.fill_(-7)
        val.fill_(-7.0)
    st, msg = _raw(sess, dt, **{**ok, "mq": 0, "q": None, "idx": None, "val": None})   # no queries: valid, writes nothing
    assert st == L.OK, msg
    gi, gv = sess.knn(x[:0], x, 8)
    assert tuple(gi.shape) == (0, 8) and tuple(gv.shape) == (0, 8)
    with pytest.raises(ValueError, match="n_neighbors = 40 exceeds the 39"):
        sess.knn(x, None, 40)


def _estimator(k, omega, centred=True):
    b = sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Random(4, 2, PIN.QR))
    if centred:
        b = b.transform_semantics(L.TRANSFORM_CENTERED)
    return b.build().set_omega(omega)


class _InHandleOf:
    """a Session-shaped view of an estimator's handle (not owned)"""

    def __init__(self, est):
        self._est, self._h = est, est._h

    knn = ops.Session.knn


def _gapped(m, n, k, seed):
    ptr, idx, val = (x.cpu().numpy() for x in synth.gapped_csr(m, n, 0.08, k, seed=seed, dtype=torch.float32))
    return sp.csr_matrix((val, idx.astype(np.int64), ptr.astype(np.int64)), shape=(m, n))


def test_a_fitted_estimator_is_untouched_and_its_scores_are_searched_in_place():
    m, n, k = 3000, 400, 8
    A = _gapped(m, n, k, 5)
    est = _estimator(k, synth.gaussian_panel(n, k + 4, 3).numpy())
    dev = sapca.DeviceCsr(_dev(A.indptr.astype(np.int64)), _dev(A.indices.astype(np.int32)), _dev(A.data), (m, n))
    scores = est.fit_transform(dev)                              # m x k on the device
    before = est.transform(dev).cpu().numpy()
    comps = est.components_(np.float64).copy()
    # end to end: neighbours of the score rows, in place (ld = n_components), against the reference on their host copy
    gi, gv = _InHandleOf(est).knn(scores, None, 15)
    S = scores.cpu().numpy().astype(np.float64)
    wi, wv = KR.knn(S, S, 16, "euclidean", exclude_self=True)
    want = KR.values_at(S, S, gi.cpu().numpy(), "euclidean")
    got = gv.cpu().numpy()
    assert (np.abs(got.astype(np.longdouble) - want) <= 2 * np.spacing(np.asarray(want, dtype=np.float64).astype(np.float32))).all()
    assert KR.is_sorted(gi.cpu().numpy(), got, "euclidean")
    bound = KR.swap_bound(S, S, np.float32)
    assert ((np.asarray(want, dtype=np.float64) ** 2 - wv[:, :15] ** 2) <= bound[:, None]).all()
    clear = (np.diff(wv ** 2, axis=1) > bound[:, None]).all(axis=1)         # lists the selection's rounding cannot reorder
    np.testing.assert_array_equal(gi.cpu().numpy()[clear], wi[clear, :15])
    # a column slice of the same buffer, cosine: the first four components only
    ci, cv = _InHandleOf(est).knn(scores[:, :4], None, 10, metric="cosine")
    w4 = KR.values_at(S[:, :4], S[:, :4], ci.cpu().numpy(), "cosine", np.float32)
    assert (np.abs(cv.cpu().numpy().astype(np.longdouble) - w4) <= 2 * np.finfo(np.float32).eps).all()
    # the model is what it was: the same projection, bit for bit
    assert est.transform(dev).cpu().numpy().tobytes() == before.tobytes()
    np.testing.assert_array_equal(est.components_(np.float64), comps)


def test_a_handle_in_a_communicator_searches_locally():
    calls = []

    def allreduce(sendbuf, recvbuf, count, dtype, user):
        calls.append(count)
        return 0

    est = _estimator(4, synth.gaussian_panel(50, 8, 1).numpy())
    est.comm_set_callback(2, 0, allreduce)                       # rank 0 of 2: the handle belongs to a communicator
    X = _integers(300, 7, 51)
    gi, gv = _InHandleOf(est).knn(_dev(X.astype(np.float32)), None, 9)
    wi, wv = KR.knn(X, X, 9, "euclidean", exclude_self=True)
    np.testing.assert_array_equal(gi.cpu().numpy(), wi)
    np.testing.assert_array_equal(gv.cpu().numpy(), wv.astype(np.float32))
    assert not calls

"""Marker columns of a labelled resident CSR on the GPU (-m gpu): sapca_rank_sums_csr_device_* and
sapca_rank_groups_csr_device_* against the host restatement tests/rank_groups_ref.py.

Bars.  rank_sum2, nonzero, group_rows and tie_sum are EQUAL (integers; tie_sum is an exact integer at these sizes).  z is
within 16 eps relative of the header's formula evaluated on the library's own rank_sum2, group_rows and tie_sum; t likewise
where the rest is one group (K = 2), so that its mean and variance are returned ingredients too.  mean is within
c eps sum|x| / n_g and var within 16 (c + K) eps sum x^2 / (n_g - 1) of exactly summed references (c: the column's stored
entries; the sums over the column).  z_pvalue is compared with math.erfc at the library's own z: 4 x the worst relative
discrepancy between math.erfc and scipy.special.erfc over the test's z values, at least 8 eps -- measured on the CPU over the
restatement's z of these fixtures: 1.15e-15 at six groups and 1.76e-15 (7.9 eps) at 1,024, so 4.6e-15 and 7.0e-15 are allowed.
t against scipy.stats.ttest_ind on the well-conditioned fixture of test_t_against_scipy: 100 x the restatement's own worst
deviation from scipy there, measured on the CPU: 6.5e-15 relative, so 6.5e-13.  Both figures are measured again where the
test runs, from the same references, and printed.

K = 1024 is SAPCA_RANK_MAX_GROUPS and also what one launch of the labelled statistics holds, so inside this operator the
code-slice loop makes one turn; its second turn is test_gpu_batch_stats.py's at 1,100 codes, through the same loop."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.special
import scipy.stats
import torch

import rank_groups_ref as R
import sapca
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

EPS = R.EPS
M = 6000
W, LM = R.WAVE_MAX, R.LDS_MAX
LENS = [0, 1, 2, 63, 64, 65, W - 1, W, W + 1, 300, 1000, LM - 1, LM, LM + 1, 5000, M]   # both class limits, every class


def _values(rng, L_, kind, dt):
    if kind == "counts":
        v = rng.integers(1, 5, L_).astype(dt)
    else:
        v = rng.normal(0.3, 2.0, L_).astype(dt)
    zero = rng.random(L_) < 0.03                       # stored zeros, half of them -0.0
    v[zero] = np.where(rng.random(int(zero.sum())) < 0.5, 0.0, -0.0).astype(dt)
    return v


def _special(rng, L_, dt):
    """a subnormal on each side of 0, stored +0.0 and -0.0, two values one ulp apart, both infinities, each twice"""
    tiny = np.nextafter(dt(0), dt(1))
    head = np.array([tiny, -tiny, 0.0, -0.0, 1.0, np.nextafter(dt(1), dt(2)), np.inf, -np.inf] * 2, dtype=dt)
    assert tiny > 0 and tiny < np.finfo(dt).tiny and head[5] != head[4]
    v = _values(rng, L_, "real", dt)
    v[:head.size] = head
    return rng.permutation(v)


def _straddling(L_, dt):
    """distinct values but for tie runs of 70 every 97 sorted positions: some run crosses every kind of chunk edge"""
    v = np.arange(1, L_ + 1, dtype=np.float64)
    for s in range(200, L_ - 70, 97):
        v[s:s + 70] = s + 0.5
    return v.astype(dt)


def _matrix(m, columns, dt):
    """CSR of `columns`: [(rows, values)]; stored zeros stay stored"""
    r = np.concatenate([c[0] for c in columns] + [np.zeros(0, dtype=np.int64)])
    j = np.concatenate([np.full(len(c[0]), k, dtype=np.int64) for k, c in enumerate(columns)] + [np.zeros(0, dtype=np.int64)])
    v = np.concatenate([c[1] for c in columns] + [np.zeros(0, dtype=dt)]).astype(dt)
    A = sp.csr_matrix((v, (r, j)), shape=(m, len(columns)))
    A.sort_indices()
    assert A.nnz == v.size
    return A


def _case(kind, dt, seed=5, m=M, lens=LENS):
    rng = np.random.default_rng(seed)
    cols = [(np.sort(rng.choice(m, L_, replace=False)), _values(rng, L_, kind, dt)) for L_ in lens]
    for L_ in (40, 600, 4500):                         # the special values in every class
        if L_ <= m:
            cols.append((np.sort(rng.choice(m, L_, replace=False)), _special(rng, L_, dt)))
    if m >= 4500:
        cols.append((rng.permutation(m)[:4500], _straddling(4500, dt)))
    return _matrix(m, cols, dt)


def _labels(m, K, seed, single=None, empty=None):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, K, m).astype(np.int32)
    for g in (single, empty):
        if g is not None:
            lab[lab == g] = (g + 1) % K
    if single is not None:
        lab[min(17, m - 1)] = single
    out = rng.random(m) < 0.05                          # -1 and >= K scattered through the rows
    lab[out] = np.where(rng.random(int(out.sum())) < 0.5, -1, K + rng.integers(0, 3, int(out.sum())))
    if single is not None:
        lab[min(17, m - 1)] = single
    return lab


def _resident(A, sess=None):
    sess = sess or ops.Session()
    return sess, sess.upload(A.indptr, A.indices, A.data, A.shape[0], A.shape[1])


def _arrays(A):
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data


def _exact_moments(A, labels, K):
    """(s, q, abs, sq): K x n exactly summed group sums and sums of squares, and per column sum|x| and sum x^2 (included rows)"""
    Ac = A.tocsc()
    n = A.shape[1]
    s, q = np.zeros((K, n)), np.zeros((K, n))
    ab, sq = np.zeros(n), np.zeros(n)
    inc = (labels >= 0) & (labels < K)
    for j in range(n):
        r = Ac.indices[Ac.indptr[j]:Ac.indptr[j + 1]]
        v = Ac.data[Ac.indptr[j]:Ac.indptr[j + 1]].astype(np.float64)
        keep = inc[r] & np.isfinite(v)
        ab[j], sq[j] = math.fsum(np.abs(v[keep])), math.fsum(v[keep] ** 2)
        for g in np.unique(labels[r[inc[r]]]):
            x = v[labels[r] == g]
            s[g, j], q[g, j] = (math.fsum(x), math.fsum(x * x)) if np.isfinite(x).all() else (x.sum(), (x * x).sum())
    return s, q, ab, sq


def _erfc_bound(z):
    """4 x the worst relative discrepancy of math.erfc against scipy.special.erfc over |z| / sqrt 2, at least 8 eps"""
    x = np.abs(np.asarray(z, dtype=np.float64).ravel()) / math.sqrt(2.0)
    a = np.array([math.erfc(t) for t in x])
    b = scipy.special.erfc(x)
    ok = b > np.finfo(np.float64).tiny
    worst = float(np.max(np.abs(a[ok] - b[ok]) / b[ok])) if ok.any() else 0.0
    print(f"math.erfc against scipy.special.erfc over {x.size} z values: worst relative discrepancy {worst:.3e}")
    return max(4.0 * worst, 8.0 * EPS)


def _check_scores(A, labels, K, got, sums, tie_correct):
    """the library's scores against its own ingredients and against exactly summed moments"""
    n = A.shape[1]
    z, _ = R.wilcoxon(sums["rank_sum2"], sums["group_rows"], sums["tie_sum"], tie_correct)
    dz = np.abs(got["z"] - z)
    print(f"z: worst relative deviation from the formula on the library's ingredients {float(np.max(dz / np.maximum(np.abs(z), 1e-300))):.3e}")
    assert (dz <= 16 * EPS * np.abs(z)).all()
    bound = _erfc_bound(got["z"])
    want_p = np.array([math.erfc(abs(t) / math.sqrt(2.0)) for t in got["z"].ravel()]).reshape(got["z"].shape)
    assert (np.abs(got["pz"] - want_p) <= bound * want_p + 4 * 2.0 ** -1074).all()
    s, q, ab, sq = _exact_moments(A, labels, K)
    cols = np.flatnonzero(np.isfinite(np.asarray(A.multiply(A).sum(axis=0)).ravel()))   # (a column with an infinity: ranks only)
    c = np.diff(A.tocsc().indptr).astype(np.float64)
    group = sums["group_rows"].astype(np.float64)
    for g in range(K):
        ng = group[g]
        if ng == 0:
            assert not got["mean"][g].any() and not got["var"][g].any() and not got["t"][g].any() and not got["df"][g].any()
            continue
        dm = np.abs(got["mean"][g] - s[g] / ng)[cols]
        assert (dm <= (c * EPS * ab / ng)[cols]).all(), (g, float(dm.max()))
        if ng < 2:
            assert not got["var"][g].any() and not got["df"][g].any()
            continue
        want_v = np.maximum(0.0, (q[g] - s[g] * s[g] / ng) / (ng - 1))
        dv = np.abs(got["var"][g] - want_v)[cols]
        assert (dv <= (16 * (c + K) * EPS * sq / (ng - 1))[cols]).all(), (g, float(dv.max()))


def _raw_groups(Rm, labels, K, tie_correct, want):
    """the C call itself: the outputs named in `want`, the others NULL"""
    m, n = Rm.shape
    suf = "f32" if Rm.dtype == np.float32 else "f64"
    d = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.int32), device="cuda") if isinstance(labels, np.ndarray) else labels
    out = {k: np.zeros((K, n), dtype=np.uint64 if k == "nz" else np.float64) for k in want if k != "rows"}
    if "rows" in want:
        out["rows"] = np.zeros(K, dtype=np.uint64)
    p = lambda k: ops._p(out[k], C.c_uint64 if k in ("nz", "rows") else C.c_double) if k in out else None   # noqa: E731
    torch.cuda.synchronize()
    L.check(Rm._s._h, getattr(L.load(), f"sapca_rank_groups_csr_device_{suf}")(
        *Rm._args(), C.c_void_p(d.data_ptr() if m else None), C.c_uint32(K), C.c_int32(tie_correct), p("rows"), p("mean"), p("var"),
        p("nz"), p("t"), p("df"), p("z"), p("pz")))
    return out


ALL = ("rows", "mean", "var", "nz", "t", "df", "z", "pz")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["counts", "real"])
def test_every_class_against_the_restatement(dt, kind):
    K = 6
    A = _case(kind, dt)
    labels = _labels(M, K, 3, single=4, empty=5)
    ptr, idx, val = _arrays(A)
    want = R.rank_sums(ptr, idx, val, M, A.shape[1], labels, K)
    assert want["group_rows"][4] == 1 and want["group_rows"][5] == 0
    # the straddling column: a tie run of the kept entries crosses a step of the long class's walk
    col = A.tocsc()
    r = col.indices[col.indptr[-2]:col.indptr[-1]]
    kept = np.sort(col.data[col.indptr[-2]:col.indptr[-1]][(labels[r] >= 0) & (labels[r] < K)])
    edges = np.arange(R.WALK_CHUNK, kept.size, R.WALK_CHUNK)
    assert kept.size > LM and (kept[edges - 1] == kept[edges]).any()
    sess, Rm = _resident(A)
    got = Rm.rank_sums(labels, K)
    for k in ("group_rows", "rank_sum2", "nonzero", "tie_sum"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert (got["rank_sum2"].sum(axis=0) == int(want["group_rows"].sum()) * (int(want["group_rows"].sum()) + 1)).all()
    for tc in (0, 1):
        g = _raw_groups(Rm, labels, K, tc, ALL)
        np.testing.assert_array_equal(g["rows"], want["group_rows"])
        np.testing.assert_array_equal(g["nz"], want["nonzero"])
        _check_scores(A, labels, K, g, got, bool(tc))
    # the same bytes on a second call and on a second handle
    again = _raw_groups(Rm, labels, K, 1, ALL)
    _, R2 = _resident(A)
    other = _raw_groups(R2, labels, K, 1, ALL)
    for k in ALL:
        assert g[k].tobytes() == again[k].tobytes() == other[k].tobytes(), k
    sums2 = R2.rank_sums(labels, K)
    assert all(got[k].tobytes() == sums2[k].tobytes() for k in got)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_only_what_is_asked_for_is_computed_and_agrees(dt):
    K = 6
    A = _case("counts", dt, seed=9, m=3000, lens=[0, 1, 70, 300, 2000, 3000])
    labels = _labels(3000, K, 4, empty=2)
    sess, Rm = _resident(A)
    full = _raw_groups(Rm, labels, K, 0, ALL)
    want = R.rank_sums(*_arrays(A), 3000, A.shape[1], labels, K)
    for subset in (("nz",), ("rows",), ("z",), ("pz", "nz"), ("t", "df"), ("mean",), ("var", "nz"), ("nz", "t")):
        part = _raw_groups(Rm, labels, K, 0, subset)    # (nz without a rank pass: the counting kernel)
        for k in subset:
            assert part[k].tobytes() == full[k].tobytes(), (subset, k)
    np.testing.assert_array_equal(full["nz"], want["nonzero"])
    r = Rm.rank_groups(labels, K, method="t-test", n_top=3)
    assert r.scores.tobytes() == full["t"].tobytes() and r.names.shape == (K, 3)
    np.testing.assert_array_equal(r.names, R.names(full["t"], 3))
    ok = np.isfinite(r.scores)                          # (a column with an infinity has no t)
    assert r.pvals is not None and ((r.pvals[ok] >= 0) & (r.pvals[ok] <= 1)).all()
    w = Rm.rank_groups(labels, K)                       # n_groups given, the default method
    assert w.scores.tobytes() == full["z"].tobytes() and w.pvals.tobytes() == full["pz"].tobytes()
    assert Rm.rank_groups(labels).group_rows.size == int(labels.max()) + 1     # n_groups from the labels


def test_t_where_the_rest_is_one_group():
    """K = 2: the rest of each group is the other, whose mean and variance the call returns: t and df from those ingredients"""
    m, n = 4000, 60
    A = sp.random(m, n, density=0.1, format="csr", random_state=3, data_rvs=lambda k: np.random.default_rng(4).integers(1, 6, k).astype(np.float64))
    A.sort_indices()
    labels = _labels(m, 2, 6)
    sess, Rm = _resident(A)
    g = _raw_groups(Rm, labels, 2, 0, ALL)
    ng = g["rows"].astype(np.float64)
    worst = 0.0
    for a, b in ((0, 1), (1, 0)):
        t, df = R.welch_pair(g["mean"][a], g["var"][a], int(ng[a]), g["mean"][b], g["var"][b], int(ng[b]))
        worst = max(worst, float(np.max(np.abs(g["t"][a] - t) / np.maximum(np.abs(t), 1e-300))))
        assert (np.abs(g["t"][a] - t) <= 16 * EPS * np.abs(t)).all() and (np.abs(g["df"][a] - df) <= 64 * EPS * df).all()
    print(f"t: worst relative deviation from the formula on the library's means and variances {worst:.3e}")


def test_t_against_scipy():
    m, n, K = 2000, 30, 3
    ptr, idx, val, labels = R.fixture(m, n, K + 1, 31, np.float64, "counts")      # (its last group is empty)
    A = sp.csr_matrix((val, idx, ptr), shape=(m, n))
    D = A.toarray()
    inc = (labels >= 0) & (labels < K + 1)
    ref = R.rank_groups(ptr, idx, val, m, n, labels, K + 1)
    sess, Rm = _resident(A)
    got = _raw_groups(Rm, labels, K + 1, 0, ("t", "df"))
    dev_ref, dev_got = 0.0, 0.0
    for g in range(K):
        res = scipy.stats.ttest_ind(D[inc & (labels == g)], D[inc & (labels != g)], equal_var=False)
        ok = np.isfinite(res.statistic) & (res.statistic != 0)
        dev_ref = max(dev_ref, float(np.max(np.abs(ref["t_score"][g][ok] - res.statistic[ok]) / np.abs(res.statistic[ok]))))
        dev_got = max(dev_got, float(np.max(np.abs(got["t"][g][ok] - res.statistic[ok]) / np.abs(res.statistic[ok]))))
    print(f"t against scipy: the restatement deviates by {dev_ref:.3e}, the library by {dev_got:.3e} (relative)")
    assert dev_got <= 100 * max(dev_ref, EPS)


def _separated(m, dt, seed):
    """columns whose values shift with the row's label, by 0.1 .. 12 standard deviations: |z| from a few to beyond 40"""
    rng = np.random.default_rng(seed)
    labels = _labels(m, 3, seed + 1)
    cols = []
    for shift in (0.1, 0.3, 1.0, 2.0, 4.0, 8.0, 12.0):
        rows = np.sort(rng.choice(m, m // 2, replace=False))
        cols.append((rows, (rng.normal(0.0, 1.0, rows.size) + shift * (labels[rows] == 1) - shift * (labels[rows] == 2)).astype(dt)))
    return _matrix(m, cols, dt), labels


def test_separated_groups_reach_the_tail_of_erfc():
    """p-values down to the subnormals and to 0: the same bars, with the erfc discrepancy measured over these z values
    (on the CPU over the restatement's z, |z| up to 41.8: 2.3e-14 relative, so 9.1e-14 is allowed)"""
    A, labels = _separated(6000, np.float64, 40)
    sess, Rm = _resident(A)
    got = Rm.rank_sums(labels, 3)
    want = R.rank_sums(*_arrays(A), 6000, A.shape[1], labels, 3)
    for k in ("group_rows", "rank_sum2", "nonzero", "tie_sum"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    g = _raw_groups(Rm, labels, 3, 1, ALL)
    assert np.abs(g["z"]).max() > 38 and g["pz"].min() == 0.0 and (g["pz"] > 1e-3).any()
    _check_scores(A, labels, 3, g, got, True)


@pytest.mark.parametrize("K", [1, R.MAX_GROUPS])
def test_one_group_and_the_most_groups(K):
    A = _case("counts", np.float32, seed=12, lens=[0, 100, 1000, 4500, M])
    labels = _labels(M, K, 8, single=K - 1 if K > 1 else None, empty=3 if K > 1 else None)
    sess, Rm = _resident(A)
    want = R.rank_sums(*_arrays(A), M, A.shape[1], labels, K)
    got = Rm.rank_sums(labels, K)
    for k in ("group_rows", "rank_sum2", "nonzero", "tie_sum"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    g = _raw_groups(Rm, labels, K, 1, ALL)
    _check_scores(A, labels, K, g, got, True)
    if K == 1:                                          # no rest
        assert not g["z"].any() and (g["pz"] == 1).all() and not g["t"].any() and not g["df"].any()


def test_a_group_that_holds_every_included_row_and_a_single_row():
    A = _case("real", np.float64, seed=2, m=700, lens=[0, 5, 300, 700])
    labels = np.ones(700, dtype=np.int32)
    labels[::9] = -1
    labels[4::11] = 3
    sess, Rm = _resident(A)
    g = _raw_groups(Rm, labels, 3, 0, ALL)
    assert g["rows"].tolist() == [0, int((labels == 1).sum()), 0]
    assert not g["z"].any() and (g["pz"] == 1).all() and not g["t"].any()
    got = Rm.rank_sums(labels, 3)
    want = R.rank_sums(*_arrays(A), 700, A.shape[1], labels, 3)
    np.testing.assert_array_equal(got["rank_sum2"], want["rank_sum2"])
    # m = 1
    one = sp.csr_matrix(np.array([[0.0, 2.5, -1.0]]))
    _, R1 = _resident(one)
    s1 = R1.rank_sums(np.zeros(1, dtype=np.int32), 2)
    assert s1["group_rows"].tolist() == [1, 0] and s1["rank_sum2"].tolist() == [[2, 2, 2], [0, 0, 0]]
    assert s1["nonzero"].tolist() == [[0, 1, 1], [0, 0, 0]] and not s1["tie_sum"].any()
    g1 = _raw_groups(R1, np.zeros(1, dtype=np.int32), 2, 1, ALL)
    assert not g1["z"].any() and (g1["pz"] == 1).all() and g1["mean"][0].tolist() == [0.0, 2.5, -1.0]


def test_device_labels_of_kmeans_in_place():
    m = 3000
    A = _case("counts", np.float32, seed=14, m=m, lens=[0, 50, 400, 3000])
    sess, Rm = _resident(A)
    X = torch.as_tensor(np.random.default_rng(1).normal(size=(m, 4)).astype(np.float32), device="cuda")
    labels = sess.kmeans(X, n_clusters=5)[0]
    assert labels.is_cuda and labels.dtype == torch.int32
    a = _raw_groups(Rm, labels, 5, 0, ALL)
    b = _raw_groups(Rm, labels.cpu().numpy(), 5, 0, ALL)
    assert all(a[k].tobytes() == b[k].tobytes() for k in ALL)
    km = sapca.KMeans(n_clusters=5).fit(X)
    r = Rm.rank_groups(km, method="both")                # the estimator's device labels, K from them
    assert r.group_rows.tolist() == np.bincount(km.labels_.cpu().numpy(), minlength=5).tolist()
    np.testing.assert_array_equal(R.rank_sums(*_arrays(A), m, A.shape[1], labels.cpu().numpy(), 5)["rank_sum2"],
                                  Rm.rank_sums(labels, 5)["rank_sum2"])


def test_a_fitted_estimator_is_untouched():
    m, n, k = 3000, 400, 6
    dev = synth.gapped_csr(m, n, 0.08, k, seed=5, dtype=torch.float32, device="cuda:0")
    est = (sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Random(4, 2, PIN.QR)).build()
           .set_omega(synth.gaussian_panel(n, k + 4, 3).numpy()))
    csr = sapca.DeviceCsr(*dev, (m, n))
    est.fit_transform(csr)
    before = est.transform(csr).cpu().numpy()
    comps = est.components_(np.float64).copy()
    sess = ops.Session.borrow(est._h)
    Rm = ops.ResidentCsr(sess, (m, n), dev[2].numel(), np.float32, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr())
    labels = _labels(m, 4, 2)
    got = Rm.rank_sums(labels, 4)
    ptr, idx, val = (x.cpu().numpy() for x in dev)
    want = R.rank_sums(ptr.astype(np.int64), idx.astype(np.int64), val, m, n, labels, 4)
    np.testing.assert_array_equal(got["rank_sum2"], want["rank_sum2"])
    assert est.transform(csr).cpu().numpy().tobytes() == before.tobytes()
    np.testing.assert_array_equal(est.components_(np.float64), comps)


def test_selection_and_canonical_buffers_as_sources():
    m = 2000
    A = _case("real", np.float32, seed=21, m=m, lens=[0, 10, 300, 1500])
    n = A.shape[1]
    sess, Rm = _resident(A)
    keep = np.random.default_rng(5).random(m) < 0.6
    S = Rm.select_rows(keep)
    labels = _labels(int(keep.sum()), 4, 9)
    want = R.rank_sums(*_arrays(A[keep]), int(keep.sum()), n, labels, 4)
    got = S.rank_sums(labels, 4)
    for k in ("group_rows", "rank_sum2", "nonzero", "tie_sum"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    # rows stored in descending column order: canonicalised on the device, then ranked
    ptr, idx, val = _arrays(A)
    ridx, rval = idx.copy(), val.copy()
    for i in range(m):
        ridx[ptr[i]:ptr[i + 1]] = idx[ptr[i]:ptr[i + 1]][::-1]
        rval[ptr[i]:ptr[i + 1]] = val[ptr[i]:ptr[i + 1]][::-1]
    _, U = _resident(sp.csr_matrix((rval, ridx, ptr), shape=(m, n)), ops.Session())
    Cn, rep = U.canonicalize()
    assert "UNSORTED" in rep.flags and Cn is not U
    lab2 = _labels(m, 3, 10)
    np.testing.assert_array_equal(Cn.rank_sums(lab2, 3)["rank_sum2"], R.rank_sums(ptr, idx, val, m, n, lab2, 3)["rank_sum2"])


def test_refusals_name_the_number_and_leave_the_handle_usable():
    A = _case("counts", np.float64, seed=30, m=500, lens=[0, 3, 100, 500])
    sess, Rm = _resident(A)
    labels = _labels(500, 3, 1)
    d = torch.as_tensor(labels, device="cuda")
    want = R.rank_sums(*_arrays(A), 500, A.shape[1], labels, 3)
    lib = L.load()
    h, m, n, nnz, p, i, v = Rm._args()
    rows = np.zeros(4, dtype=np.uint64)

    def sums(m_=m, labels_=C.c_void_p(d.data_ptr()), K=3):
        return lib.sapca_rank_sums_csr_device_f64(h, m_, n, nnz, p, i, v, labels_, C.c_uint32(K), ops._p(rows, C.c_uint64), None, None, None)

    def groups(tc):
        return lib.sapca_rank_groups_csr_device_f64(h, m, n, nnz, p, i, v, C.c_void_p(d.data_ptr()), C.c_uint32(3), C.c_int32(tc),
                                                    ops._p(rows, C.c_uint64), None, None, None, None, None, None, None)

    def last():
        return lib.sapca_last_error(h).decode()

    for call, words in ((lambda: sums(K=0), ("n_groups is 0",)),
                        (lambda: sums(K=1025), ("1025", "SAPCA_RANK_MAX_GROUPS = 1024")),
                        (lambda: sums(m_=C.c_uint64(2 ** 31)), (str(2 ** 31), "rows")),
                        (lambda: groups(2), ("tie_correct = 2",)),
                        (lambda: groups(-1), ("tie_correct = -1",)),
                        (lambda: sums(labels_=None), ("d_labels is NULL", "m = 500")),
                        (lambda: lib.sapca_rank_sums_csr_device_f64(h, m, n, nnz, None, i, v, C.c_void_p(d.data_ptr()), C.c_uint32(3),
                                                                    ops._p(rows, C.c_uint64), None, None, None), ("null CSR array",))):
        assert call() == L.ERR_ARG
        assert all(w in last() for w in words), last()
        np.testing.assert_array_equal(Rm.rank_sums(labels, 3)["rank_sum2"], want["rank_sum2"])   # a checked call on the same handle
    with pytest.raises(ValueError, match="n_groups"):
        Rm.rank_sums(labels, 0)
    # an empty shape is valid
    zeros = torch.zeros(8, dtype=torch.int64, device="cuda")
    E = ops.ResidentCsr(sess, (0, 4), 0, np.float64, zeros.data_ptr(), 0, 0)
    e = E.rank_sums(np.zeros(0, dtype=np.int32), 2)
    assert not e["group_rows"].any() and not e["rank_sum2"].any() and e["rank_sum2"].shape == (2, 4)
    E2 = ops.ResidentCsr(sess, (5, 0), 0, np.float64, zeros.data_ptr(), 0, 0)
    assert E2.rank_sums(np.array([0, 1, 1, -1, 7], dtype=np.int32), 2)["group_rows"].tolist() == [1, 2]
    np.testing.assert_array_equal(Rm.rank_sums(labels, 3)["rank_sum2"], want["rank_sum2"])

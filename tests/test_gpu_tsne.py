"""t-SNE of device-resident rows (-m gpu): sapca_tsne_* through Session.tsne_affinities / tsne_gradient / tsne_embed / tsne.

The reference is tests/tsne_ref.py (numpy, f64; held to scikit-learn's gradient and KL by tests/test_tsne_cpu.py).

Tolerances of the gradient and trajectory tests are measured here, on the CPU, from the reference alone and before the GPU
result is looked at: `spread64` is how far the reference moves when every sum over j runs in the opposite order, `spread32`
how far the restatement with f32 pair arithmetic and f32 sums is from the f64 one.  The GPU's tile order is a third order,
so it is granted 16 x the spread.  Where the reference's two orders agree exactly (two rows: one addend per sum) the spread
is 0 although a fused multiply-add already rounds differently, so where the measured spread is below ONE rounding of the
largest term of the sum it bounds (the unit roundoff eps / 2 of the arithmetic times that term) that one rounding takes its
place; it comes from the number format and the reference's terms, not from the code under test.  Every case prints which of
the two set its tolerance ("spread" or "one rounding"); DESIGN.md, "t-SNE", records how many cases each governed.
Measured spreads and the largest GPU error: DESIGN.md, "t-SNE"."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import knn_ref as KR
import tsne_ref as TR
import sapca
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
IDS = dict(ids=["f32", "f64"])
DTYPES = [np.float32, np.float64]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def sess():
    return ops.Session()


@pytest.fixture(scope="module")
def gold(golden):
    g = dict(golden("g8_tsne.npz"))
    m = g["X"].shape[0]
    g["P"] = sp.csr_matrix((g["P_data"], g["P_indices"], g["P_indptr"]), shape=(m, m))
    return g


def _resident(sess, P, dt):
    """a scipy CSR as a ResidentCsr of dtype dt on the session (the caller's own arrays, adopted)"""
    P = sp.csr_matrix(P)
    return ops.ResidentCsr.from_torch(sess, _dev(P.indptr.astype(np.int64)), _dev(P.indices.astype(np.int32)), _dev(P.data.astype(dt)),
                                      P.shape)


def _host_csr(P):
    d = P.as_device_csr()
    return sp.csr_matrix((d.values.cpu().numpy(), d.col_indices.cpu().numpy(), d.row_offsets.cpu().numpy()), shape=P.shape)


# ------------------------------------------------------------------ 1. affinities
def _affinity_case(gold, which):
    if which == "fixture":
        return gold["indices"], gold["dist"], float(gold["perplexity"])
    X = TR.clusters(31, 4, 11)[0]                      # m = K + 1: every row is everyone's neighbour
    idx, dist = KR.knn(X, X, 30, "euclidean", exclude_self=True)
    return idx.astype(np.int32), dist, 10.0


def _check_affinities(P, beta, idx, dist_t, perp, dt):
    """the returned graph against the rows numpy recomputes from the returned beta and the distances as the library saw
    them (distances of unfilled slots are never looked at); returns the host copy"""
    m, K = idx.shape
    got = _host_csr(P)
    ok = (idx >= 0) & (idx < m)
    D = np.where(ok, dist_t.astype(np.float64), 0.0) ** 2
    rows = [TR.entropy_gap(D[i], ok[i], beta[i], perp) for i in range(m)]
    gaps = np.array([r[0] for r in rows])
    print(f"largest |H - ln perplexity| {np.abs(gaps).max():.3e}")
    assert np.abs(gaps).max() < 1e-5                                           # the search's own stopping rule
    want = TR.symmetrise(idx, np.stack([r[1] for r in rows]), dt)
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    ulps = np.abs(got.data.astype(np.float64) - want.data.astype(np.float64)) / np.spacing(np.abs(want.data))
    print(f"largest value error {ulps.max():.2f} ulp")
    assert ulps.max() <= 2
    assert got.data.dtype == np.dtype(dt)
    rep = P.check()
    assert rep.canonical, rep
    assert (got != got.T).nnz == 0                                             # P_ij == P_ji bit for bit
    assert abs(got.data.astype(np.float64).sum() - 1.0) <= (1e-12 if dt == np.float64 else 1e-6)
    return got


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("which", ["fixture", "m_is_K_plus_1"])
def test_affinities(sess, gold, which, dt):
    idx, dist, perp = _affinity_case(gold, which)
    m, K = idx.shape
    dist_t = dist.astype(dt)
    P, beta = sess.tsne_affinities(_dev(idx), _dev(dist_t), perp)
    beta = beta.cpu().numpy()
    got = _check_affinities(P, beta, idx, dist_t, perp, dt)
    first = (got.indptr.tobytes(), got.indices.tobytes(), got.data.tobytes(), beta.tobytes())
    listed = sp.csr_matrix((np.ones(m * K), (np.repeat(np.arange(m), K), idx.ravel())), shape=(m, m))
    mutual = listed.multiply(listed.T).nnz
    if which == "fixture":
        assert 0 < mutual < listed.nnz                                         # mutual and one-sided neighbours both occur
    else:
        assert mutual == listed.nnz == m * (m - 1)
    assert got.nnz == 2 * listed.nnz - mutual
    P2, beta2 = sess.tsne_affinities(_dev(idx), _dev(dist_t), perp)
    again = _host_csr(P2)
    assert (again.indptr.tobytes(), again.indices.tobytes(), again.data.tobytes(), beta2.cpu().numpy().tobytes()) == first


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_unfilled_slots_contribute_nothing(sess, gold, dt):
    idx, dist, perp = gold["indices"].copy(), gold["dist"].astype(dt), 5.0
    idx[::7, 20:] = -1                                                         # as the search leaves a slot it could not fill
    dist[::7, 20:] = np.nan
    P, beta = sess.tsne_affinities(_dev(idx), _dev(dist), perp)
    got = _check_affinities(P, beta.cpu().numpy(), idx, dist, perp, dt)
    assert np.isfinite(got.data).all() and np.isfinite(beta.cpu().numpy()).all()


def _bytes_of(P, beta):
    got = _host_csr(P)
    return got.indptr.tobytes(), got.indices.tobytes(), got.data.tobytes(), beta.cpu().numpy().tobytes()


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_affinities_through_every_length_class_of_the_row_sort(sess, dt):
    """hand-made lists: one raw row beyond canon_lds_cap() that merges mutual pairs, one between 65 entries and the cap"""
    idx, dist = TR.hub_lists()
    m, K = idx.shape
    counts, merged = TR.sort_classes(idx)
    print(f"rows that need the sort per length class {counts}, merged entries {merged}")
    assert all(c > 0 for c in counts) and merged > 0                           # from the lists alone, before the GPU runs
    assert np.isin(idx[0], np.nonzero((idx == 0).any(axis=1))[0]).all()        # the long row lists rows that list it back
    dist_t = dist.astype(dt)
    P, beta = sess.tsne_affinities(_dev(idx), _dev(dist_t), 2.0)
    got = _check_affinities(P, beta.cpu().numpy(), idx, dist_t, 2.0, dt)
    assert got.nnz == 2 * m * K - merged and np.diff(got.indptr)[0] == m - 1
    assert _bytes_of(*sess.tsne_affinities(_dev(idx), _dev(dist_t), 2.0)) == _bytes_of(P, beta)


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_affinities_of_a_directed_ring_merge_nothing(sess, dt):
    """K = 1, no mutual pair: every row is sorted, none merges, and the offsets stay the raw ones"""
    m = 65
    idx = ((np.arange(m) + 1) % m).astype(np.int32)[:, None]
    dist_t = np.random.default_rng(65).uniform(0.5, 1.5, size=(m, 1)).astype(np.float32).astype(dt)
    assert TR.sort_classes(idx) == ([m - 2, 0, 0], 0)                          # (rows 0 and m - 1 are ascending as emitted)
    P, beta = sess.tsne_affinities(_dev(idx), _dev(dist_t), 1.0)
    got = _check_affinities(P, beta.cpu().numpy(), idx, dist_t, 1.0, dt)
    assert got.nnz == 2 * m
    np.testing.assert_array_equal(got.indptr, 2 * np.arange(m + 1))
    assert _bytes_of(*sess.tsne_affinities(_dev(idx), _dev(dist_t), 1.0)) == _bytes_of(P, beta)


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_affinities_without_a_valid_slot_are_an_empty_graph(sess, dt):
    m, K = 8, 3
    idx = np.full((m, K), -1, dtype=np.int32)
    dist_t = np.full((m, K), np.nan, dtype=dt)
    P, beta = sess.tsne_affinities(_dev(idx), _dev(dist_t), 2.0)
    got = _host_csr(P)
    assert got.shape == (m, m) and got.nnz == 0 and (got.indptr == 0).all() and got.data.dtype == np.dtype(dt)
    assert np.isfinite(beta.cpu().numpy()).all()
    assert P.check().canonical
    assert _bytes_of(*sess.tsne_affinities(_dev(idx), _dev(dist_t), 2.0)) == _bytes_of(P, beta)


# ------------------------------------------------------------------ 2. gradient
_GRAD = {}


def _graph(m):
    """an affinity matrix on m rows (random points, up to 15 neighbours), built by the reference"""
    X = np.random.default_rng(1000 + m).normal(size=(m, 5))
    K = min(m - 1, 15)
    idx, dist = KR.knn(X, X, K, "euclidean", exclude_self=True)
    return TR.symmetrise(idx, TR.conditional(idx, dist, max(1.0, K / 3.0))[0])


def _grad_case(m, D, scale, e):
    """the reference at one point, once: P, Y (f32-representable, so both dtypes see the same numbers), the f64 result and
    the two spreads with their floors"""
    key = (m, D, scale, e)
    if key not in _GRAD:
        P = _graph(m)
        Y = (scale * np.random.default_rng(7 * m + D).normal(size=(m, D))).astype(np.float32).astype(np.float64)
        g, Z, kl = TR.gradient(P, Y, e)
        gr, Zr, klr = TR.gradient(P, Y, e, reverse=True)
        g32, Z32, kl32 = TR.gradient(P, Y, e, arith=np.float32)
        # the largest term of each sum: one rounding of it is the least two evaluation orders can differ by
        minus_rep = TR.gradient(P, Y, 0.0)[0]                                  # e = 0 leaves -repulsion / Z
        top = np.abs(g - minus_rep).max() + np.abs(minus_rep).max()            # e * attraction, repulsion / Z
        _GRAD[key] = dict(P=P, Y=Y, g=g, Z=Z, kl=kl, top=top,
                          s64=(np.abs(g - gr).max(), abs(Z - Zr) / Z, abs(kl - klr)),
                          s32=(np.abs(g32 - g).max(), abs(Z32 - Z) / Z, abs(kl32 - kl)))
    return _GRAD[key]


GRAD_M = [2, 63, 64, 65, 257, 1500]        # 1500: two j tiles, few i blocks -- the j-split route by shape


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("e", [1.0, 12.0])
@pytest.mark.parametrize("scale", [1e-4, 10.0])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("m", GRAD_M)
def test_gradient_against_the_reference(sess, m, D, scale, e, dt):
    c = _grad_case(m, D, scale, e)
    u = float(np.finfo(dt).eps) / 2                                            # one rounding: the unit roundoff
    spread = c["s64"] if dt == np.float64 else tuple(max(a, b) for a, b in zip(c["s64"], c["s32"]))
    # the KL is an average of logarithms (sum P = 1) of about ln Z: one rounding of that, and what a rounded argument moves a logarithm by
    one = (u * c["top"], u, u * (1.0 + max(abs(c["kl"]), abs(math.log(c["Z"])))))
    tol_g, tol_z, tol_kl = (16 * max(sp_, r) for sp_, r in zip(spread, one))
    by = "/".join("spread" if sp_ >= r else "one rounding" for sp_, r in zip(spread, one))
    grad, Z, kl = sess.tsne_gradient(_resident(sess, c["P"], dt), _dev(c["Y"].astype(dt)), e)
    err = np.abs(grad.cpu().numpy().astype(np.float64) - c["g"]).max()
    print(f"m={m} D={D} scale={scale} e={e} {np.dtype(dt).name}: spread64 {c['s64'][0]:.3e} spread32 {c['s32'][0]:.3e} one rounding {one[0]:.3e} (g/Z/kl set by {by}) "
          f"gpu error {err:.3e} (of {tol_g:.3e}); Z rel {abs(Z - c['Z']) / c['Z']:.3e} (of {tol_z:.3e}); kl {abs(kl - c['kl']):.3e} (of {tol_kl:.3e})")
    assert grad.dtype == DT[np.dtype(dt)] and tuple(grad.shape) == (m, D)
    assert err <= tol_g
    assert abs(Z - c["Z"]) / c["Z"] <= tol_z
    assert abs(kl - c["kl"]) <= tol_kl


@pytest.mark.parametrize("m", [257, 1500])
def test_z_of_integer_coordinates_is_exact_to_rounding(sess, m):
    rng = np.random.default_rng(m)
    Y = rng.integers(0, 40, size=(m, 2)).astype(np.float64)                   # coincident rows occur
    d2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    off = ~np.eye(m, dtype=bool)
    want = math.fsum((1.0 / (1.0 + d2[off])).tolist())
    ring = sp.csr_matrix((np.full(2 * m, 2.0 ** -10), (np.repeat(np.arange(m), 2), np.stack([(np.arange(m) + 1) % m, (np.arange(m) - 1) % m], 1).ravel())),
                         shape=(m, m))
    ring.sort_indices()
    grad, Z, kl = sess.tsne_gradient(_resident(sess, ring, np.float64), _dev(Y), 1.0)
    print(f"m={m}: Z relative error {abs(Z - want) / want:.3e}")
    assert abs(Z - want) <= 1e-15 * want
    assert np.isfinite(grad.cpu().numpy()).all() and np.isfinite(kl)


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_coincident_rows_count_in_z_and_exert_no_force(sess, dt):
    m = 130
    P = _graph(m)
    Y = np.random.default_rng(3).normal(size=(m, 2)).astype(np.float32).astype(np.float64)
    Y[65:] = Y[:65]                                                            # every row twice
    g, Z, kl = TR.gradient(P, Y, 1.0)
    grad, gz, gkl = sess.tsne_gradient(_resident(sess, P, dt), _dev(Y.astype(dt)), 1.0)
    grad = grad.cpu().numpy()
    assert np.isfinite(grad).all() and np.isfinite(gz) and np.isfinite(gkl)
    eps = float(np.finfo(dt).eps)
    assert abs(gz - Z) <= 64 * eps * Z                                         # the 2 * 65 coincident pairs count 1 each
    assert gz > 130.0
    np.testing.assert_allclose(grad, g, atol=64 * eps * np.abs(g).max())
    # all rows in one place: Z = m (m - 1), no force at all
    same = np.zeros((m, 2))
    grad, gz, gkl = sess.tsne_gradient(_resident(sess, P, dt), _dev(same.astype(dt)), 12.0)
    assert gz == m * (m - 1) and (grad.cpu().numpy() == 0).all() and np.isfinite(gkl)


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("m", [1500, 2500, 9000])
def test_split_and_unsplit_routes_give_the_same_bytes(debug_switches, monkeypatch, m, dt):
    D = 2 if m != 2500 else 3
    rng = np.random.default_rng(m)
    Y = _dev((5.0 * rng.normal(size=(m, D))).astype(dt))
    K = 4
    cols = (np.arange(m)[:, None] + np.arange(1, K + 1)[None, :]) % m
    C0 = sp.csr_matrix((np.full(m * K, 1.0 / (2 * m * K)), (np.repeat(np.arange(m), K), cols.ravel())), shape=(m, m))
    P = (C0 + C0.T).tocsr()
    P.sort_indices()
    out = {}
    for split in ("0", "1"):
        monkeypatch.setenv("SAPCA_TSNE_SPLIT", split)
        s = ops.Session()
        grad, Z, kl = s.tsne_gradient(_resident(s, P, dt), Y, 1.0)
        out[split] = (grad.cpu().numpy().tobytes(), Z, kl)
    assert out["0"] == out["1"]
    monkeypatch.delenv("SAPCA_TSNE_SPLIT")
    s = ops.Session()
    grad, Z, kl = s.tsne_gradient(_resident(s, P, dt), Y, 1.0)                 # and the route the shape alone picks
    assert (grad.cpu().numpy().tobytes(), Z, kl) == out["0"]


# ------------------------------------------------------------------ 3. trajectory
def test_twenty_epochs_follow_the_reference(sess, gold):
    epochs = int(gold["epochs"])
    Yr, klr = TR.embed(gold["P"], gold["Y0"], epochs, reverse=True)
    spread = np.abs(Yr - gold["Y20"]).max()
    Y, kl = sess.tsne_embed(_resident(sess, gold["P"], np.float64), epochs=epochs, init=_dev(gold["Y0"]))
    err = np.abs(Y.cpu().numpy() - gold["Y20"]).max()
    print(f"reordered reference after {epochs} epochs: {spread:.3e}; gpu error {err:.3e} (of {16 * spread:.3e}); max |Y| {np.abs(gold['Y20']).max():.3e}")
    assert err <= 16 * spread
    assert abs(kl - float(gold["kl20"])) <= 16 * max(abs(klr - float(gold["kl20"])), np.finfo(np.float64).eps * abs(klr))


# ------------------------------------------------------------------ 4. end to end
@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_three_clusters_end_to_end(sess, dt):
    X, labels = TR.clusters(600, 10, 3)
    x = _dev(X.astype(dt))
    Y0, kl0 = sess.tsne(x, perplexity=20.0, epochs=0)
    Y, kl = sess.tsne(x, perplexity=20.0, epochs=300)
    y = Y.cpu().numpy().astype(np.float64)
    assert Y.dtype == DT[np.dtype(dt)] and tuple(Y.shape) == (600, 2)
    nn = KR.knn(y, y, 1, "euclidean", exclude_self=True)[0][:, 0]
    share = (labels[nn] == labels).mean()
    print(f"{np.dtype(dt).name}: KL {kl0:.4f} -> {kl:.4f}; nearest embedded neighbour shares the label for {100 * share:.2f} %")
    assert share >= 0.99
    assert np.isfinite(kl) and kl < kl0
    # columns have mean 0 to 1e-9 max|y|.  In f32 that cannot hold for the stored values: y_i - mean (the mean exact to f64
    # rounding) is rounded to f32 once, an error of at most eps32 / 2 = 2^-24 of |y_i - mean| each, so the mean of the stored
    # column is the mean of those errors: at most 2^-24 max|y| (+ the f64 mean's own 1e-16).  That derived bound is asserted
    # for f32 (a stated deviation: sapca.h, DESIGN.md "t-SNE"); the f32 values recentred once more in f64 must meet 1e-9 too
    tol = 1e-9 if dt == np.float64 else 2.0 ** -24 + 1e-15
    means = np.abs(y.mean(axis=0)).max() / np.abs(y).max()
    print(f"{np.dtype(dt).name}: largest |column mean| / max|y| {means:.3e} (of {tol:.3e})")
    assert means <= tol
    Y2, kl2 = sess.tsne(x, perplexity=20.0, epochs=300)
    assert Y2.cpu().numpy().tobytes() == Y.cpu().numpy().tobytes() and kl2 == kl
    Y3, _ = sess.tsne(x, perplexity=20.0, epochs=300, seed=7)
    assert Y3.cpu().numpy().tobytes() != Y.cpu().numpy().tobytes()
    est = sapca.TSNE(perplexity=20.0, epochs=300, random_seed=42)
    assert est.fit_transform(x).cpu().numpy().tobytes() == Y.cpu().numpy().tobytes() and est.kl_divergence_ == kl


# ------------------------------------------------------------------ 5. routes
@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_host_route_device_route_and_the_stages_by_hand_agree_bit_for_bit(sess, gold, dt):
    X = gold["X"].astype(dt)
    perp, epochs = 10.0, 30
    Yh, klh = sess.tsne(X, perplexity=perp, epochs=epochs, output_dim=3)
    assert isinstance(Yh, np.ndarray) and Yh.dtype == np.dtype(dt)
    x = _dev(X)
    Yd, kld = sess.tsne(x, perplexity=perp, epochs=epochs, output_dim=3)
    assert Yd.cpu().numpy().tobytes() == Yh.tobytes() and kld == klh
    idx, dist = sess.knn(x, None, 30)
    P, _ = sess.tsne_affinities(idx, dist, perp)
    Ys, kls = sess.tsne_embed(P, epochs=epochs, output_dim=3)
    assert Ys.cpu().numpy().tobytes() == Yh.tobytes() and kls == klh
    # a caller's initial embedding, through both routes
    init = (1e-2 * np.random.default_rng(5).normal(size=(X.shape[0], 3))).astype(dt)
    Yi, _ = sess.tsne(X, perplexity=perp, epochs=epochs, output_dim=3, init=init)
    Yj, _ = sess.tsne(x, perplexity=perp, epochs=epochs, output_dim=3, init=_dev(init))
    assert Yi.tobytes() == Yj.cpu().numpy().tobytes() and Yi.tobytes() != Yh.tobytes()


# ------------------------------------------------------------------ 6. refusals
def _raw_tsne(sess, dt, m, x, ldx, d, o, y):
    fn = getattr(L.load(), f"sapca_tsne_device_{'f32' if dt == np.float32 else 'f64'}")
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)   # noqa: E731
    kl = C.c_double()
    torch.cuda.synchronize()
    st = fn(sess._h, C.c_uint64(m), p(x), C.c_uint64(ldx), C.c_uint64(d), C.byref(o), p(y), C.byref(kl))
    return st, (L.load().sapca_last_error(sess._h) or b"").decode(), kl.value


def _options(**changes):
    o = L.default_tsne_options()
    o.perplexity, o.epochs = 5.0, 5
    for k, v in changes.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_refusals_leave_the_handle_usable(dt):
    sess = ops.Session()
    X = TR.clusters(40, 6, 2)[0].astype(dt)
    x = _dev(X)
    y = torch.full((40, 2), -7.0, dtype=DT[np.dtype(dt)], device="cuda")
    ok = dict(m=40, x=x, ldx=6, d=6, y=y)
    st, msg, kl_ok = _raw_tsne(sess, dt, o=_options(), **ok)
    assert st == L.OK, msg
    good = y.cpu().numpy().tobytes()
    y.fill_(-7.0)
    cases = [
        (dict(), dict(struct_size=80), "options->struct_size is 80"),
        (dict(), dict(output_dim=0), "output_dim = 0 is outside 1 .. 3"),
        (dict(), dict(output_dim=4), "output_dim = 4 is outside 1 .. 3"),
        (dict(), dict(perplexity=float("nan")), "perplexity = nan must be finite and at least 1"),
        (dict(), dict(perplexity=0.5), "perplexity = 0.5 must be finite and at least 1"),
        (dict(), dict(perplexity=43.0), "perplexity 43 needs 129 neighbours, at most 128"),
        (dict(), dict(perplexity=20.0), "perplexity too large for the number of rows"),
        (dict(m=2 ** 31), dict(), f"m = {2 ** 31} rows"),
        (dict(d=0), dict(), "d is 0"),
        (dict(d=1025, ldx=2000), dict(), "d = 1025 exceeds 1024"),
        (dict(ldx=5), dict(), "ldx = 5 is less than d = 6"),
        (dict(ldx=2 ** 28), dict(), f"a row stride of {2 ** 28} elements; 2^28 or more are not supported"),
        (dict(), dict(theta=-0.5), "theta = -0.5 must not be negative"),
        (dict(), dict(theta=float("nan")), "theta = nan must not be negative"),
        (dict(), dict(init_given=2), "init_given = 2 is neither 0 nor 1"),
        (dict(), dict(learning_rate=-1.0), "learning_rate = -1 must be finite and not negative"),
        (dict(), dict(momentum=float("inf")), "momentum = inf must be finite and not negative"),
        (dict(), dict(final_momentum=float("nan")), "final_momentum = nan must be finite and not negative"),
        (dict(), dict(exaggeration=-12.0), "exaggeration = -12 must be finite and not negative"),
        (dict(x=None), dict(), "a NULL panel with m = 40"),
        (dict(y=None), dict(), "a NULL panel with m = 40"),
    ]
    for change, opt, message in cases:
        st, msg, _ = _raw_tsne(sess, dt, o=_options(**opt), **{**ok, **change})
        assert st == L.ERR_ARG and message in msg, f"{change} {opt}: status {st}, message {msg!r}"
        assert (y == -7).all(), f"{change} {opt}: the output was written"
        st, msg, kl = _raw_tsne(sess, dt, o=_options(), **ok)                   # the same handle, straight after
        assert st == L.OK, msg
        assert y.cpu().numpy().tobytes() == good and kl == kl_ok
        y.fill_(-7.0)
    # the stage calls refuse the same way
    with pytest.raises(L.SapcaError, match="K = 129 neighbours per row is outside 1 .. 128"):
        sess.tsne_affinities(torch.zeros((200, 129), dtype=torch.int32, device="cuda"), torch.zeros((200, 129), dtype=DT[np.dtype(dt)], device="cuda"), 5.0)
    with pytest.raises(L.SapcaError, match="output_dim = 4 is outside 1 .. 3"):
        sess.tsne_gradient(_resident(sess, _graph(40), dt), torch.zeros((40, 4), dtype=DT[np.dtype(dt)], device="cuda"))
    fn = getattr(L.load(), f"sapca_tsne_gradient_device_{'f32' if dt == np.float32 else 'f64'}")
    P = _resident(sess, _graph(40), dt)
    grad = torch.full((40, 2), -7.0, dtype=DT[np.dtype(dt)], device="cuda")
    for ldy, message in ((1, "ldy = 1 is less than output_dim = 2"), (2 ** 28, f"a row stride of {2 ** 28} elements; 2^28 or more are not supported")):
        st = fn(sess._h, C.c_uint64(40), C.c_uint64(P.nnz), C.c_void_p(P.d_ptr), C.c_void_p(P.d_idx), C.c_void_p(P.d_val),
                C.c_void_p(y.data_ptr()), C.c_uint64(ldy), C.c_uint32(2), C.c_double(1.0), C.c_void_p(grad.data_ptr()), None, None)
        msg = (L.load().sapca_last_error(sess._h) or b"").decode()
        assert st == L.ERR_ARG and message in msg, msg
        assert (grad == -7).all()
    st, msg, _ = _raw_tsne(sess, dt, o=_options(), **ok)
    assert st == L.OK and y.cpu().numpy().tobytes() == good


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_a_single_row_has_no_repulsion_and_no_nan(sess, dt):
    """m = 1: Z = 0 (no pair); the gradient is 0, the embedding the origin, the KL 0 -- for the stage calls, which accept it"""
    P = _resident(sess, sp.csr_matrix((1, 1)), dt)
    grad, Z, kl = sess.tsne_gradient(P, _dev(np.array([[3.0, -4.0]], dtype=dt)), 12.0)
    assert Z == 0.0 and kl == 0.0 and (grad.cpu().numpy() == 0).all()
    Y, kl = sess.tsne_embed(P, epochs=3)
    assert (Y.cpu().numpy() == 0).all() and kl == 0.0


def test_zero_epochs_return_the_initial_embedding_recentred(sess, gold):
    P = _resident(sess, gold["P"], np.float64)
    init = gold["Y1"] + np.array([3.0, -2.0])
    Y, kl = sess.tsne_embed(P, epochs=0, init=_dev(init))
    want = init - init.mean(axis=0)
    np.testing.assert_allclose(Y.cpu().numpy(), want, atol=4 * np.finfo(np.float64).eps * np.abs(init).max())
    assert abs(kl - TR.gradient(gold["P"], want, 1.0)[2]) <= 1e-12 * abs(kl)
    Yb, klb = sess.tsne_embed(P, epochs=0)                                     # built-in start: 1e-4 N(0, 1) under the session's seed
    want_b = TR.initial_embedding(300, 2, 42)
    want_b -= want_b.mean(axis=0)
    np.testing.assert_allclose(Yb.cpu().numpy(), want_b, atol=1e-18)
    assert np.isfinite(klb)


# ------------------------------------------------------------------ 7. a fitted estimator, a communicator
def _estimator(k, omega):
    return (sapca.SparsePCABuilder.new().n_components(k).svd_method(SVDMethod.Random(4, 2, PIN.QR))
            .transform_semantics(L.TRANSFORM_CENTERED).build().set_omega(omega))


def test_a_fitted_estimator_is_untouched_by_an_embedding_of_its_scores(sess):
    m, n, k = 1200, 300, 8
    ptr, idx, val = (x.cpu().numpy() for x in synth.gapped_csr(m, n, 0.08, k, seed=5, dtype=torch.float32))
    est = _estimator(k, synth.gaussian_panel(n, k + 4, 3).numpy())
    dev = sapca.DeviceCsr(_dev(ptr.astype(np.int64)), _dev(idx.astype(np.int32)), _dev(val), (m, n))
    scores = est.fit_transform(dev)
    before = est.transform(dev).cpu().numpy()
    getters = [est.components_(np.float64).copy(), est.explained_variance_ratio(np.float64).copy(), est.mean_(np.float64).copy(),
               est.singular_values_(np.float64).copy()]
    Y, kl = est.session().tsne(scores, perplexity=10.0, epochs=25, seed=42)
    Yw, klw = sess.tsne(scores.clone(), perplexity=10.0, epochs=25, seed=42)     # the same rows on a bare handle
    assert Y.cpu().numpy().tobytes() == Yw.cpu().numpy().tobytes() and kl == klw and np.isfinite(kl)
    Yc, _ = est.session().tsne(scores[:, :4], perplexity=10.0, epochs=5)      # a column slice, searched in place
    assert np.isfinite(Yc.cpu().numpy()).all()
    assert est.transform(dev).cpu().numpy().tobytes() == before.tobytes()
    after = [est.components_(np.float64), est.explained_variance_ratio(np.float64), est.mean_(np.float64), est.singular_values_(np.float64)]
    for a, b in zip(getters, after):
        assert a.tobytes() == b.tobytes()


def test_a_handle_in_a_communicator_embeds_locally(sess):
    calls = []

    def allreduce(sendbuf, recvbuf, count, dtype, user):
        calls.append(count)
        return 0

    est = _estimator(4, synth.gaussian_panel(50, 8, 1).numpy())
    est.comm_set_callback(2, 0, allreduce)                       # rank 0 of 2: the handle belongs to a communicator
    X = _dev(TR.clusters(200, 7, 9)[0].astype(np.float32))
    Y, kl = est.session().tsne(X, perplexity=8.0, epochs=20, seed=42)
    Yw, klw = sess.tsne(X, perplexity=8.0, epochs=20, seed=42)
    assert Y.cpu().numpy().tobytes() == Yw.cpu().numpy().tobytes() and kl == klw
    assert not calls

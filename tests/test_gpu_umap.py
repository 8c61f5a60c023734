"""UMAP of device-resident rows (-m gpu): sapca_umap_* through Session.umap_graph / umap_embed / umap and sapca.UMAP.

The reference is tests/umap_ref.py (numpy, f64; tests/test_umap_cpu.py holds its curve fit to scipy and its fixture fixed).

Graph: rho is exact and sigma bit-identical wherever the floor does not govern (every decision of the fixture's searches
clears its threshold by 1e-9, tests/test_umap_cpu.py); a floored sigma is a sum in another order: K eps_f64 relative for a
row's own K-term sum, m K eps_f64 where rho is 0 and the floor is the panel's m K-term sum.  The values are then compared,
to 2 ulp of T, with the union numpy forms from the memberships at the RETURNED sigma (as the t-SNE test does with beta).

Trajectory: the tolerance is measured here, on the CPU, from the reference alone and before the GPU result is looked at:
16 x how far the restatement moves when every vertex adds its terms in the opposite order and takes s^b as exp(b ln s), in
the same storage.  Every case prints both figures.  Measured spreads and the largest GPU errors: DESIGN.md, "UMAP"."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import knn_ref as KR
import umap_ref as UR
import sapca
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
IDS = dict(ids=["f32", "f64"])
DTYPES = [np.float32, np.float64]
EPS = np.finfo(np.float64).eps


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def sess():
    return ops.Session()


@pytest.fixture(scope="module")
def gold(golden):
    g = dict(golden("g10_umap.npz"))
    m = g["X"].shape[0]
    g["G"] = sp.csr_matrix((g["G_data"], g["G_indices"], g["G_indptr"]), shape=(m, m))
    return g


def _resident(sess, G, dt):
    """a scipy CSR as a ResidentCsr of dtype dt on the session (the caller's own arrays, adopted)"""
    G = sp.csr_matrix(G)
    return ops.ResidentCsr.from_torch(sess, _dev(G.indptr.astype(np.int64)), _dev(G.indices.astype(np.int32)), _dev(G.data.astype(dt)),
                                      G.shape)


def _host_csr(G):
    d = G.as_device_csr()
    return sp.csr_matrix((d.values.cpu().numpy(), d.col_indices.cpu().numpy(), d.row_offsets.cpu().numpy()), shape=G.shape)


# ------------------------------------------------------------------ 1. / 2. the graph
def _check_graph(sess, idx, dist_t, nn, dt, expect_floored=None):
    """umap_graph on (idx, dist_t) against the restatement; returns (host G, sigma, rho, floored)"""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    m, K = idx.shape
    G, sigma, rho = sess.umap_graph(_dev(idx), _dev(dist_t), nn)
    sigma, rho = sigma.cpu().numpy(), rho.cpu().numpy()
    want_sigma, want_rho, floored, margin = UR.smooth(idx, dist_t, nn)
    print(f"smallest decision margin of these searches {margin:.3e}; {int(floored.sum())} floored rows of {m}")
    if expect_floored is not None:
        assert floored[expect_floored].all()
    assert np.isfinite(sigma).all() and np.isfinite(rho).all() and (sigma > 0).all()
    np.testing.assert_array_equal(rho, want_rho)                                # exact
    np.testing.assert_array_equal(sigma[~floored], want_sigma[~floored])       # bit for bit where the floor does not govern
    if floored.any():
        rel = np.abs(sigma[floored] - want_sigma[floored]) / want_sigma[floored]
        bound = np.where(want_rho[floored] > 0, K * EPS, float(m) * K * EPS)
        print(f"largest floored-sigma error {rel.max() / EPS:.2f} eps_f64")
        assert (rel <= bound).all()
    got = _host_csr(G)
    want = UR.union(idx, UR.memberships(idx, dist_t, sigma, rho), dt)
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    assert got.data.dtype == np.dtype(dt)
    if want.nnz:
        ulps = np.abs(got.data.astype(np.float64) - want.data.astype(np.float64)) / np.spacing(np.abs(want.data)).astype(np.float64)
        print(f"largest value error {ulps.max():.2f} ulp")
        assert ulps.max() <= 2
        assert np.isfinite(got.data).all() and (got.data >= 0).all() and (got.data <= 1).all()
    assert G.check().canonical
    assert (got != got.T).nnz == 0                                             # G_ij == G_ji bit for bit
    G2, sigma2, rho2 = sess.umap_graph(_dev(idx), _dev(dist_t), nn)            # the same bytes from call to call
    again = _host_csr(G2)
    assert (again.indptr.tobytes(), again.indices.tobytes(), again.data.tobytes(), sigma2.cpu().numpy().tobytes(),
            rho2.cpu().numpy().tobytes()) == (got.indptr.tobytes(), got.indices.tobytes(), got.data.tobytes(), sigma.tobytes(),
                                              rho.tobytes())
    return got, sigma, rho, floored


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("which", ["fixture", "m_is_K_plus_1"])
def test_graph(sess, gold, which, dt):
    if which == "fixture":
        idx, dist, nn = gold["indices"], gold["dist"], int(gold["n_neighbors"])
    else:
        X = UR.clusters(31, 4, 11)[0]                                          # m = K + 1: every row is everyone's neighbour
        idx, dist = KR.knn(X, X, 30, "euclidean", exclude_self=True)
        nn = 31
    m, K = idx.shape
    got = _check_graph(sess, idx, dist.astype(dt), nn, dt)[0]
    listed = sp.csr_matrix((np.ones(m * K), (np.repeat(np.arange(m), K), idx.ravel())), shape=(m, m))
    mutual = listed.multiply(listed.T).nnz
    if which == "fixture":
        assert 0 < mutual < listed.nnz                                         # mutual and one-sided neighbours both occur
        if dt == np.float64:                                                   # the searches ran on the fixture's own distances
            np.testing.assert_array_equal(got.indptr, gold["G_indptr"])
            np.testing.assert_array_equal(got.indices, gold["G_indices"])
    else:
        assert mutual == listed.nnz == m * (m - 1)
    assert got.nnz == 2 * listed.nnz - mutual


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("K", [1, 63, 64, 65, 128])
def test_graph_at_the_wave_and_row_tail_boundaries(sess, K, dt):
    X = np.random.default_rng(257 + K).normal(size=(257, 5))
    idx, dist = KR.knn(X, X, K, "euclidean", exclude_self=True)
    _check_graph(sess, idx, dist.astype(dt), K + 1, dt)


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_two_rows(sess, dt):
    idx = np.array([[1], [0]], dtype=np.int32)
    dist = np.array([[0.75], [0.75]], dtype=dt)
    got, sigma, rho, _ = _check_graph(sess, idx, dist, 2, dt)
    assert (sigma == 1.0).all() and (rho == 0.75).all()                        # psum = 1 = log2(2) at the first step
    assert got.nnz == 2 and (got.data == 1).all()


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_degenerate_rows_and_unfilled_slots(sess, gold, dt):
    idx, dist, nn = gold["indices"].copy(), gold["dist"].astype(dt), int(gold["n_neighbors"])
    dist[3, :] = 0                                                             # every distance 0: rho 0, memberships 1, the panel's floor
    dist[5, :] = dist[5, 0]                                                    # all equal and positive: psum stays K, the search runs out
    idx[::7, 10:] = -1                                                         # as the search leaves a slot it could not fill
    dist[::7, 10:] = np.nan
    idx[11, :] = -1                                                            # a row with no neighbour at all
    got, sigma, rho, floored = _check_graph(sess, idx, dist, nn, dt, expect_floored=[3, 5])
    assert rho[3] == 0 and rho[5] == dist[5, 0] and rho[11] == 0
    assert (got[3].data[np.isin(got[3].indices, idx[3])] >= 1 - 2.0 ** -53).all()   # (1 + b) - b: 1 up to one rounding


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_graph_through_every_length_class_of_the_row_sort(sess, dt):
    """hand-made lists: one raw row beyond canon_lds_cap() that merges mutual pairs, one between 65 entries and the cap"""
    idx, dist = UR.hub_lists()
    m, K = idx.shape
    counts, merged = UR.sort_classes(idx)
    print(f"rows that need the sort per length class {counts}, merged entries {merged}")
    assert all(c > 0 for c in counts) and merged > 0                           # from the lists alone, before the GPU runs
    assert np.isin(idx[0], np.nonzero((idx == 0).any(axis=1))[0]).all()        # the long row lists rows that list it back
    got = _check_graph(sess, idx, dist.astype(dt), K + 1, dt)[0]
    assert got.nnz == 2 * m * K - merged and np.diff(got.indptr)[0] == m - 1


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_graph_of_a_directed_ring_merges_nothing(sess, dt):
    """K = 1, no mutual pair: every row is sorted, none merges, and the offsets stay the raw ones"""
    m = 65
    idx = ((np.arange(m) + 1) % m).astype(np.int32)[:, None]
    dist = np.random.default_rng(65).uniform(0.5, 1.5, size=(m, 1)).astype(np.float32)
    assert UR.sort_classes(idx) == ([m - 2, 0, 0], 0)                          # (rows 0 and m - 1 are ascending as emitted)
    got = _check_graph(sess, idx, dist.astype(dt), 2, dt)[0]
    assert got.nnz == 2 * m
    np.testing.assert_array_equal(got.indptr, 2 * np.arange(m + 1))


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_graph_without_a_valid_slot_is_empty(sess, dt):
    m, K = 8, 3
    got, sigma, rho, _ = _check_graph(sess, np.full((m, K), -1, dtype=np.int32), np.full((m, K), np.nan, dtype=dt), K + 1, dt)
    assert got.shape == (m, m) and got.nnz == 0 and (got.indptr == 0).all()
    assert np.isfinite(sigma).all() and np.isfinite(rho).all()


# ------------------------------------------------------------------ 3. the trajectory
@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("D,rate", [(2, 5), (1, 5), (3, 5), (2, 0), (2, 31)], ids=["D2", "D1", "D3", "rate0", "rate31"])
def test_trajectory(sess, gold, D, rate, dt):
    a, b, n_epochs, seed = float(gold["a"]), float(gold["b"]), int(gold["epochs"]), int(gold["layout_seed"])
    Gs = gold["G"].astype(dt)
    Y0 = gold["Y0"] if D == 2 else UR.init_random(200, D, seed)
    name = "f32" if dt == np.float32 else "f64"
    if (D, rate) == (2, 5):
        want = gold[f"Y20_{name}"]
        stats = UR.layout(Gs, Y0, n_epochs, a, b, rate, seed=seed, storage=dt, return_stats=True)[1]
    else:
        want, stats = UR.layout(Gs, Y0, n_epochs, a, b, rate, seed=seed, storage=dt, return_stats=True)
    assert stats["qmax"] <= 2 * rate and 0 < stats["used"].sum() < Gs.nnz      # the filter leaves entries out, and keeps some
    rev = UR.layout(Gs, Y0, n_epochs, a, b, rate, seed=seed, storage=dt, reverse=True)
    spread = float(np.abs(rev.astype(np.float64) - want.astype(np.float64)).max())
    Y = sess.umap_embed(_resident(sess, Gs, dt), n_epochs=n_epochs, output_dim=D, init=_dev(Y0.astype(dt)), negative_sample_rate=rate,
                        a=a, b=b, seed=seed)
    Y = Y.cpu().numpy()
    assert Y.dtype == np.dtype(dt) and np.isfinite(Y).all()
    err = float(np.abs(Y.astype(np.float64) - want.astype(np.float64)).max())
    print(f"{name} D={D} rate={rate}: reordered restatement differs by {spread:.3e}, the GPU by {err:.3e} (max |Y| {np.abs(want).max():.3e})")
    assert err <= 16 * spread


# ------------------------------------------------------------------ 4. the schedule's edges
@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_filtered_entries_are_never_sampled(sess, dt):
    """20 epochs: w_max / 20 = 0.05, so the pair (4, 5) at 0.01 is left out; vertices 4 and 5 have no other entry and keep
    their coordinates bit for bit (negative samples hang off sampled entries: none for them either)"""
    rows = np.array([0, 1, 2, 3, 4, 5, 0, 2])
    cols = np.array([1, 0, 3, 2, 5, 4, 2, 0])
    vals = np.array([1.0, 1.0, 0.5, 0.5, 0.01, 0.01, 0.2, 0.2])
    G = sp.csr_matrix((vals, (rows, cols)), shape=(6, 6)).astype(dt)
    G.sort_indices()
    Y0 = (UR.init_random(6, 2, 3) - 5.0).astype(dt)
    Y0[4, 0] = -0.0
    a, b = UR.find_ab(1.0, 0.1)
    want, stats = UR.layout(G, Y0, 20, a, b, 5, seed=9, storage=dt, return_stats=True)
    assert stats["sampled"][[G.indptr[4], G.indptr[5]]].tolist() == [0, 0] and stats["sampled"].sum() > 0
    rev = UR.layout(G, Y0, 20, a, b, 5, seed=9, storage=dt, reverse=True)
    Y = sess.umap_embed(_resident(sess, G, dt), n_epochs=20, init=_dev(Y0), a=a, b=b, seed=9).cpu().numpy()
    assert Y[4:].tobytes() == Y0[4:].tobytes()
    assert (Y[:4] != Y0[:4]).any()
    spread = float(np.abs(rev.astype(np.float64) - want.astype(np.float64)).max())
    err = float(np.abs(Y.astype(np.float64) - want.astype(np.float64)).max())
    print(f"reordered restatement differs by {spread:.3e}, the GPU by {err:.3e}")
    assert err <= 16 * spread


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_a_zero_learning_rate_returns_the_initial_embedding(sess, dt):
    X = UR.clusters(64, 5, 4)[0].astype(dt)
    X[:, 1] = 2.5                                                              # a constant column gives 0
    for D in (1, 2, 3):
        Y = sess.umap(_dev(X), n_neighbors=8, n_epochs=1, learning_rate=0.0, output_dim=D, init="panel").cpu().numpy()
        want = UR.init_panel(X, D).astype(dt)                                  # f64 from the stored values, rounded once
        assert Y.tobytes() == want.tobytes()
        if D >= 2:
            assert (Y[:, 1] == 0).all() and Y[:, 0].min() == 0 and abs(Y[:, 0].max() - 10) < 1e-5
        Y = sess.umap(_dev(X), n_neighbors=8, n_epochs=1, learning_rate=0.0, output_dim=D, init="random", seed=77).cpu().numpy()
        u = synth.hash_u01(77, 31, torch.arange(64 * D, dtype=torch.int64)).numpy().reshape(64, D)
        assert Y.tobytes() == (10.0 * u).astype(dt).tobytes()
    given = (UR.init_random(64, 2, 5) - 3.0).astype(dt)
    Y = sess.umap(_dev(X), n_neighbors=8, n_epochs=1, learning_rate=0.0, init=_dev(given)).cpu().numpy()
    assert Y.tobytes() == given.tobytes()


def test_m_zero_is_valid_and_writes_nothing(sess):
    Y = sess.umap(torch.zeros((0, 4), dtype=torch.float32, device="cuda"))
    assert tuple(Y.shape) == (0, 2)
    G, sigma, rho = sess.umap_graph(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), torch.zeros((0, 3), dtype=torch.float32, device="cuda"), 4)
    assert G.nnz == 0 and G.shape == (0, 0)


# ------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_end_to_end_separates_clusters_and_every_route_agrees(sess, dt):
    X, labels = UR.clusters(600, 10, 3)
    X = X.astype(dt)
    x = _dev(X)
    est = sapca.UMAP(n_epochs=200)
    Y = est.fit_transform(x)
    assert est.embedding_ is Y and Y.dtype == DT[np.dtype(dt)] and tuple(Y.shape) == (600, 2)
    y = Y.cpu().numpy()
    assert np.isfinite(y).all()
    share = UR.same_cluster_share(y, labels)
    print(f"panel init: share {share:.4f}")
    assert share >= 0.99
    first = y.tobytes()
    assert est.fit_transform(x).cpu().numpy().tobytes() == first               # the same bytes on a second run
    assert sess.umap(x, n_epochs=200).cpu().numpy().tobytes() == first         # the device route on a bare handle
    assert sess.umap(X, n_epochs=200).tobytes() == first                       # the host route
    idx, dist = sess.knn(x, n_neighbors=14)                                    # the stages by hand
    G = sess.umap_graph(idx, dist, 15)[0]
    init = _dev(UR.init_panel(X, 2).astype(dt))
    assert sess.umap_embed(G, n_epochs=200, init=init).cpu().numpy().tobytes() == first
    r1 = sess.umap(x, n_epochs=200, init="random", seed=1).cpu().numpy()
    r2 = sess.umap(x, n_epochs=200, init="random", seed=2).cpu().numpy()
    assert r1.tobytes() == sess.umap(x, n_epochs=200, init="random", seed=1).cpu().numpy().tobytes()
    assert r1.tobytes() != r2.tobytes()                                        # another seed, another embedding
    share = UR.same_cluster_share(r1, labels)
    print(f"random init: share {share:.4f}")
    assert np.isfinite(r1).all() and share >= 0.99


# ------------------------------------------------------------------ 6. refusals
def _options(**kw):
    o = L.default_umap_options()
    o.epochs = 5
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _raw_umap(sess, dt, o, m, x, ldx, d, y):
    fn = getattr(L.load(), f"sapca_umap_device_{'f32' if dt == np.float32 else 'f64'}")
    st = fn(sess._h, C.c_uint64(m), C.c_void_p(x.data_ptr() if x is not None else None), C.c_uint64(ldx), C.c_uint64(d), C.byref(o),
            C.c_void_p(y.data_ptr() if y is not None else None))
    return st, (L.load().sapca_last_error(sess._h) or b"").decode()


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_refusals_leave_the_handle_usable(dt):
    sess = ops.Session()
    tdt = DT[np.dtype(dt)]
    X = UR.clusters(40, 6, 2)[0].astype(dt)
    x = _dev(X)
    y = torch.full((40, 3), -7.0, dtype=tdt, device="cuda")
    ok = dict(m=40, x=x, ldx=6, d=6, y=y)
    st, msg = _raw_umap(sess, dt, o=_options(), **ok)
    assert st == L.OK, msg
    good = y.cpu().numpy().tobytes()
    y.fill_(-7.0)
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(), dict(struct_size=88), "options->struct_size is 88"),
        (dict(), dict(output_dim=0), "output_dim = 0 is outside 1 .. 3"),
        (dict(), dict(output_dim=4), "output_dim = 4 is outside 1 .. 3"),
        (dict(), dict(init=3), "init = 3 is not a sapca_umap_init"),
        (dict(), dict(n_neighbors=1), "n_neighbors = 1 is outside 2 .. 129"),
        (dict(), dict(n_neighbors=130), "n_neighbors = 130 is outside 2 .. 129"),
        (dict(), dict(n_neighbors=41), "n_neighbors = 41 exceeds the m = 40 rows"),
        (dict(), dict(negative_sample_rate=32), "negative_sample_rate = 32 exceeds 31"),
        (dict(), dict(learning_rate=-1.0), "learning_rate = -1 must be finite and not negative"),
        (dict(), dict(learning_rate=nan), "learning_rate = nan must be finite and not negative"),
        (dict(), dict(repulsion_strength=inf), "repulsion_strength = inf must be finite and not negative"),
        (dict(), dict(a=1.5), "a = 1.5, b = 0: give both"),
        (dict(), dict(b=0.9), "a = 0, b = 0.9: give both"),
        (dict(), dict(a=-1.0, b=1.0), "a = -1, b = 1 must be finite and not negative"),
        (dict(), dict(a=1.0, b=nan), "a = 1, b = nan must be finite and not negative"),
        (dict(), dict(spread=0.0), "spread = 0 must be finite and positive"),
        (dict(), dict(spread=nan), "spread = nan must be finite and positive"),
        (dict(), dict(min_dist=-0.1), "min_dist = -0.1 must be finite and not negative"),
        (dict(), dict(min_dist=3.0), "min_dist = 3 must be below 3 spread = 3"),
        (dict(d=2), dict(output_dim=3), "takes the first output_dim = 3 columns, the panel has d = 2"),
        (dict(m=2 ** 31), dict(), f"m = {2 ** 31} rows"),
        (dict(d=0), dict(), "d is 0"),
        (dict(d=1025, ldx=2000), dict(), "d = 1025 exceeds 1024"),
        (dict(ldx=5), dict(), "ldx = 5 is less than d = 6"),
        (dict(ldx=2 ** 28), dict(), f"a row stride of {2 ** 28} elements; 2^28 or more are not supported"),
        (dict(x=None), dict(), "a NULL panel with m = 40"),
        (dict(y=None), dict(), "a NULL panel with m = 40"),
    ]
    for change, opt, message in cases:
        st, msg = _raw_umap(sess, dt, o=_options(**opt), **{**ok, **change})
        assert st == L.ERR_ARG and message in msg, f"{change} {opt}: status {st}, message {msg!r}"
        assert (y == -7).all(), f"{change} {opt}: the output was written"
        st, msg = _raw_umap(sess, dt, o=_options(), **ok)                       # the same handle, straight after
        assert st == L.OK, msg
        assert y.cpu().numpy().tobytes() == good
        y.fill_(-7.0)
    # a given curve needs no fit: (spread, min_dist) are not looked at
    st, msg = _raw_umap(sess, dt, o=_options(a=1.5, b=0.9, spread=0.0), **ok)
    assert st == L.OK, msg
    # 0 is a valid rate and strength
    st, msg = _raw_umap(sess, dt, o=_options(learning_rate=0.0, repulsion_strength=0.0), **ok)
    assert st == L.OK, msg
    y.fill_(-7.0)
    # the stage calls refuse the same way
    with pytest.raises(L.SapcaError, match="K = 129 neighbours per row is outside 1 .. 128"):
        sess.umap_graph(torch.zeros((200, 129), dtype=torch.int32, device="cuda"), torch.zeros((200, 129), dtype=tdt, device="cuda"), 15)
    with pytest.raises(L.SapcaError, match="n_neighbors = 1 must be at least 2"):
        sess.umap_graph(torch.zeros((20, 4), dtype=torch.int32, device="cuda"), torch.zeros((20, 4), dtype=tdt, device="cuda"), 1)
    idx, dist = sess.knn(x, n_neighbors=9)
    G = sess.umap_graph(idx, dist, 10)[0]
    with pytest.raises(L.SapcaError, match="SAPCA_UMAP_INIT_PANEL"):
        sess.umap_embed(G, n_epochs=5, init="panel")
    with pytest.raises(L.SapcaError, match="output_dim = 4 is outside 1 .. 3"):
        sess.umap_embed(G, n_epochs=5, output_dim=4)
    fn = getattr(L.load(), f"sapca_umap_embed_device_{'f32' if dt == np.float32 else 'f64'}")
    o = _options(init=L.UMAP_INIT_RANDOM)
    st = fn(sess._h, C.c_uint64(40), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx), C.c_void_p(G.d_val), C.byref(o), None)
    assert st == L.ERR_ARG and "d_y is NULL with m = 40" in (L.load().sapca_last_error(sess._h) or b"").decode()
    st = fn(sess._h, C.c_uint64(40), C.c_uint64(G.nnz), None, C.c_void_p(G.d_idx), C.c_void_p(G.d_val), C.byref(o), C.c_void_p(y.data_ptr()))
    assert st == L.ERR_ARG and "null CSR array" in (L.load().sapca_last_error(sess._h) or b"").decode()
    assert (y == -7).all()
    st, msg = _raw_umap(sess, dt, o=_options(), **ok)
    assert st == L.OK and y.cpu().numpy().tobytes() == good


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
    Y = est.session().umap(scores, n_neighbors=10, n_epochs=25, seed=42)
    Yw = sess.umap(scores.clone(), n_neighbors=10, n_epochs=25, seed=42)        # the same rows on a bare handle
    assert Y.cpu().numpy().tobytes() == Yw.cpu().numpy().tobytes() and np.isfinite(Y.cpu().numpy()).all()
    Yc = est.session().umap(scores[:, :4], n_neighbors=10, n_epochs=5)         # a column slice, searched in place
    assert np.isfinite(Yc.cpu().numpy()).all()
    assert Yc.cpu().numpy().tobytes() == sess.umap(scores[:, :4].contiguous(), n_neighbors=10, n_epochs=5).cpu().numpy().tobytes()
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
    X = _dev(UR.clusters(200, 7, 9)[0].astype(np.float32))
    Y = est.session().umap(X, n_neighbors=8, n_epochs=20, seed=42)
    Yw = sess.umap(X, n_neighbors=8, n_epochs=20, seed=42)
    assert Y.cpu().numpy().tobytes() == Yw.cpu().numpy().tobytes()
    assert not calls

"""Louvain clustering of a device-resident graph (-m gpu): sapca_louvain_* through Session.modularity / louvain_sweep /
louvain_aggregate / louvain and sapca.Louvain.

The reference is tests/louvain_ref.py (numpy; tests/test_louvain_cpu.py holds it to networkx and its fixture fixed).  It does
not restate the order of any sum, so results are compared exactly only where that order cannot matter: on graphs whose weights
are k / 8 (every sum is exact), and on whole runs whose every decision clears its threshold by more than 1e-9 (the margins of
the CPU test), which a reordering of at most a few thousand f64 additions of values below 1 cannot cross."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import louvain_ref as LR
import sapca
from sapca import _lib as L
from sapca import ops

pytestmark = pytest.mark.gpu

IDS = dict(ids=["f32", "f64"])
DTYPES = [np.float32, np.float64]
EPS = np.finfo(np.float64).eps
SEED = 42
# the comb's hubs: the issue's degrees, which already straddle the two path thresholds of the rows kernel (64 and 4096)
HUBS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 20000]
DYADIC = ["ring64", "ring1024", "grid30", "planted_g05", "planted_g1", "planted_g2", "matching64", "k16", "star5000", "two_cliques"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def sess():
    return ops.Session()


@pytest.fixture(scope="module")
def gold(golden):
    return dict(golden("g11_louvain.npz"))


@pytest.fixture(scope="module")
def comb():
    return LR.comb(HUBS)


def _graph(gold, name):
    m = len(gold[f"{name}_indptr"]) - 1
    return sp.csr_matrix((gold[f"{name}_data"], gold[f"{name}_indices"], gold[f"{name}_indptr"]), shape=(m, m))


def _resident(sess, G, dt):
    G = sp.csr_matrix(G)
    return ops.ResidentCsr.from_torch(sess, _dev(G.indptr.astype(np.int64)), _dev(G.indices.astype(np.int32)), _dev(G.data.astype(dt)),
                                      G.shape)


def _host_csr(G):
    d = G.as_device_csr()
    return sp.csr_matrix((d.values.cpu().numpy(), d.col_indices.cpu().numpy(), d.row_offsets.cpu().numpy()), shape=G.shape)


def _comb_start(comb, kind):
    n = comb.shape[0]
    c = np.arange(n, dtype=np.int32)
    if kind == "three":
        nh = len(HUBS)
        c[nh:] = nh + (np.arange(n - nh) % 3)
    return c


# ------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("gamma", [1.0, 2.0])
@pytest.mark.parametrize("t", [0, 5])
@pytest.mark.parametrize("start", ["singletons", "three"])
def test_sweep_is_exact_on_the_comb(sess, comb, start, t, gamma):
    """every weight is k / 8, so w, k, tot and S are exact in any order: labels and n_moved equal the restatement's, in both
    dtypes; the hubs' rows cover all three paths of the rows kernel and both sides of their thresholds"""
    assert {64, 65, 4096, 4097} <= set(HUBS) and L.load() is not None
    c = _comb_start(comb, start)
    want, moved, _ = LR.sweep(comb, c, SEED, 0, t, gamma)
    assert moved > 0
    for dt in DTYPES:
        out, n_moved = sess.louvain_sweep(_resident(sess, comb, dt), c, seed=SEED, level=0, sweep=t, resolution=gamma)
        got = out.cpu().numpy()
        assert n_moved == moved, (dt, n_moved, moved)
        assert np.array_equal(got, want), (dt, np.flatnonzero(got != want)[:10])


def _sweep_bound_check(G, c, got, t, gamma):
    """every vertex's choice has a gain within 2 (n_i + 3) eps (k_i + r_i max tot) of the best, gains in longdouble"""
    R = LR.gains(G, c, SEED, 0, t, gamma, dtype=np.longdouble)
    n = G.shape[0]
    best = R["g_c"].copy()
    cand = sp.csr_matrix((np.ones(len(R["rows"])), (R["rows"], R["D"])), shape=(n, n))
    gain_of = {(int(r), int(d)): g for r, d, g in zip(R["rows"], R["D"], R["g"])}
    np.maximum.at(best, R["rows"], R["g"])
    n_i = np.diff(G.indptr)
    bound = 2 * (n_i + 3) * EPS * (R["k"] + R["r"] * R["tot"].max())
    worst = 0.0
    for i in range(n):
        if got[i] == c[i]:
            g = R["g_c"][i]
        else:
            assert R["active"][i] and cand[i, got[i]] == 1, (i, got[i])
            g = gain_of[(i, int(got[i]))]
        assert best[i] - g <= bound[i], (i, float(best[i] - g), float(bound[i]))
        worst = max(worst, float((best[i] - g) / bound[i]))
    return worst


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_sweep_on_general_weights_takes_a_best_gain(sess, gold, dt):
    G = LR.as_csr(_graph(gold, "G").astype(dt).astype(np.float64))
    starts = [np.arange(G.shape[0], dtype=np.int32)]
    c = starts[0].astype(np.int64)
    for t in range(3):
        c = LR.sweep(G, c, SEED, 0, t, 1.0)[0]
    starts.append(c.astype(np.int32))
    for c in starts:
        for t in (3, 4):
            out, n_moved = sess.louvain_sweep(_resident(sess, G, dt), c, seed=SEED, level=0, sweep=t, resolution=1.0)
            got = out.cpu().numpy()
            want, moved, _ = LR.sweep(G, c, SEED, 0, t, 1.0)
            worst = _sweep_bound_check(G, c, got, t, 1.0)
            print(f"sweep {t}: {int((got != want).sum())} choices differ from the restatement's, {n_moved} moved (restatement {moved}), "
                  f"worst gap / bound {worst:.3f}")
            assert n_moved == int((got != c).sum())


# ------------------------------------------------------------------ modularity
@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_modularity_against_longdouble(sess, gold, golden, dt):
    """Order of the implementation's sums: k_i and s_i by 64 strided lanes and a 6-step butterfly (at most ceil(n_i / 64) + 6
    roundings each), S, sum s_i and sum (tot_C / S)^2 by 256 strided threads, an 8-step tree and the same again over the
    blocks (at most 18 roundings here, m <= 256), tot_C left to right over its members (at most m - 1).  With u = eps / 2 the
    first-order bound on Q is ((7 + 18 + 26) + gamma (2 (m + 25) + 18)) u, about (m + 60) eps at gamma = 1; the one-community
    assignment is the case that reaches for it.  The issue caps the bound at m eps_f64, which is what is asserted."""
    G = LR.as_csr(_graph(gold, "G").astype(dt).astype(np.float64))
    m = G.shape[0]
    R = _resident(sess, G, dt)
    km = dict(golden("g10_umap.npz"))["labels"].astype(np.int32)
    for name, c in (("clusters", km), ("singletons", np.arange(m, dtype=np.int32)), ("one", np.zeros(m, dtype=np.int32))):
        for gamma in (0.5, 1.0, 2.0):
            got = sess.modularity(R, c, resolution=gamma)
            want = LR.modularity(G, c, gamma, dtype=np.longdouble)
            print(f"{name} gamma {gamma}: Q {got:.15f}, off by {abs(got - float(want)) / EPS:.2f} eps (bound {m} eps)")
            assert abs(np.longdouble(got) - want) <= m * EPS


# ------------------------------------------------------------------ aggregation
def _check_aggregate(sess, G, c, dt, exact):
    R = _resident(sess, G, dt)
    coarse, ren = sess.louvain_aggregate(R, c)
    want, want_ren = LR.aggregate(G, c)
    got = _host_csr(coarse)
    assert coarse.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(ren.cpu().numpy(), want_ren)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert coarse.check().canonical
    # entries merged into a coarse entry: at most the entries of the fine graph between the two communities
    ok = (np.asarray(c) >= 0) & (np.asarray(c) < G.shape[0])
    P = sp.csr_matrix((np.ones(int(ok.sum())), (np.flatnonzero(ok), want_ren[ok])), shape=(G.shape[0], want.shape[0]))
    ones = sp.csr_matrix((np.ones_like(G.data), G.indices, G.indptr), shape=G.shape)
    merged = (P.T @ ones @ P).tocsr()
    merged.sort_indices()
    if exact:
        assert np.array_equal(got.data, want.data)
        assert (got != got.T).nnz == 0
    else:
        assert np.all(np.abs(got.data - want.data) <= merged.data * EPS * np.abs(want.data))
        T = got.T.tocsr()
        T.sort_indices()
        assert np.array_equal(T.indices, got.indices) and np.all(np.abs(T.data - got.data) <= merged.data * EPS * np.abs(want.data))
    return got, want_ren


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_aggregate_on_the_comb_is_exact(sess, comb, dt):
    c = _comb_start(comb, "three")
    got, ren = _check_aggregate(sess, comb, c, dt, exact=True)
    assert np.all(np.diff(ren[np.argsort(c, kind="stable")]) >= 0)           # the renumbering ascends with the label
    c1 = LR.sweep(comb, c, SEED, 0, 0, 1.0)[0]                               # hubs and leaves mixed: long coarse rows
    _check_aggregate(sess, comb, c1.astype(np.int32), dt, exact=True)


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_aggregate_on_general_weights(sess, gold, dt):
    G = LR.as_csr(_graph(gold, "G").astype(dt).astype(np.float64))
    c = gold["G_level_labels"][0]
    assert len(np.unique(c)) > 3
    # (level labels are renumbered already: spread them over [0, m) again so that the renumbering has work to do)
    c = np.sort(np.random.default_rng(0).choice(G.shape[0], len(np.unique(c)), replace=False))[c].astype(np.int32)
    got, ren = _check_aggregate(sess, G, c, dt, exact=False)
    assert np.all(got.diagonal() > 0)                                        # every community of a kept level has inner weight


# ------------------------------------------------------------------ the whole run
def _run(sess, G, dt, **kw):
    labels, n, q, levels = sess.louvain(_resident(sess, G, dt), seed=SEED, **kw)
    return labels.cpu().numpy(), n, q, levels


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("name", DYADIC)
def test_run_equals_the_golden_on_dyadic_graphs(sess, gold, name, dt):
    G = _graph(gold, name)
    gamma = float(gold[f"{name}_gamma"])
    labels, n, q, levels = _run(sess, G, dt, resolution=gamma)
    assert (n, levels) == (int(gold[f"{name}_n_communities"]), int(gold[f"{name}_n_levels"]))
    assert np.array_equal(labels, gold[f"{name}_labels"])
    q0 = sess.modularity(_resident(sess, G, dt), labels, resolution=gamma)
    print(f"{name}: Q {q:.15f}, at level 0 {q0:.15f}, golden {float(gold[f'{name}_Q']):.15f}")
    assert abs(q - q0) <= G.shape[0] * EPS and abs(q - float(gold[f"{name}_Q"])) <= G.shape[0] * EPS


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_run_on_general_weights(sess, gold, dt):
    """the margins of the run on G (tests/test_louvain_cpu.py) license the exact comparison; the f32 graph is another graph,
    so the restatement runs on its values"""
    G = LR.as_csr(_graph(gold, "G").astype(dt).astype(np.float64))
    want = LR.run(G, seed=SEED)
    assert min(want["margin_gain"], want["margin_q"]) > 1e-9
    labels, n, q, levels = _run(sess, G, dt)
    assert (n, levels) == (want["n_communities"], want["n_levels"]) and np.array_equal(labels, want["labels"])
    if dt == np.float64:
        assert np.array_equal(labels, gold["G_labels"]) and levels == int(gold["G_n_levels"])
    assert abs(q - sess.modularity(_resident(sess, G, dt), labels)) <= G.shape[0] * EPS
    assert abs(q - want["Q"]) <= G.shape[0] * EPS


@pytest.mark.parametrize("kw", [dict(max_levels=1), dict(max_sweeps=1), dict(max_sweeps=3, max_levels=2)], ids=["levels1", "sweeps1", "3x2"])
def test_caps_stop_where_the_restatement_stops(sess, gold, kw):
    G = _graph(gold, "grid30")
    want = LR.run(G, seed=SEED, **kw)
    labels, n, q, levels = _run(sess, G, np.float64, **kw)
    assert (n, levels) == (want["n_communities"], want["n_levels"]) and np.array_equal(labels, want["labels"])
    assert abs(q - want["Q"]) <= G.shape[0] * EPS


def test_repeatable(sess, gold):
    G = _graph(gold, "G")
    a = _run(sess, G, np.float32)
    b = _run(sess, G, np.float32)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]


# ------------------------------------------------------------------ edges
def test_edge_shapes(sess, gold):
    for dt in DTYPES:
        empty = sp.csr_matrix((0, 0), dtype=dt)
        labels, n, q, levels = _run(sess, empty, dt)
        assert labels.shape == (0,) and (n, q, levels) == (0, 0.0, 0)
        assert sess.modularity(_resident(sess, empty, dt), np.zeros(0, dtype=np.int32)) == 0.0
        labels, n, q, levels = _run(sess, sp.csr_matrix((1, 1), dtype=dt), dt)
        assert labels.tolist() == [0] and (n, q, levels) == (1, 0.0, 0)
        labels, n, q, levels = _run(sess, sp.csr_matrix((100, 100), dtype=dt), dt)
        assert np.array_equal(labels, np.arange(100)) and (n, q, levels) == (100, 0.0, 0)
        # isolated vertices beside a ring, and a stored diagonal at level 0
        ring = sp.block_diag([LR.ring(64), sp.csr_matrix((10, 10))]).tocsr()
        diag = (LR.two_cliques(8) + sp.diags(np.arange(16) % 3 / 4.0)).tocsr()
        diag.eliminate_zeros()
        for G in (ring, diag):
            want = LR.run(G, seed=SEED)
            labels, n, q, levels = _run(sess, G, dt)
            assert (n, levels) == (want["n_communities"], want["n_levels"]) and np.array_equal(labels, want["labels"])
            assert abs(q - want["Q"]) <= G.shape[0] * EPS


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_bad_labels_and_columns_touch_nothing_outside(sess, gold, dt):
    """a label or a column out of range is skipped where it is read; guard words around the outputs stay"""
    G = LR.as_csr(_graph(gold, "planted_g1"))
    m = G.shape[0]
    suf = "f32" if dt == np.float32 else "f64"
    lib = L.load()
    c = np.arange(m, dtype=np.int32)
    bad = np.array([3, 77, 300, 599])
    c[bad] = [-1, m, 2 ** 31 - 1, -2 ** 31]
    idx = G.indices.astype(np.int32).copy()
    idx[[5, 1000, len(idx) - 1]] = [-7, m, 2 ** 31 - 1]
    for indices in (G.indices.astype(np.int32), idx):
        R = ops.ResidentCsr.from_torch(sess, _dev(G.indptr.astype(np.int64)), _dev(indices), _dev(G.data.astype(dt)), G.shape)
        GUARD, PAD = 0x5A5A5A5A, 64
        buf = torch.full((m + 2 * PAD,), GUARD, dtype=torch.int32, device="cuda")
        d_c = _dev(c)
        moved = C.c_uint64()
        torch.cuda.synchronize()
        L.check(sess._h, getattr(lib, f"sapca_louvain_sweep_device_{suf}")(
            sess._h, C.c_uint64(m), C.c_uint64(R.nnz), C.c_void_p(R.d_ptr), C.c_void_p(R.d_idx), C.c_void_p(R.d_val),
            C.c_void_p(d_c.data_ptr()), C.c_uint32(SEED), C.c_uint32(0), C.c_uint32(1), C.c_double(1.0),
            C.c_void_p(buf.data_ptr() + 4 * PAD), C.byref(moved)))
        out = buf.cpu().numpy()
        assert np.all(out[:PAD] == GUARD) and np.all(out[-PAD:] == GUARD)
        got = out[PAD:-PAD]
        assert np.array_equal(got[bad], c[bad])                               # copied through
        rest = np.delete(got, bad)
        assert rest.min() >= 0 and rest.max() < m
        if indices is not idx:
            want, want_moved, _ = LR.sweep(G, c, SEED, 0, 1, 1.0)
            assert np.array_equal(got, want) and moved.value == want_moved
        buf.fill_(GUARD)
        n_out, nnz = C.c_uint64(), C.c_uint64()
        dp, di, dv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(sess._h, getattr(lib, f"sapca_louvain_aggregate_device_{suf}")(
            sess._h, C.c_uint64(m), C.c_uint64(R.nnz), C.c_void_p(R.d_ptr), C.c_void_p(R.d_idx), C.c_void_p(R.d_val),
            C.c_void_p(d_c.data_ptr()), C.byref(n_out), C.byref(nnz), C.byref(dp), C.byref(di), C.byref(dv),
            C.c_void_p(buf.data_ptr() + 4 * PAD)))
        out = buf.cpu().numpy()
        assert np.all(out[:PAD] == GUARD) and np.all(out[-PAD:] == GUARD)
        assert n_out.value == m - len(bad) and np.array_equal(out[PAD:-PAD][bad], c[bad])
        coarse = ops.ResidentCsr(sess, (n_out.value, n_out.value), nnz.value, np.float64, dp.value, di.value, dv.value)
        assert coarse.check().canonical
        q = sess.modularity(R, c)
        assert np.isfinite(q)
        if indices is not idx:
            assert abs(q - float(LR.modularity(G, c, 1.0, dtype=np.longdouble))) <= m * EPS


# ------------------------------------------------------------------ neighbours, end to end
@pytest.fixture(scope="module")
def panel():
    from tsne_ref import clusters
    X, _ = clusters(600, 8, 4)
    return X


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_neighbours_are_undisturbed_and_end_to_end(sess, panel, dt):
    X = _dev(panel.astype(dt))
    # an earlier canonicalize result and k-means outputs
    raw = sp.csr_matrix((np.array([1.0, 2.0, 3.0, 4.0], dtype=dt), np.array([2, 0, 0, 1], dtype=np.int32), np.array([0, 3, 4, 4])), shape=(3, 3))
    canon, _ = _resident(sess, raw, dt).canonicalize()
    canon_before = _host_csr(canon)
    km_labels, km_cen, inertia, _ = sess.kmeans(X, n_clusters=4, seed=SEED)
    km_before = (km_labels.cpu().numpy().copy(), km_cen.cpu().numpy().copy())
    idx, dist = sess.knn(X, n_neighbors=14, metric="euclidean", exclude_self=True)
    G = sess.umap_graph(idx, dist, 15)[0]
    before = _host_csr(G)
    labels, n, q, levels = sess.louvain(G, seed=SEED)
    after = _host_csr(G)
    assert before.indptr.tobytes() == after.indptr.tobytes() and before.indices.tobytes() == after.indices.tobytes()
    assert before.data.tobytes() == after.data.tobytes()
    c2 = _host_csr(canon)
    assert canon_before.indptr.tobytes() == c2.indptr.tobytes() and canon_before.indices.tobytes() == c2.indices.tobytes()
    assert canon_before.data.tobytes() == c2.data.tobytes()
    assert km_before[0].tobytes() == km_labels.cpu().numpy().tobytes() and km_before[1].tobytes() == km_cen.cpu().numpy().tobytes()
    assert 2 <= n <= 60 and levels >= 1 and 0.3 < q < 1.0
    got = labels.cpu().numpy()
    assert got.min() == 0 and got.max() == n - 1
    # the modularity entry point scores other labels on the same graph: k-means' cannot beat what Louvain kept by much
    assert abs(sess.modularity(G, labels) - q) <= X.shape[0] * EPS
    assert np.isfinite(sess.modularity(G, km_labels))
    # Session.louvain(X) is knn -> umap_graph -> louvain; the estimator is Session.louvain
    l2, n2, q2, lv2 = sess.louvain(X, seed=SEED, n_neighbors=15)
    assert l2.cpu().numpy().tobytes() == got.tobytes() and (n2, q2, lv2) == (n, q, levels)
    est = sapca.Louvain(seed=SEED)
    l3 = est.fit_predict(X)
    assert l3.cpu().numpy().tobytes() == got.tobytes()
    assert (est.n_communities_, est.modularity_, est.n_levels_) == (n, q, levels) and est.labels_ is l3
    # the host route
    h = _host_csr(G)
    l4, n4, q4, lv4 = sess.louvain_host(h.indptr, h.indices, h.data, seed=SEED)
    assert l4.tobytes() == got.tobytes() and (n4, q4, lv4) == (n, q, levels)


def test_refusals_name_their_number_and_leave_the_handle_usable(sess, gold):
    G = _graph(gold, "ring64")
    R = _resident(sess, G, np.float64)
    m = G.shape[0]
    lib = L.load()
    labels = torch.empty((m,), dtype=torch.int32, device="cuda")

    def call(o, m_=m, ptr=R.d_ptr, lab=None):
        n, q, lv = C.c_uint64(), C.c_double(), C.c_uint32()
        st = lib.sapca_louvain_device_f64(sess._h, C.c_uint64(m_), C.c_uint64(R.nnz), C.c_void_p(ptr), C.c_void_p(R.d_idx), C.c_void_p(R.d_val),
                                          C.byref(o), C.c_void_p(labels.data_ptr() if lab is None else lab), C.byref(n), C.byref(q), C.byref(lv))
        return st, lib.sapca_last_error(sess._h).decode()

    def opts(**kw):
        o = L.default_louvain_options()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    cases = [(opts(struct_size=24), {}, "24"), (opts(resolution=-0.5), {}, "-0.5"), (opts(resolution=float("inf")), {}, "inf"),
             (opts(tol=-1e-3), {}, "-0.001"), (opts(tol=float("nan")), {}, "nan"), (opts(max_sweeps=0), {}, "max_sweeps = 0"),
             (opts(max_sweeps=5000), {}, "5000"), (opts(max_levels=65), {}, "65"), (opts(), dict(m_=2 ** 31), str(2 ** 31)),
             (opts(), dict(ptr=None), f"m = {m}"), (opts(), dict(lab=0), f"m = {m}")]
    for o, kw, needle in cases:
        st, msg = call(o, **kw)
        assert st == 1 and needle in msg, (needle, st, msg)
        got, n, q, levels = sess.louvain(R, seed=SEED)                      # the handle is usable
        assert np.array_equal(got.cpu().numpy(), gold["ring64_labels"])
    moved = C.c_uint64()
    st = lib.sapca_louvain_sweep_device_f64(sess._h, C.c_uint64(m), C.c_uint64(R.nnz), C.c_void_p(R.d_ptr), C.c_void_p(R.d_idx),
                                            C.c_void_p(R.d_val), C.c_void_p(labels.data_ptr()), C.c_uint32(1), C.c_uint32(0), C.c_uint32(4096),
                                            C.c_double(1.0), C.c_void_p(labels.data_ptr()), C.byref(moved))
    assert st == 1 and "4096" in lib.sapca_last_error(sess._h).decode()
    with pytest.raises(ValueError, match="max_sweeps = 0"):
        sess.louvain(R, max_sweeps=0)
    with pytest.raises(ValueError, match="resolution"):
        sess.modularity(R, np.zeros(m, dtype=np.int32), resolution=-1.0)

"""Spectral embedding and diffusion maps of a device-resident graph (-m gpu): sapca_graph_components_device, sapca_spectral_*
and sapca_umap_spectral_init_device_* through ops.Session.

The reference is tests/spectral_ref.py (numpy; tests/test_spectral_cpu.py holds it to scipy and scikit-learn).  Bounds:
  scale   the row sum d_i differs from an exact one by at most len_i eps sum|w| (len_i additions of positive numbers), so
          NORMALIZED s_i = 1 / sqrt(d_i) by (len_i / 2 + 3) eps relative (half of d's error, the square root, the division and one
          to spare); DIFFMAP s_i = 1 / (q_i sqrt(z_i)), z_i = (sum_j w_ij / q_j) / q_i, by (L_i + 2 len_i + 6) eps relative, L_i the
          longest row among i's own neighbours (each q_j carries len_j eps, the quotient one, the sum len_i, the division by q_i len_i + 1; the square root
          halves that; q_i, the product, the square root and the division add len_i + 3)
  apply   |y_i - ref| <= (len_i + 4) eps sum_j |S_ij x_j| with S_ij = w_ij (s_i s_j) from the s the library returned
  solve   r_i = |S v_i - theta_i v_i| <= tol + 64 n_steps eps, |theta_i - lambda_i| <= r_i and |v_i - v_ref,i| <= 4 r_i / gap_i,
          with r_i from the f64 variant's vectors in longdouble and the reference pairs refined in longdouble
          (spectral_ref.refined_pairs: their error is far below eps); the f32 variant adds 2^-23 to the vector bound."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph
import torch

import sapca
import spectral_ref as SR
from sapca import _lib as L
from sapca import ops

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DTYPES = [np.float32, np.float64]
IDS = dict(ids=["f32", "f64"])
KINDS = (SR.NORMALIZED, SR.DIFFMAP)
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 1000]
GROUPS = (8, 16, 32, 64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _resident(sess, G, dt):
    G = sp.csr_matrix(G)
    return ops.ResidentCsr.from_torch(sess, _dev(G.indptr.astype(np.int64)), _dev(G.indices.astype(np.int32)), _dev(G.data.astype(dt)),
                                      G.shape)


@pytest.fixture(scope="module")
def sess():
    return ops.Session()


@pytest.fixture(scope="module")
def gold(golden):
    return dict(golden("g14_spectral.npz"))


def _graph(gold, name):
    m = len(gold[f"{name}_indptr"]) - 1
    return sp.csr_matrix((gold[f"{name}_data"].astype(np.float64), gold[f"{name}_indices"], gold[f"{name}_indptr"]), shape=(m, m))


_REF = {}


def _ref(gold, name, kind):
    """the restatement's 16 pairs (their gaps come from eigh's whole spectrum) and their longdouble refinement, once per fixture
    and kind"""
    if (name, kind) not in _REF:
        G = _graph(gold, name)
        r = SR.eigenpairs(G.indptr, G.indices, G.data, kind, 16)
        r["fine"] = SR.refined_pairs(r)
        r["S_ld"] = r["S"].astype(np.longdouble)
        _REF[name, kind] = r
    return _REF[name, kind]


# ------------------------------------------------------------------ components
def _components_equal_scipy(sess, A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    labels, n = sess.graph_components(_resident(sess, A, np.float32))
    n_want, want = csgraph.connected_components(A, directed=False) if A.shape[0] else (0, np.zeros(0, dtype=np.int32))
    assert n == n_want
    assert np.array_equal(labels.cpu().numpy(), want)


def _sym(rows, cols, m):
    A = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(m, m))
    return sp.csr_matrix(A + A.T)


def test_components_of_tiny_graphs(sess):
    _components_equal_scipy(sess, sp.csr_matrix((0, 0)))
    _components_equal_scipy(sess, sp.csr_matrix((1, 1)))
    _components_equal_scipy(sess, sp.csr_matrix((2, 2)))
    _components_equal_scipy(sess, _sym([0], [1], 2))
    _components_equal_scipy(sess, sp.csr_matrix(np.eye(2)))   # (self loops join nothing)


def test_components_of_a_randomly_numbered_path(sess):
    perm = np.random.default_rng(1).permutation(5000)
    _components_equal_scipy(sess, _sym(perm[:-1], perm[1:], 5000))


def test_components_of_a_star_and_of_cliques_with_isolated_vertices(sess):
    m = 3000
    _components_equal_scipy(sess, _sym(np.full(m - 1, 1234), np.delete(np.arange(m), 1234), m))
    rng = np.random.default_rng(2)
    ids = rng.permutation(40)
    a, b = ids[:13], ids[13:30]                    # two cliques, 10 vertices left alone
    rows = np.concatenate([np.repeat(a, len(a)), np.repeat(b, len(b))])
    cols = np.concatenate([np.tile(a, len(a)), np.tile(b, len(b))])
    keep = rows != cols
    _components_equal_scipy(sess, _sym(rows[keep], cols[keep], 40))


def test_components_of_a_random_forest(sess):
    m = 70000
    rng = np.random.default_rng(3)
    child = np.arange(1, m)
    parent = (rng.random(m - 1) * child).astype(np.int64)      # a random recursive tree ...
    keep = rng.random(m - 1) < 0.97                             # ... cut into some two thousand trees
    perm = rng.permutation(m)
    _components_equal_scipy(sess, _sym(perm[child[keep]], perm[parent[keep]], m))


def test_components_of_the_golden_graphs(sess, gold):
    for name in ("conn", "disc"):
        G = _graph(gold, name)
        labels, n = sess.graph_components(_resident(sess, G, np.float64))
        assert n == int(gold[f"{name}_n_components"]) and np.array_equal(labels.cpu().numpy(), gold[f"{name}_labels"])


# ------------------------------------------------------------------ scale and apply
def mixed_graph(m, seed=7):
    """A symmetric graph whose first rows have the lengths of LENGTHS that fit (a special row holds only columns behind the
    special rows, so its length is exact); the other rows get what symmetry hands them.  Weights in (0.5, 1.5), float32-exact."""
    rng = np.random.default_rng(seed)
    targets = [t for t in LENGTHS if t <= m - len(LENGTHS)] if m > len(LENGTHS) else []
    ns = len(targets)
    rows, cols = [], []
    for v, t in enumerate(targets):
        pick = ns + (np.arange(t) * 7 + 3 * v) % (m - ns) if t < (m - ns) else ns + np.arange(m - ns)
        pick = np.unique(pick)
        extra = ns
        while len(pick) < t:                         # (collisions of the stride: fill with the lowest free columns)
            if extra not in pick:
                pick = np.append(pick, extra)
            extra += 1
        rows += [v] * t
        cols += list(np.sort(pick)[:t])
    # a few edges among the other rows so that they are not all alike
    others = np.arange(ns, m)
    if len(others) > 2:
        a = rng.choice(others, size=2 * len(others))
        b = rng.choice(others, size=2 * len(others))
        keep = a != b
        rows += list(a[keep])
        cols += list(b[keep])
    A = sp.csr_matrix((np.ones(len(rows)), (np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64))), shape=(m, m))
    A = sp.csr_matrix(((A + A.T) > 0).astype(np.float64))
    U = sp.triu(A, k=1).tocoo()
    w = (0.5 + rng.random(U.nnz)).astype(np.float32).astype(np.float64)
    Wt = sp.csr_matrix((w, (U.row, U.col)), shape=(m, m))
    A = sp.csr_matrix(Wt + Wt.T)
    A.sort_indices()
    return A, targets


def _rowsum_ld(terms, ptr):
    """per-row sums of longdouble terms (error 2^-64 relative: exact for these bounds)"""
    out = np.zeros(len(ptr) - 1, dtype=np.longdouble)
    for i in range(len(ptr) - 1):
        if ptr[i + 1] > ptr[i]:
            out[i] = terms[ptr[i]:ptr[i + 1]].sum(dtype=np.longdouble)
    return out


def _scale_reference(A, kind):
    ptr, idx, w = A.indptr, A.indices, A.data.astype(np.longdouble)
    q = _rowsum_ld(w, ptr)
    ok = q > 0
    s = np.zeros(len(q), dtype=np.longdouble)
    if kind == SR.NORMALIZED:
        s[ok] = 1 / np.sqrt(q[ok])
    else:
        t = _rowsum_ld(w / q[idx], ptr)
        z = np.zeros_like(q)
        z[ok] = t[ok] / q[ok]
        s[ok] = 1 / (q[ok] * np.sqrt(z[ok]))
    return s


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 4099])
def test_scale_and_apply_under_every_packing(debug_switches, monkeypatch, m, dt):
    A, targets = mixed_graph(m)
    lens = np.diff(A.indptr)
    if m == 4099:
        assert targets == LENGTHS and list(lens[:len(LENGTHS)]) == LENGTHS
    elif m > len(LENGTHS):
        assert list(lens[:len(targets)]) == targets and len(targets) >= 7
    rows = np.repeat(np.arange(m), lens)
    Lnb = np.zeros(m)      # the longest row among a row's own neighbours
    for i in np.flatnonzero(lens):
        Lnb[i] = lens[A.indices[A.indptr[i]:A.indptr[i + 1]]].max()
    x = np.random.default_rng(11).normal(size=m)
    for kind in KINDS:
        want_s = _scale_reference(A, kind)
        rel = (lens / 2 + 3) * EPS if kind == SR.NORMALIZED else (Lnb + 2 * lens + 6) * EPS
        seen = {}
        for group in GROUPS + (None,):
            if group is None:
                monkeypatch.delenv("SAPCA_SPECTRAL_GROUP", raising=False)
            else:
                monkeypatch.setenv("SAPCA_SPECTRAL_GROUP", str(group))
            s = ops.Session()
            G = _resident(s, A, dt)
            sc_t = s.spectral_scale(G, kind)
            sc = sc_t.cpu().numpy()
            err = np.abs(sc.astype(np.longdouble) - want_s)
            assert np.all(err <= rel * want_s), (kind, group, float(np.max(err / np.maximum(rel * want_s, 1e-300))))
            assert np.all(sc[lens == 0] == 0.0) and np.all(sc[lens > 0] > 0.0)
            y_t = s.spectral_apply(G, _dev(x), kind)
            y = y_t.cpu().numpy()
            terms = A.data.astype(np.longdouble) * (sc[rows] * sc[A.indices]).astype(np.longdouble) * x[A.indices].astype(np.longdouble)
            want_y = _rowsum_ld(terms, A.indptr)
            mag = _rowsum_ld(np.abs(terms), A.indptr)
            erry = np.abs(y.astype(np.longdouble) - want_y)
            assert np.all(erry <= (lens + 4) * EPS * mag), (kind, group, float(np.max(erry / np.maximum((lens + 4) * EPS * mag, 1e-300))))
            assert np.all(y[lens == 0] == 0.0)
            # the same bytes from call to call
            assert s.spectral_scale(G, kind).cpu().numpy().tobytes() == sc.tobytes()
            assert s.spectral_apply(G, _dev(x), kind).cpu().numpy().tobytes() == y.tobytes()
            seen[group] = sc.tobytes() + y.tobytes()
        if m == 4099:
            # the switch takes effect: the long rows' sums end in other bits under another packing, and the library's own choice
            # is the smallest group that is not below the mean row length
            assert len({seen[g] for g in GROUPS}) >= 2, kind
            own = next((g for g in GROUPS if A.nnz <= g * m), 64)
            assert seen[None] == seen[own] and any(seen[None] != seen[g] for g in GROUPS if g != own), (kind, own)


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_scaled_copy_is_symmetric_bit_for_bit(sess, dt):
    m = 65
    A, _ = mixed_graph(m)
    G = _resident(sess, A, dt)
    for kind in KINDS:
        S = np.zeros((m, m))
        for j in range(m):                     # S e_j: a column of the scaled copy, exactly (every other product is a 0)
            e = np.zeros(m)
            e[j] = 1.0
            S[:, j] = sess.spectral_apply(G, _dev(e), kind).cpu().numpy()
        assert S.tobytes() == np.ascontiguousarray(S.T).tobytes()
        assert np.array_equal(S != 0, A.toarray() != 0)


def test_packing_follows_the_mean_row_length(sess):
    # rings of 2 k neighbours: mean lengths 4, 12, 24, 48, 100 take groups of 8, 16, 32, 64, 64; every one gives the sums of ones
    m = 300
    x = np.random.default_rng(4).normal(size=m)
    for half in (2, 6, 12, 24, 50):
        off = np.concatenate([np.arange(1, half + 1), -np.arange(1, half + 1)])
        rows = np.repeat(np.arange(m), len(off))
        cols = (rows + np.tile(off, m)) % m
        A = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(m, m))
        A.sort_indices()
        G = _resident(sess, A, np.float64)
        sc = sess.spectral_scale(G, "normalized").cpu().numpy()
        assert np.all(sc == sc[0]) and abs(sc[0] - 1.0 / np.sqrt(2.0 * half)) <= 3 * EPS * sc[0]   # (the sum of ones is exact)
        y = sess.spectral_apply(G, _dev(x), "normalized").cpu().numpy()
        want = (A @ x) / (2 * half)
        # (2 half + 4) eps sum_j |S_ij x_j| for the library and as much for numpy's own sum
        assert np.max(np.abs(y - want)) <= 2 * (2 * half + 4) * EPS * np.max(np.abs(x))


# ------------------------------------------------------------------ the eigen-solve
def _check_pairs(gold, name, kind, dt, n_eigen, evals, evecs, evecs64, ncomp, steps, tol):
    """evecs: the variant under test; evecs64: the f64 variant's of the same graph, which r_i is taken from"""
    LD = np.longdouble
    r = _ref(gold, name, kind)
    fine, S = r["fine"], r["S_ld"]
    V, V64 = evecs.astype(LD), evecs64.astype(LD)
    c = min(r["n_locked"], n_eigen)
    assert ncomp == r["n_components"]
    assert np.all(evals[:c] == 1.0)
    ulp4 = 4 * np.spacing(np.abs(r["evecs"][:, :c]).astype(dt)).astype(np.float64)
    assert np.all(np.abs(evecs[:, :c].astype(np.float64) - r["evecs"][:, :c].astype(dt).astype(np.float64)) <= ulp4)
    if c >= n_eigen:
        assert steps == 0
        return
    assert 0 < steps
    rb = tol + 64 * steps * EPS
    assert np.all(np.diff(evals) <= 0)
    for i in range(c, n_eigen):
        gap = r["gaps"][i]
        theta = LD(evals[i])
        ri = float(np.sqrt(np.sum((S @ V64[:, i] - theta * V64[:, i]) ** 2)))
        dth = float(abs(theta - fine["evals"][i]))
        dv = float(np.sqrt(np.sum((V[:, i] - fine["evecs"][:, i]) ** 2)))
        extra = 2.0 ** -23 if dt == np.float32 else 0.0
        print(f"{name} {kind} {np.dtype(dt).name} n_eigen {n_eigen} pair {i}: r {ri:.3e} (bound {rb:.3e}), |theta - lambda| {dth:.3e}, "
              f"|v - v_ref| {dv:.3e} (bound {4 * ri / gap + extra:.3e}, gap {gap:.3e})")
        assert ri <= rb, (i, ri, rb)
        assert dth <= ri, (i, dth, ri)
        assert dv <= 4 * ri / gap + extra, (i, dv, ri, gap)
        at = int(np.argmax(np.abs(evecs[:, i])))
        assert evecs[at, i] > 0


@pytest.mark.parametrize("n_eigen", [1, 3, 16])
@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["conn", "disc"])
def test_eigenpairs_of_the_golden_graphs(sess, gold, name, kind, dt, n_eigen):
    G = _resident(sess, _graph(gold, name), dt)
    tol = 1e-8
    evals, evecs, ncomp, steps = sess.spectral(G, n_eigen=n_eigen, kind=kind, tol=tol)
    E = evecs.cpu().numpy()
    assert E.dtype == dt and E.shape == (G.shape[0], n_eigen)
    E64 = E
    if dt == np.float32:     # the graph is float32-exact and every sum is f64: the f64 variant runs the same iteration
        ev64, E64t, _, st64 = sess.spectral(_resident(sess, _graph(gold, name), np.float64), n_eigen=n_eigen, kind=kind, tol=tol)
        assert ev64.tobytes() == evals.tobytes() and st64 == steps
        E64 = E64t.cpu().numpy()
    _check_pairs(gold, name, kind, dt, n_eigen, evals, E, E64, ncomp, steps, tol)
    if name == "disc":
        assert ncomp == 5 and np.all(evals[:min(3, n_eigen)] == 1.0)
        if n_eigen <= 3:
            assert steps == 0
    else:
        assert evals[0] == 1.0
    # the same bytes from call to call, and from the host route
    ev2, E2, nc2, st2 = sess.spectral(G, n_eigen=n_eigen, kind=kind, tol=tol)
    assert ev2.tobytes() == evals.tobytes() and E2.cpu().numpy().tobytes() == E.tobytes() and (nc2, st2) == (ncomp, steps)
    A = _graph(gold, name)
    ev3, E3, nc3, st3 = sess.spectral_host(A.indptr, A.indices, A.data.astype(dt), n_eigen=n_eigen, kind=kind, tol=tol)
    assert ev3.tobytes() == evals.tobytes() and E3.tobytes() == E.tobytes() and (nc3, st3) == (ncomp, steps)


def _planted(m, blocks=4, seed=12):
    """a connected graph of `blocks` planted clusters: 10 partners inside the own cluster and 1 anywhere per vertex, weights in
    (0.5, 1.5): three eigenvalues stand clear of the bulk, so a few dozen steps converge 4 pairs"""
    rng = np.random.default_rng(seed)
    size = m // blocks
    v = np.arange(m)
    own = (v // size).clip(max=blocks - 1)
    lo = own * size
    hi = np.where(own == blocks - 1, m, lo + size)
    rows = np.concatenate([np.repeat(v, 10), v])
    cols = np.concatenate([(lo[:, None] + (rng.random((m, 10)) * (hi - lo)[:, None]).astype(np.int64)).ravel(), rng.integers(0, m, m)])
    keep = rows != cols
    A = sp.csr_matrix((np.ones(keep.sum()), (rows[keep], cols[keep])), shape=(m, m))
    A = sp.triu(sp.csr_matrix(((A + A.T) > 0).astype(np.float64)), k=1).tocoo()
    w = (0.5 + rng.random(A.nnz)).astype(np.float32).astype(np.float64)
    U = sp.csr_matrix((w, (A.row, A.col)), shape=(m, m))
    G = sp.csr_matrix(U + U.T)
    G.sort_indices()
    return G


def _with_stray_columns(A, rows=(0, 17)):
    """A's arrays with a column of -1 in front of and columns of m and 2^31 - 1 behind the entries of `rows` (weight 1)"""
    m = A.shape[0]
    ptr, idx, dat = [0], [], []
    for i in range(m):
        c, v = A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]
        if i in rows:
            c, v = np.concatenate([[-1], c, [m, 2 ** 31 - 1]]), np.concatenate([[1.0], v, [1.0, 1.0]])
        idx.append(c)
        dat.append(v)
        ptr.append(ptr[-1] + len(c))
    return np.array(ptr, dtype=np.int64), np.concatenate(idx).astype(np.int32), np.concatenate(dat)


def _sparse_operator(A, kind):
    q = np.asarray(A.sum(axis=1)).ravel()
    if kind == SR.NORMALIZED:
        s = 1.0 / np.sqrt(q)
    else:
        z = np.asarray((sp.diags(1.0 / q) @ A @ sp.diags(1.0 / q)).sum(axis=1)).ravel()
        s = 1.0 / (q * np.sqrt(z))
    return sp.csr_matrix(sp.diags(s) @ A @ sp.diags(s))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [300, 4500])
def test_columns_outside_the_graph_are_skipped_by_the_solve(sess, gold, m, kind):
    """m = 300: the step's product is the wave-per-row kernel; m = 4500: the one with x staged in LDS (4096 <= m <= 19200).
    Neither looks at its columns, so the solve gives them a safe copy: a graph with stray columns is solved as the graph
    without them (the sums run over other lane positions, hence bounds and not bytes)."""
    A = _graph(gold, "conn") if m == 300 else _planted(m)
    assert csgraph.connected_components(A, directed=False)[0] == 1
    S = _sparse_operator(A, kind)
    tol, n_eigen = 1e-8, 4
    ptr, idx, dat = _with_stray_columns(A)
    clean = _resident(sess, A, np.float64)
    stray = ops.ResidentCsr.from_torch(sess, _dev(ptr), _dev(idx), _dev(dat), A.shape)
    results = []
    for G in (clean, stray):
        evals, E, ncomp, steps = sess.spectral(G, n_eigen=n_eigen, kind=kind, tol=tol)
        V = E.cpu().numpy()
        assert ncomp == 1 and evals[0] == 1.0 and 0 < steps < 400
        for i in range(n_eigen):
            assert np.linalg.norm(S @ V[:, i] - evals[i] * V[:, i]) <= tol + 64 * steps * EPS + 16 * EPS, (i, steps)
        np.testing.assert_allclose(V.T @ V, np.eye(n_eigen), atol=1e-10)
        results.append((evals, V))
    # two solves of the same operator: eigenvalues within the sum of their residual bounds
    assert np.max(np.abs(results[0][0] - results[1][0])) <= 2 * (tol + 64 * 400 * EPS)
    np.testing.assert_allclose(sess.spectral_scale(stray, kind).cpu().numpy(), sess.spectral_scale(clean, kind).cpu().numpy(), rtol=128 * EPS)   # (the scale test's own bound at these row lengths)
    x = _dev(np.random.default_rng(3).normal(size=m))
    y0, y1 = sess.spectral_apply(clean, x, kind).cpu().numpy(), sess.spectral_apply(stray, x, kind).cpu().numpy()
    assert np.max(np.abs(y0 - y1)) <= 512 * EPS * np.max(np.abs(x.cpu().numpy()))
    assert np.array_equal(sess.graph_components(stray)[0].cpu().numpy(), np.zeros(m, dtype=np.int32))


def _raw_spectral(sess, G, o, evals=True, evecs=True, m=None, ptr=True):
    m = G.shape[0] if m is None else m
    ev = np.zeros(64)
    E = torch.empty((max(G.shape[0], 1), 64), dtype=torch.float64, device="cuda")
    return L.load().sapca_spectral_device_f64(
        sess._h, C.c_uint64(m), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr if ptr else None), C.c_void_p(G.d_idx), C.c_void_p(G.d_val),
        C.byref(o) if o is not None else None, ev.ctypes.data_as(C.POINTER(C.c_double)) if evals else None,
        C.c_void_p(E.data_ptr() if evecs else None), None, None)


def test_refusals_name_their_number_and_leave_the_handle_usable(sess, gold):
    G = _resident(sess, _graph(gold, "conn"), np.float64)

    def refused(match, **kw):
        o = L.default_spectral_options()
        for k, v in kw.pop("opts", {}).items():
            setattr(o, k, v)
        st = _raw_spectral(sess, G, o, **kw)
        msg = (L.load().sapca_last_error(sess._h) or b"").decode()
        assert st == 1 and match in msg, (st, msg)

    refused("struct_size is 31", opts=dict(struct_size=31))
    refused("unknown kind 2", opts=dict(kind=2))
    refused("n_eigen = 0 is outside 1 .. 64", opts=dict(n_eigen=0))
    refused("n_eigen = 65 is outside 1 .. 64", opts=dict(n_eigen=65))
    refused("max_steps = 4097 exceeds 4096", opts=dict(max_steps=4097))
    refused("tol = -1", opts=dict(tol=-1.0))
    refused("tol = nan", opts=dict(tol=float("nan")))
    refused("tol = inf", opts=dict(tol=float("inf")))
    refused("m = 2147483648 rows", m=1 << 31)
    refused("n_eigen = 16 exceeds m = 8", m=8)
    refused("NULL row offsets with m = 300", ptr=False)
    refused("a NULL output with m = 300", evals=False)
    refused("a NULL output with m = 300", evecs=False)
    assert _raw_spectral(sess, G, None) == 1 and b"null options" in L.load().sapca_last_error(sess._h)
    st = L.load().sapca_spectral_scale_device_f64(sess._h, C.c_uint64(300), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx),
                                                  C.c_void_p(G.d_val), C.c_uint32(7), None)
    assert st == 1 and b"unknown kind 7" in L.load().sapca_last_error(sess._h)
    E = torch.zeros((300, 3), dtype=torch.float64, device="cuda")
    Y = torch.zeros((300, 3), dtype=torch.float64, device="cuda")
    for od, ne, ld, match in ((0, 3, 3, b"output_dim = 0"), (4, 5, 5, b"output_dim = 4"), (3, 3, 3, b"n_eigen = 3"), (2, 3, 2, b"ld = 2")):
        st = L.load().sapca_umap_spectral_init_device_f64(sess._h, C.c_uint64(300), C.c_uint32(od), C.c_void_p(E.data_ptr()), C.c_uint64(ld),
                                                          C.c_uint32(ne), C.c_uint32(1), C.c_void_p(Y.data_ptr()))
        assert st == 1 and match in L.load().sapca_last_error(sess._h), (od, ne, ld)
    # five steps cannot converge 15 pairs: SAPCA_ERR_SVD with the counts, and the handle goes on working
    with pytest.raises(L.SapcaError, match=r"spectral: Lanczos did not converge 15 of 16 pairs in 5 steps") as e:
        sess.spectral(G, n_eigen=16, max_steps=5)
    assert e.value.status == 4
    evals, _, ncomp, steps = sess.spectral(G, n_eigen=3)
    assert evals[0] == 1.0 and ncomp == 1 and steps >= 2
    # a graph without weights has nothing to iterate on beyond one vector: refused, not padded with zero pairs
    bare = _resident(sess, sp.csr_matrix((5, 5)), np.float64)
    with pytest.raises(L.SapcaError, match=r"spectral: the Krylov space is exhausted after 1 steps, 3 pairs were to be iterated") as e:
        sess.spectral(bare, n_eigen=3)
    assert e.value.status == 4
    ev1, E1, n1, s1 = sess.spectral(bare, n_eigen=1)
    assert ev1[0] == 0.0 and (n1, s1) == (5, 1) and abs(np.linalg.norm(E1.cpu().numpy()) - 1.0) <= 4 * EPS
    # m == 0 writes nothing
    Z = _resident(sess, sp.csr_matrix((0, 0)), np.float64)
    ev0, E0, n0, s0 = sess.spectral(Z, n_eigen=1)
    assert (n0, s0) == (0, 0) and tuple(E0.shape) == (0, 1)


def test_other_buffers_are_untouched(gold):
    rng = np.random.default_rng(6)
    m, n = 600, 90
    dense = (rng.random((m, n)) < 0.15) * rng.random((m, n))
    M = sp.csr_matrix(dense.astype(np.float32))
    pca = (sapca.SparsePCABuilder.new().n_components(4).random_seed(42)
           .svd_method(sapca.SVDMethod.Random(4, 2, sapca.PowerIterationNormalizer.QR)).build())
    scores = pca.fit_transform(sapca.DeviceCsr(_dev(M.indptr.astype(np.int64)), _dev(M.indices.astype(np.int32)), _dev(M.data), (m, n)))
    comps = pca.components_(np.float64).copy()

    def transformed():
        return pca.transform(sapca.DeviceCsr(_dev(M.indptr.astype(np.int64)), _dev(M.indices.astype(np.int32)), _dev(M.data), (m, n))
                             ).cpu().numpy().tobytes()
    projected = transformed()
    s = pca.session()
    idx, dist = s.knn(scores, n_neighbors=14, metric="euclidean", exclude_self=True)
    G = s.umap_graph(idx, dist, 15)[0]

    def host(R):
        d = R.as_device_csr()
        return d.row_offsets.cpu().numpy().tobytes(), d.col_indices.cpu().numpy().tobytes(), d.values.cpu().numpy().tobytes()
    labels, _, _, _ = s.louvain(G, seed=42)
    coarse, ren = s.louvain_aggregate(G, labels)
    before = (host(G), host(coarse), labels.cpu().numpy().tobytes())
    for kind in KINDS:
        s.spectral(G, n_eigen=8, kind=kind)
        s.spectral_apply(G, _dev(np.ones(m)).to(torch.float64), kind)
    s.graph_components(G)
    assert (host(G), host(coarse), labels.cpu().numpy().tobytes()) == before
    assert pca.components_(np.float64).tobytes() == comps.tobytes()
    assert transformed() == projected      # the fitted model still projects to the same bytes


# ------------------------------------------------------------------ the spectral start and the diffusion map
@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_spectral_start_is_the_formula_and_feeds_the_layout(sess, gold, dt):
    G = _resident(sess, _graph(gold, "conn"), dt)
    for D in (1, 2, 3):
        Y0 = sess.umap_spectral_init(G, output_dim=D, seed=9)
        _, E, _, _ = sess.spectral(G, n_eigen=D + 1, kind="normalized", seed=9)
        want = SR.umap_spectral_init(E.cpu().numpy(), D, 9)
        assert Y0.cpu().numpy().dtype == dt and Y0.cpu().numpy().tobytes() == want.tobytes()
        assert abs(float(np.abs(want).max()) - 10.0) <= 2e-4
    Y0 = sess.umap_spectral_init(G, output_dim=2, seed=9)
    Y1 = sess.umap_embed(G, n_epochs=30, output_dim=2, init=Y0, seed=5)
    Y2 = sess.umap_embed(G, n_epochs=30, output_dim=2, init=Y0, seed=5)
    assert Y1.cpu().numpy().tobytes() == Y2.cpu().numpy().tobytes() and np.all(np.isfinite(Y1.cpu().numpy()))
    assert Y1.cpu().numpy().tobytes() != Y0.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="unknown init"):
        sess.umap(torch.zeros((40, 3), device="cuda"), init="spectral")
    # a disconnected graph: the start is computed, with a warning
    D = _resident(sess, _graph(gold, "disc"), dt)
    with pytest.warns(RuntimeWarning, match="5 connected components"):
        Yd = sess.umap_spectral_init(D, output_dim=2, seed=9)
    assert np.all(np.isfinite(Yd.cpu().numpy()))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sess.umap_spectral_init(G, output_dim=2, seed=9)


@pytest.mark.parametrize("dt", DTYPES, **IDS)
def test_diffmap_of_a_panel_is_the_solve_on_its_graph(sess, dt):
    rng = np.random.default_rng(8)
    X = _dev(np.concatenate([rng.normal(size=(150, 6)), rng.normal(size=(150, 6)) + 2.5]).astype(dt))
    Xd, ev = sess.diffmap(X, n_comps=6, n_neighbors=15)
    idx, dist = sess.knn(X, n_neighbors=14, metric="euclidean", exclude_self=True)
    G = sess.umap_graph(idx, dist, 15)[0]
    ev2, E2, _, _ = sess.spectral(G, n_eigen=6, kind="diffmap")
    assert ev.tobytes() == ev2.tobytes() and Xd.cpu().numpy().tobytes() == E2.cpu().numpy().tobytes()
    Xg, ev3 = sess.diffmap(G, n_comps=6)
    assert ev3.tobytes() == ev.tobytes() and Xg.cpu().numpy().tobytes() == E2.cpu().numpy().tobytes()
    assert ev[0] == 1.0 and np.all(np.diff(ev) <= 0) and tuple(Xd.shape) == (300, 6)

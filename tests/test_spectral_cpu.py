"""The numpy restatement of the spectral section (tests/spectral_ref.py) held to scipy and scikit-learn, the golden file held
to the restatement, and what of the new surface can be checked without a device."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph
import scipy.sparse.linalg as spla

import spectral_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (SR.NORMALIZED, SR.DIFFMAP)
FIXTURES = ("conn", "disc")
MIN_GAP = 5e-4


@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_spectral.npz")


def _csr(z, name):
    ptr, idx, dat = z[f"{name}_indptr"], z[f"{name}_indices"], z[f"{name}_data"].astype(np.float64)
    m = len(ptr) - 1
    return ptr, idx, dat, sp.csr_matrix((dat, idx, ptr), shape=(m, m))


@pytest.fixture(scope="module")
def restated(g14):
    """the restatement on every fixture and kind, once"""
    out = {}
    for name in FIXTURES:
        ptr, idx, dat, _ = _csr(g14, name)
        for kind in KINDS:
            out[name, kind] = SR.eigenpairs(ptr, idx, dat, kind, 16)
    return out


def test_fixtures_are_what_the_issue_asks_for(g14):
    ptr, idx, dat, A = _csr(g14, "conn")
    assert A.shape == (300, 300) and 13 <= A.nnz / 300 <= 15
    assert abs(A - A.T).max() == 0 and A.data.min() > 0
    assert np.array_equal(g14["conn_data"].astype(np.float64).astype(np.float32), g14["conn_data"])
    ptr, idx, dat, B = _csr(g14, "disc")
    assert B.shape == (402, 402) and abs(B - B.T).max() == 0
    lens = np.diff(ptr)
    assert sorted(np.flatnonzero(lens == 0).tolist()) == [7, 401]
    assert int(g14["conn_n_components"]) == 1 and int(g14["disc_n_components"]) == 5
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g14_spectral.npz")) < 200 * 1024


def test_golden_is_the_restatement(g14, restated):
    for (name, kind), r in restated.items():
        np.testing.assert_allclose(g14[f"{name}_{kind}_evals"], r["evals"], rtol=0, atol=1e-12)
        assert int(g14[f"{name}_{kind}_n_locked"]) == r["n_locked"]
        # vectors up to what eigh's rounding does at the smallest gap
        err = np.abs(g14[f"{name}_{kind}_evecs"] - r["evecs"]).max()
        assert err <= 1e-10 / MIN_GAP, (name, kind, err)
        assert np.array_equal(g14[f"{name}_labels"], r["labels"])


def test_every_compared_gap_is_at_least_5e_4(restated):
    for (name, kind), r in restated.items():
        assert np.min(r["gaps"]) >= MIN_GAP, (name, kind, np.min(r["gaps"]))
        # ... and the compared eigenvalues themselves are apart by as much (the locked 1.0s are exact copies and are not compared)
        free = r["evals"][r["n_locked"]:]
        assert np.min(-np.diff(free)) >= MIN_GAP, (name, kind)


def test_refined_pairs_are_eigenpairs_far_below_eps(restated):
    LD = np.longdouble
    assert np.finfo(LD).eps < 1e-18, "the refinement needs a longdouble wider than double (x86's 80-bit format)"
    for (name, kind), r in restated.items():
        fine = SR.refined_pairs(r)
        S = r["S"].astype(LD)
        for i in range(r["n_locked"], 16):
            v, lam = fine["evecs"][:, i], fine["evals"][i]
            assert float(np.sqrt(np.sum((S @ v - lam * v) ** 2))) <= 1e-17, (name, kind, i)
            assert abs(float(np.dot(v, v)) - 1.0) <= 1e-17
            assert abs(float(lam) - r["evals"][i]) <= 1e-13
            assert float(np.sqrt(np.sum((v - r["evecs"][:, i]) ** 2))) <= 1e-13 / r["gaps"][i]


def test_normalized_operator_is_identity_minus_scipy_laplacian(g14):
    for name in FIXTURES:
        _, _, _, A = _csr(g14, name)
        S, s = SR.operator(A.toarray(), SR.NORMALIZED)
        Lsym = csgraph.laplacian(A, normed=True).toarray()
        keep = s > 0   # (scipy leaves a 0 on the diagonal of an isolated vertex where I - S has a 1)
        np.testing.assert_allclose((np.eye(A.shape[0]) - S)[np.ix_(keep, keep)], Lsym[np.ix_(keep, keep)], rtol=0, atol=4e-16)
        assert np.all(S[~keep] == 0) and np.all(S[:, ~keep] == 0)


def test_eigenvalues_equal_eigsh_on_the_connected_fixture(g14, restated):
    _, _, _, A = _csr(g14, "conn")
    for kind in KINDS:
        S, _ = SR.operator(A.toarray(), kind)
        w = np.sort(spla.eigsh(sp.csr_matrix(S), k=16, which="LA", tol=1e-12, v0=np.ones(300))[0])[::-1]
        np.testing.assert_allclose(restated["conn", kind]["evals"], w, rtol=0, atol=1e-10)
        assert restated["conn", kind]["evals"][0] == 1.0 and restated["conn", kind]["n_locked"] == 1


def test_sklearn_spectral_embedding_is_the_eigenvectors_divided_by_sqrt_d(g14, restated):
    from sklearn.manifold import spectral_embedding
    _, _, _, A = _csr(g14, "conn")
    k = 8
    emb = spectral_embedding(A, n_components=k, norm_laplacian=True, drop_first=False, eigen_solver="arpack", random_state=0,
                             eigen_tol=1e-12)
    d = np.asarray(A.sum(axis=1)).ravel()
    V = emb * np.sqrt(d)[:, None]            # its division by sqrt(d) undone
    V /= np.linalg.norm(V, axis=0)
    r = restated["conn", SR.NORMALIZED]
    want = r["evecs"][:, :k]
    for c in range(k):
        sign = np.sign(V[:, c] @ want[:, c])
        bound = 1e-7 / r["gaps"][c] if np.isfinite(r["gaps"][c]) else 1e-7
        assert np.linalg.norm(sign * V[:, c] - want[:, c]) <= bound, c
    # the first is the analytic one: sqrt(d) normalised
    np.testing.assert_allclose(want[:, 0], np.sqrt(d) / np.linalg.norm(np.sqrt(d)), rtol=1e-14)


def test_component_labels_equal_scipy(g14):
    rng = np.random.default_rng(5)
    graphs = [_csr(g14, name)[3] for name in FIXTURES]
    perm = rng.permutation(200)
    graphs.append(sp.csr_matrix((np.ones(199), (perm[:-1], perm[1:])), shape=(200, 200)))          # a path, randomly numbered
    graphs.append(sp.csr_matrix((np.ones(40), (rng.integers(0, 120, 40), rng.integers(0, 120, 40))), shape=(120, 120)))
    graphs.append(sp.csr_matrix((3, 3)))
    for A in graphs:
        A = sp.csr_matrix(A + A.T)
        lab, n = SR.components(A.indptr.astype(np.int64), A.indices.astype(np.int32))
        n_want, want = csgraph.connected_components(A, directed=False)
        assert n == n_want and np.array_equal(lab, want)


def test_diffmap_matrix_is_scanpys_transition_matrix(g14):
    for name in FIXTURES:
        _, _, _, A = _csr(g14, name)
        W = A.toarray()
        S, s = SR.operator(W, SR.DIFFMAP)
        keep = s > 0
        # scanpy's compute_transitions(density_normalize=True): K = Q^-1 W Q^-1, z = K 1, T_sym = Z^-1/2 K Z^-1/2
        q = W.sum(axis=1)
        Wk, qk = W[np.ix_(keep, keep)], q[keep]
        K = Wk / np.outer(qk, qk)
        z = K.sum(axis=1)
        Tsym = K / np.sqrt(np.outer(z, z))
        np.testing.assert_allclose(S[np.ix_(keep, keep)], Tsym, rtol=1e-13, atol=0)
        # sqrt(z) = 1 / (s q) is an eigenvector of eigenvalue 1 on every component (T_sym sqrt(z) = Z^-1/2 K 1 = sqrt(z)); the
        # vector q sqrt(z) = 1 / s is NOT one unless q is constant: S (q sqrt(z)) = 1 / sqrt(z)
        u = SR.analytic(W, SR.DIFFMAP, s)
        np.testing.assert_allclose(S @ u, u, rtol=1e-12, atol=1e-12 * u.max())
        np.testing.assert_allclose(u[keep], np.sqrt(z), rtol=1e-13)
        v = np.where(keep, 1.0 / np.where(keep, s, 1.0), 0.0)
        np.testing.assert_allclose((S @ v)[keep], 1.0 / np.sqrt(z), rtol=1e-12)
        # ... and the random-walk matrix Z^-1/2 S Z^1/2 has unit row sums
        T = Tsym * np.sqrt(z)[None, :] / np.sqrt(z)[:, None]
        np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=1e-12)


def test_locked_vectors_are_orthonormal_eigenvectors(restated):
    for kind in KINDS:
        r = restated["disc", kind]
        assert r["n_locked"] == 3 and r["n_components"] == 5 and np.all(r["evals"][:3] == 1.0)
        U = r["evecs"][:, :3]
        np.testing.assert_allclose(U.T @ U, np.eye(3), atol=1e-14)
        np.testing.assert_allclose(r["S"] @ U, U, atol=1e-14)
        assert np.all(U >= 0) and np.all(U[[7, 401]] == 0)
        V = r["evecs"]
        np.testing.assert_allclose(V.T @ V, np.eye(16), atol=1e-10)


def test_rounds_restatement_equals_eigh_with_multiplicity():
    """SR.lanczos_rounds (stage 5 of include/sapca.h restated: runs, locking, the closing round) on graphs whose leading
    eigenvalues are repeated, nearly repeated or few: values equal eigh's counted with multiplicity, every vector lies in the
    eigenspace of its value's cluster, the columns are orthonormal; on a graph with simple leading values the first run's
    pairs are the result and one closing round is made; single_round is the single run"""
    import lanczos_spectra_cases as LC
    for name in LC.GRAPHS:
        for kind in KINDS:
            g = LC.graph_spectrum(name, kind)
            c = g["U"].shape[1]
            for n_eigen in (3, 9):
                k = n_eigen - c
                r = SR.lanczos_rounds(g["S"], g["U"], k)
                np.testing.assert_allclose(r["evals"], g["w"][:k], rtol=0, atol=1e-10, err_msg=f"{name} {kind} {n_eigen}")
                V = r["evecs"]
                np.testing.assert_allclose(V.T @ V, np.eye(k), atol=1e-12)
                np.testing.assert_allclose(g["U"].T @ V, 0, atol=1e-12)
                groups = LC.clusters(g["w"], 10 * LC.TOL)
                for i in range(k):
                    a, b = next(x for x in groups if x[0] <= i < x[1])
                    gap = min(g["w"][a - 1] - g["w"][a] if a else np.inf, g["w"][b - 1] - g["w"][b] if b < len(g["w"]) else np.inf)
                    Qc = g["Q"][:, a:b]
                    assert np.linalg.norm(V[:, i] - Qc @ (Qc.T @ V[:, i])) <= 4 * np.sqrt(1 + 2 * k) * LC.TOL / gap + 1e-10, (name, kind, i)
                    assert V[np.argmax(np.abs(V[:, i])), i] > 0
    # simple leading values: the golden connected graph
    z = np.load(os.path.join(ROOT, "tests", "golden", "g14_spectral.npz"))
    ptr, idx, dat, _ = _csr(z, "conn")
    ref = SR.eigenpairs(ptr, idx, dat, SR.NORMALIZED, 6)
    W = SR.dense(ptr, idx, dat)
    S, s = SR.operator(W, SR.NORMALIZED)
    U = SR.locked_vectors(SR.analytic(W, SR.NORMALIZED, s), ref["labels"], ref["n_components"])
    r = SR.lanczos_rounds(S, U, 5)
    one = SR.lanczos_rounds(S, U, 5, single_round=True)
    assert r["rounds"] == 2 and one["rounds"] == 1 and one["steps"] < r["steps"]
    assert np.array_equal(r["evals"], one["evals"]) and np.array_equal(r["evecs"], one["evecs"]) and np.array_equal(r["first"], r["evals"])
    np.testing.assert_allclose(r["evals"], ref["evals"][1:], rtol=0, atol=1e-10)


def test_sign_rule_and_start_formula():
    V = np.array([[0.5, -0.2], [-0.5, 0.1], [0.1, -0.2]])
    F = SR.fix_sign(V)
    assert F[0, 0] > 0 and F[0, 1] > 0 and np.array_equal(np.abs(F), np.abs(V))   # (ties: the lowest index decides)
    from sapca import synth
    import torch
    idx = torch.arange(12, dtype=torch.int64)
    want = synth.hash_u01(9, 51, idx).numpy()
    got = np.array([SR.hash_u01(9, 51, int(i)) for i in idx])
    assert np.array_equal(got, want)
    E = np.random.default_rng(0).normal(size=(6, 3))
    Y = SR.umap_spectral_init(E, 2, 9)
    assert Y.shape == (6, 2) and abs(np.abs(Y).max() - 10.0) <= 1e-4 + 1e-12
    # the same formula written once more, vectorised, with the package's generator
    for dt in (np.float32, np.float64):
        Et = np.random.default_rng(1).normal(size=(50, 4)).astype(dt)
        for D in (1, 2, 3):
            u = synth.hash_u01(9, 51, torch.arange(50 * D, dtype=torch.int64)).numpy().reshape(50, D)
            lead = Et[:, 1:1 + D].astype(np.float64)
            want2 = ((10.0 * lead) / np.abs(lead).max() + 1e-4 * (2.0 * u - 1.0)).astype(dt)
            assert SR.umap_spectral_init(Et, D, 9).tobytes() == want2.tobytes()


def test_host_side_argument_checks_need_no_device():
    from sapca import ops
    s = ops.Session.borrow(None)               # no handle: everything below fails before one is needed
    with pytest.raises(ValueError, match="unknown kind"):
        s.spectral(None, kind="laplacian")
    with pytest.raises(ValueError, match="unknown kind"):
        s.spectral_scale(None, kind="sym")
    with pytest.raises(ValueError, match="unknown kind"):
        s.spectral_apply(None, None, kind=3)
    with pytest.raises(ValueError, match="n_eigen = 65 is outside 1 .. 64"):
        s.spectral(None, n_eigen=65)
    with pytest.raises(ValueError, match="n_eigen = 0 is outside"):
        s.spectral_host([0], [], np.zeros(0), n_eigen=0)
    with pytest.raises(ValueError, match="tol must be finite"):
        s.spectral(None, tol=-1.0)
    with pytest.raises(ValueError, match="tol must be finite"):
        s.spectral(None, tol=float("nan"))
    with pytest.raises(ValueError, match="max_steps = 5000 is outside"):
        s.spectral(None, max_steps=5000)
    with pytest.raises(ValueError, match="square ResidentCsr"):
        s.spectral(np.zeros((4, 4)))
    with pytest.raises(ValueError, match="square ResidentCsr"):
        s.graph_components(np.zeros((4, 4)))
    with pytest.raises(ValueError, match="float32 / float64"):
        s.spectral_host([0, 1], [0], np.ones(1, dtype=np.int32))
    with pytest.raises(ValueError, match="n_eigen = 3 exceeds m = 2"):
        s.spectral_host([0, 1, 2], [1, 0], np.ones(2), n_eigen=3)
    with pytest.raises(ValueError, match="n_comps = 0 is outside"):
        s.diffmap(None, n_comps=0)
    with pytest.raises(ValueError, match="output_dim = 4 is outside 1 .. 3"):
        s.umap_spectral_init(None, output_dim=4)
    with pytest.raises(ValueError, match="unknown init"):       # the string stays refused: the start is given as an array
        ops.Session.umap(s, np.zeros((40, 3)), init="spectral")
    o = s._spectral_options(16, "diffmap", 1e-8, None, 7)
    assert (o.kind, o.n_eigen, o.max_steps, o.random_seed, o.tol, o.struct_size) == (1, 16, 0, 7, 1e-8, 32)


def test_symbols_are_declared_everywhere():
    import sapca
    from sapca import _lib as L
    from sapca import ops
    lib = sapca.load()
    names = ["sapca_spectral_options_default", "sapca_graph_components_device"] + [f"{n}_{suf}" for suf in ("f32", "f64") for n in (
        "sapca_spectral_scale_device", "sapca_spectral_apply_device", "sapca_spectral_device", "sapca_spectral",
        "sapca_umap_spectral_init_device")]
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    hpp = open(os.path.join(ROOT, "single-algebra_amd", "host", "cpp", "sapca.hpp")).read()
    sys_rs = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca-sys", "src", "lib.rs")).read()
    for n in names:
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n) and re.search(rf"\b{n}\(", header), n
        assert f"pub fn {n}" in sys_rs, n
        assert n in hpp, n
    assert "pub struct sapca_spectral_options" in sys_rs and "SpectralOptions" in hpp
    for method in ("graph_components", "spectral_scale", "spectral_apply", "spectral", "spectral_host", "diffmap", "umap_spectral_init"):
        assert callable(getattr(ops.Session, method))
    o = L.default_spectral_options()
    assert (o.struct_size, o.random_seed, o.kind, o.n_eigen, o.max_steps, o.tol) == (32, 42, L.SPECTRAL_NORMALIZED, 16, 0, 1e-8)
    assert "#define SAPCA_ABI_VERSION 4" in header

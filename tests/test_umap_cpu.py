"""UMAP without a GPU: the numpy restatement (tests/umap_ref.py) against the fixture tests/golden/g10_umap.npz
(tests/golden/make_golden_umap.py), the properties the GPU tests rely on, sapca_umap_find_ab (pure host code) against the
restatement and scipy's curve_fit, the options struct against the header, and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.optimize import curve_fit

import knn_ref as KR
import umap_ref as UR
import sapca
from sapca import _lib as L
from sapca import ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g10_umap.npz")
AB_CASES = [(1.0, 0.1), (1.0, 0.5), (1.0, 0.0), (2.0, 0.3), (0.5, 0.25), (1.0, 0.99)]


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    m = g["X"].shape[0]
    g["G"] = sp.csr_matrix((g["G_data"], g["G_indices"], g["G_indptr"]), shape=(m, m))
    return g


@pytest.fixture(scope="module")
def searched(gold):
    return UR.smooth(gold["indices"], gold["dist"], int(gold["n_neighbors"]))


def test_fixture_is_what_the_restatement_computes(gold, searched):
    X, nn = gold["X"], int(gold["n_neighbors"])
    assert X.shape == (200, 8) and nn == 15 and gold["indices"].shape == (200, 14)
    idx, dist = KR.knn(X, X, nn - 1, "euclidean", exclude_self=True)
    np.testing.assert_array_equal(idx, gold["indices"])
    np.testing.assert_array_equal(dist, gold["dist"])
    sigma, rho, _, _ = searched
    np.testing.assert_array_equal(sigma, gold["sigma"])
    np.testing.assert_array_equal(rho, gold["rho"])
    G = UR.union(idx, UR.memberships(idx, dist, sigma, rho))
    np.testing.assert_array_equal(G.indptr, gold["G_indptr"])
    np.testing.assert_array_equal(G.indices, gold["G_indices"])
    np.testing.assert_array_equal(G.data, gold["G_data"])
    assert UR.find_ab(1.0, 0.1) == (float(gold["a"]), float(gold["b"]))
    np.testing.assert_array_equal(UR.init_random(200, 2, int(gold["layout_seed"])), gold["Y0"])
    for name, st in (("f32", np.float32), ("f64", np.float64)):
        Y = UR.layout(gold["G"].astype(st), gold["Y0"], int(gold["epochs"]), float(gold["a"]), float(gold["b"]),
                      seed=int(gold["layout_seed"]), storage=st)
        assert Y.dtype == st
        np.testing.assert_array_equal(Y, gold[f"Y20_{name}"])


def test_the_generator_is_the_librarys():
    import torch
    idx = np.array([0, 1, 2, 12345678901, (1 << 63) + 5], dtype=np.uint64)
    for stream in (31, 32):
        want = synth.hash_u01(42, stream, torch.from_numpy(idx.view(np.int64))).numpy()
        np.testing.assert_array_equal(UR.hash_u01(42, stream, idx), want)


def test_graph_has_the_stated_properties(gold):
    G, idx, dist, rho = gold["G"], gold["indices"], gold["dist"], gold["rho"]
    m, K = idx.shape
    assert (G != G.T).nnz == 0                                           # symmetric bit for bit
    assert G.has_canonical_format
    assert (G.data > 0).all() and (G.data <= 1).all()
    has_positive = (dist > 0).any(axis=1)
    assert has_positive.all() and (rho == dist.min(axis=1)).all()
    # every row's largest membership is 1 (its nearest neighbour's).  The union keeps it up to ONE rounding: fl(1 + b) - b is 1
    # or 1 - 2^-53 in f64, never above 1 (measured on this fixture: both occur); rounded to f32 it is 1 exactly
    a = UR.memberships(idx, dist, gold["sigma"], rho)
    assert (a.max(axis=1)[has_positive] == 1.0).all()
    top = G.max(axis=1).toarray().ravel()[has_positive]
    assert (top <= 1.0).all() and (top >= 1.0 - 2.0 ** -53).all()
    assert (G.astype(np.float32).max(axis=1).toarray().ravel()[has_positive] == 1.0).all()
    listed = sp.csr_matrix((np.ones(m * K), (np.repeat(np.arange(m), K), idx.ravel())), shape=(m, m))
    mutual = listed.multiply(listed.T).nnz
    assert 0 < mutual < listed.nnz                                       # mutual and one-sided neighbours both occur
    assert G.nnz == 2 * listed.nnz - mutual
    # a one-sided pair carries its membership unchanged: (a + 0) - a 0 == a
    one_sided = [(i, k) for i in range(m) for k in range(K) if listed[idx[i, k], i] == 0]
    assert one_sided and all(G[i, idx[i, k]] == a[i, k] for i, k in one_sided)


def test_every_decision_of_the_fixtures_searches_has_a_margin(searched):
    """what lets the GPU test demand identical sigma: no step of any of the 200 searches comes within 1e-9 of stopping
    (|psum - target| against 1e-5) or of turning the other way (psum against target)"""
    sigma, rho, floored, margin = searched
    print(f"smallest decision margin {margin:.3e}; {int(floored.sum())} floored rows")
    assert margin >= 1e-9


@pytest.mark.parametrize("spread,min_dist", AB_CASES)
def test_find_ab_equals_the_restatement_and_scipy(spread, min_dist):
    a, b = sapca.find_ab_params(spread, min_dist)
    ra, rb = UR.find_ab(spread, min_dist)
    print(f"library ({a!r}, {b!r}) restatement ({ra!r}, {rb!r})")
    assert abs(a - ra) <= 1e-10 * ra and abs(b - rb) <= 1e-10 * rb
    x, y = UR.curve_points(spread, min_dist)
    (sa, sb), _ = curve_fit(UR.curve, x, y)
    print(f"scipy differs by {abs(sa / ra - 1):.2e}, {abs(sb / rb - 1):.2e} relative")
    assert abs(sa - ra) <= 1e-5 * ra and abs(sb - rb) <= 1e-5 * rb
    if (spread, min_dist) == (1.0, 0.1):
        assert abs(a - 1.576944) < 5e-7 and abs(b - 0.895061) < 5e-7


@pytest.mark.parametrize("spread,min_dist", [(0.0, 0.1), (-1.0, 0.1), (1.0, -0.1), (1.0, 3.0), (1.0, 5.0), (np.nan, 0.1),
                                             (1.0, np.nan), (np.inf, 0.1), (1.0, np.inf)])
def test_find_ab_refusals(spread, min_dist):
    with pytest.raises(L.SapcaError) as e:
        sapca.find_ab_params(spread, min_dist)
    assert e.value.status == 1                                           # SAPCA_ERR_ARG
    a, b = C.c_double(7.0), C.c_double(7.0)
    assert L.load().sapca_umap_find_ab(C.c_double(1.0), C.c_double(0.1), None, C.byref(b)) == 1
    assert sapca.find_ab_params(1.0, 0.1) == sapca.find_ab_params(1.0, 0.1)


@pytest.mark.parametrize("init", ["panel", "random"])
def test_the_restatement_separates_clusters(init):
    X, labels = UR.clusters(600, 10, 3)
    idx, dist = KR.knn(X, X, 14, "euclidean", exclude_self=True)
    G = UR.graph(idx, dist, 15)[0]
    a, b = UR.find_ab(1.0, 0.1)
    Y0 = UR.init_panel(X, 2) if init == "panel" else UR.init_random(600, 2, 42)
    Y, stats = UR.layout(G, Y0, 200, a, b, return_stats=True)
    share = UR.same_cluster_share(Y, labels)
    print(f"{init}: share {share:.4f}, largest q {stats['qmax']}")
    assert np.isfinite(Y).all()
    assert share >= 0.99
    assert stats["qmax"] <= 2 * 5                                        # q <= 2 negative_sample_rate


def _header_struct():
    text = open(os.path.join(ROOT, "include", "sapca.h")).read()
    body = re.search(r"typedef struct sapca_umap_options \{(.*?)\} sapca_umap_options;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_options_struct_matches_the_header():
    ctypes_of = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
    assert [(n, ctypes_of[t]) for n, t in _header_struct()] == list(L.UmapOptions._fields_)
    o = L.default_umap_options()
    assert o.struct_size == C.sizeof(L.UmapOptions) == 80
    got = {n: getattr(o, n) for n, _ in L.UmapOptions._fields_}
    assert got == dict(struct_size=80, random_seed=42, output_dim=2, init=0, n_neighbors=15, negative_sample_rate=5, epochs=0,
                       min_dist=0.1, spread=1.0, a=0.0, b=0.0, learning_rate=1.0, repulsion_strength=1.0)
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    assert re.search(r"SAPCA_UMAP_INIT_PANEL = 0, SAPCA_UMAP_INIT_RANDOM = 1, SAPCA_UMAP_INIT_GIVEN = 2", header)
    assert (L.UMAP_INIT_PANEL, L.UMAP_INIT_RANDOM, L.UMAP_INIT_GIVEN) == (0, 1, 2)
    assert L.load().sapca_abi_version() == 4 and "#define SAPCA_ABI_VERSION 4" in header
    assert re.search(r"additive, ABI 4: sapca_umap_options_default", header)


def test_bindings_are_present():
    lib = L.load()
    names = ["sapca_umap_options_default", "sapca_umap_find_ab"] + [f"{n}_{s}" for s in ("f32", "f64") for n in (
        "sapca_umap_graph_device", "sapca_umap_embed_device", "sapca_umap_device", "sapca_umap")]
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    for n in names:
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n) and re.search(rf"\b{n}\(", header), n
    for method in ("umap_graph", "umap_embed", "umap"):
        assert callable(getattr(ops.Session, method))
    est = sapca.UMAP()
    assert callable(est.fit_transform) and est.embedding_ is None
    assert (est.n_neighbors, est.min_dist, est.spread, est.n_epochs, est.output_dim, est.init, est.negative_sample_rate,
            est.learning_rate, est.repulsion_strength, est.a, est.b, est.random_seed) == (15, 0.1, 1.0, None, 2, "panel", 5, 1.0,
                                                                                          1.0, None, None, 42)
    hpp = open(os.path.join(ROOT, "single-algebra_amd", "host", "cpp", "sapca.hpp")).read()
    assert "umap_device" in hpp and "UmapOptions" in hpp
    rust = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca", "src", "lib.rs")).read()
    assert "pub mod umap" in rust and "pub struct UmapConfig" in rust
    umap_mod = rust[rust.index("pub mod umap"):]
    assert "pub fn run_f32" in umap_mod and "pub fn run_f64" in umap_mod
    sys_rs = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca-sys", "src", "lib.rs")).read()
    assert "pub struct sapca_umap_options" in sys_rs and "pub fn sapca_umap_find_ab" in sys_rs


def test_host_side_argument_checks_need_no_device():
    s = ops.Session.borrow(None)               # no handle: everything below fails before one is needed
    with pytest.raises(ValueError, match="unknown init"):
        ops.Session.umap(s, np.zeros((40, 3)), init="spectral")
    with pytest.raises(ValueError, match="give both"):
        ops.Session.umap(s, np.zeros((40, 3)), a=1.5)
    with pytest.raises(ValueError, match="two-dimensional float32 / float64"):
        ops.Session.umap(s, np.zeros((4, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="init must have shape"):
        ops.Session.umap(s, np.zeros((40, 3)), init=np.zeros((40, 3)))
    o, given = s._umap_options(15, 0.1, 1.0, None, 2, "random", 5, 1.0, 1.0, None, None, 7)
    assert (o.init, o.epochs, o.random_seed, o.a, o.b, given) == (L.UMAP_INIT_RANDOM, 0, 7, 0.0, 0.0, None)

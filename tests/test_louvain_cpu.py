"""Louvain clustering without a GPU: tests/louvain_ref.py (the numpy restatement the GPU tests are held to) against networkx's
louvain_communities / modularity, its decision margins, the edge shapes, the golden file, and the surface of sapca_louvain_*."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import louvain_ref as LR
import sapca
from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QUALITY = ["ring64", "ring1024", "grid30", "planted_g05", "planted_g1", "planted_g2", "G", "blob"]
GENERAL = ["G", "blob"]


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_louvain", os.path.join(ROOT, "tests", "golden", "make_golden_louvain.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def generator():
    return _generator()


@pytest.fixture(scope="module")
def fixtures(generator):
    return generator.fixtures()


@pytest.fixture(scope="module")
def built(generator):
    pytest.importorskip("networkx")
    return generator.build()


@pytest.fixture(scope="module")
def gold(golden):
    return dict(golden("g11_louvain.npz"))


def _nx_modularity(A, labels, gamma):
    nx = pytest.importorskip("networkx")
    G = nx.from_scipy_sparse_array(sp.csr_matrix(A))
    comm = [set(np.flatnonzero(labels == c).tolist()) for c in np.unique(labels)]
    return nx.community.modularity(G, comm, weight="weight", resolution=gamma)


# ------------------------------------------------------------------ 1. modularity
@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0])
def test_modularity_equals_networkx(fixtures, gold, gamma):
    for name, (A, _, _) in fixtures.items():
        if name == "blob":
            continue
        for labels in (gold[f"{name}_labels"], np.arange(A.shape[0]) % 5):
            assert abs(LR.modularity(A, labels, gamma) - _nx_modularity(A, labels, gamma)) <= 1e-12, name


def test_a_stored_diagonal_is_the_matrix_entry():
    """A_ii counts once in k_i and in s_i (the matrix convention; networkx counts a self-loop twice in the degree)"""
    A = (LR.two_cliques(4) + sp.diags(np.arange(8) / 8.0)).tocsr()
    labels = np.arange(8) // 4
    D = A.toarray()
    k = D.sum(axis=1)
    same = labels[:, None] == labels[None, :]
    for gamma in (0.5, 1.0, 2.0):
        want = ((D - gamma * np.outer(k, k) / k.sum()) * same).sum() / k.sum()
        assert abs(LR.modularity(A, labels, gamma) - want) <= 1e-12


# ------------------------------------------------------------------ 2. - 4. quality, sweeps, margins
@pytest.mark.parametrize("name", QUALITY)
def test_quality_is_inside_networkx_own_spread(gold, name):
    q, lo, hi = float(gold[f"{name}_Q"]), float(gold[f"{name}_nx_lo"]), float(gold[f"{name}_nx_hi"])
    print(f"{name}: restatement {q:.5f}, networkx seeds 0-4 {lo:.5f} .. {hi:.5f}")
    assert q >= lo - (hi - lo)
    if hi - lo < 1e-12:
        assert abs(q - lo) <= 1e-12


def test_level_zero_needs_fewer_sweeps_than_the_default_cap(gold, fixtures):
    for name in fixtures:
        assert int(gold[f"{name}_sweeps"][0]) < L.default_louvain_options().max_sweeps == 256, name


@pytest.mark.parametrize("name", GENERAL)
def test_margins_of_general_weights(gold, name):
    gain, q = float(gold[f"{name}_margin_gain"]), float(gold[f"{name}_margin_q"])
    print(f"{name}: smallest gain margin {gain:.3e}, smallest |Q' - Q - tol| {q:.3e}")
    assert gain > 1e-9 and q > 1e-9


# ------------------------------------------------------------------ 5. edge shapes
def test_edge_shapes():
    r = LR.run(LR.matching(64))
    assert r["n_communities"] == 32 and np.array_equal(r["labels"][0::2], r["labels"][1::2])
    assert LR.run(LR.clique(16))["n_communities"] == 1
    assert LR.run(LR.star(5000))["n_communities"] == 1
    r = LR.run(LR.two_cliques(8))
    assert r["n_communities"] == 2 and len(set(r["labels"][:8])) == 1 and len(set(r["labels"][8:])) == 1
    r = LR.run(LR.planted(6, 100), gamma=50.0)
    assert r["n_communities"] == 600 and r["n_levels"] == 0 and np.array_equal(r["labels"], np.arange(600))
    r = LR.run(sp.csr_matrix((0, 0)))
    assert r["n_communities"] == 0 and r["n_levels"] == 0 and r["Q"] == 0.0
    r = LR.run(sp.csr_matrix((100, 100)))
    assert r["n_communities"] == 100 and r["n_levels"] == 0 and r["Q"] == 0.0
    r = LR.run(sp.block_diag([LR.ring(64), sp.csr_matrix((10, 10))]).tocsr())
    lone = r["labels"][64:]
    assert len(set(lone)) == 10 and not set(lone) & set(r["labels"][:64])


def test_the_anchor_rule_keeps_joined_communities(fixtures):
    """no community that is joined in a sweep empties in that sweep: targets hold an inactive vertex"""
    A = fixtures["grid30"][0]
    c = np.arange(A.shape[0])
    for t in range(6):
        c2, moved, _ = LR.sweep(A, c, 42, 0, t, 1.0)
        joined = np.unique(c2[c2 != c])
        assert moved > 0 and np.isin(joined, c2[c2 == c]).all()
        c = c2


# ------------------------------------------------------------------ 6. surface
def _header_struct():
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    body = re.search(r"typedef struct sapca_louvain_options \{(.*?)\} sapca_louvain_options;", header, re.S).group(1)
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_options_struct_matches_the_header():
    ctypes_of = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
    assert [(n, ctypes_of[t]) for n, t in _header_struct()] == list(L.LouvainOptions._fields_)
    o = L.default_louvain_options()
    assert o.struct_size == C.sizeof(L.LouvainOptions) == 32
    got = {n: getattr(o, n) for n, _ in L.LouvainOptions._fields_}
    assert got == dict(struct_size=32, random_seed=42, max_levels=0, max_sweeps=256, resolution=1.0, tol=1e-7)
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    assert L.load().sapca_abi_version() == 4 and "#define SAPCA_ABI_VERSION 4" in header
    assert re.search(r"additive, ABI 4: sapca_louvain_options_default", header)


def test_bindings_are_present():
    lib = L.load()
    names = ["sapca_louvain_options_default"] + [f"{n}_{s}" for s in ("f32", "f64") for n in (
        "sapca_louvain_modularity_device", "sapca_louvain_sweep_device", "sapca_louvain_aggregate_device", "sapca_louvain_device",
        "sapca_louvain")]
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    for n in names:
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n) and re.search(rf"\b{n}\(", header), n
    for method in ("modularity", "louvain_sweep", "louvain_aggregate", "louvain"):
        assert callable(getattr(ops.Session, method))
    est = sapca.Louvain()
    assert callable(est.fit_predict) and est.labels_ is None and est.modularity_ is None and est.n_communities_ is None and est.n_levels_ is None
    assert (est.resolution, est.tol, est.max_sweeps, est.max_levels, est.n_neighbors, est.seed) == (1.0, 1e-7, 256, None, 15, 42)
    hpp = open(os.path.join(ROOT, "single-algebra_amd", "host", "cpp", "sapca.hpp")).read()
    assert "louvain_device" in hpp and "LouvainOptions" in hpp
    rust = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca", "src", "lib.rs")).read()
    assert "pub mod louvain" in rust and "pub struct LouvainConfig" in rust
    mod = rust[rust.index("pub mod louvain"):]
    assert "pub fn run_f32" in mod and "pub fn run_f64" in mod
    sys_rs = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca-sys", "src", "lib.rs")).read()
    assert "pub struct sapca_louvain_options" in sys_rs and "pub fn sapca_louvain_device_f32" in sys_rs


def test_host_side_argument_checks_need_no_device():
    s = ops.Session.borrow(None)               # no handle: everything below fails before one is needed
    with pytest.raises(ValueError, match="max_sweeps = 0"):
        s._louvain_options(1.0, 1e-7, 0, None, None)
    with pytest.raises(ValueError, match="max_levels = 65"):
        s._louvain_options(1.0, 1e-7, 256, 65, None)
    with pytest.raises(ValueError, match="resolution"):
        s._louvain_options(float("nan"), 1e-7, 256, None, None)
    with pytest.raises(ValueError, match="tol"):
        s._louvain_options(1.0, -1.0, 256, None, None)
    with pytest.raises(ValueError, match="square ResidentCsr"):
        ops.Session.modularity(s, np.zeros((3, 3)), np.zeros(3, dtype=np.int32))
    o = s._louvain_options(2.0, 1e-6, 100, 3, 7)
    assert (o.resolution, o.tol, o.max_sweeps, o.max_levels, o.random_seed) == (2.0, 1e-6, 100, 3, 7)


# ------------------------------------------------------------------ 7. the golden file
def test_fixture_is_what_the_generator_writes(gold, built):
    assert sorted(gold) == sorted(built)
    for key, want in built.items():
        got = gold[key]
        assert got.dtype == np.asarray(want).dtype and got.shape == np.asarray(want).shape, key
        if key.endswith(("_nx_lo", "_nx_hi", "_Q", "_level_Q", "_margin_gain", "_margin_q", "_data")):
            assert np.allclose(got, want, rtol=0, atol=1e-12), key
        else:
            assert np.array_equal(got, want), key

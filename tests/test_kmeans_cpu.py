"""K-means without a GPU: the numpy restatement (tests/kmeans_ref.py) against scikit-learn's own KMeans as recorded in
tests/golden/g9_kmeans.npz (tests/golden/make_golden_kmeans.py), the seeding's uniforms and edge rules, the options struct
against the header, the exports and the bindings' host-side checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import kmeans_ref as KR
import sapca
from sapca import _lib as L
from sapca import ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g9_kmeans.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.mark.parametrize("tname,tol", [("tol0", 0.0), ("tol1e4", 1e-4)])
@pytest.mark.parametrize("name", ["a600", "b900"])
def test_restatement_equals_scikit_learn(gold, name, tname, tol):
    X, init = gold[f"{name}_X"], gold[f"{name}_init"]
    k = init.shape[0]
    want_labels, want_centers = gold[f"{name}_{tname}_labels"], gold[f"{name}_{tname}_centers"]
    assert np.bincount(want_labels, minlength=k).min() > 0          # no empty cluster: the one place where the two rules differ
    got = KR.lloyd(X, init, 300, tol)
    assert got["min_margin"] > 1e-10                                # no assignment hangs on the order of a sum
    assert got["n_iter"] == int(gold[f"{name}_{tname}_n_iter"])
    np.testing.assert_array_equal(got["labels"], want_labels)
    assert np.abs(got["centroids"] - want_centers).max() <= 1e-12 * np.abs(want_centers).max()
    assert abs(got["inertia"] - float(gold[f"{name}_{tname}_inertia"])) <= 1e-12 * got["inertia"]


def test_uniforms_are_the_librarys_counter_generator():
    for seed in (0, 1, 42, 2 ** 32 - 1):
        want = synth.hash_u01(seed, KR.STREAM, torch.arange(40, dtype=torch.int64)).numpy()
        np.testing.assert_array_equal(KR.uniforms(seed, 40), want)
    assert KR.STREAM == 21


def test_seeding_first_row_and_zero_total_fallback():
    X, _ = KR.blobs(500, 6, 4, 0.5, 2)
    for seed in (1, 7, 42):
        u = KR.uniforms(seed, 6)
        rows, boundary = KR.seed(X, 6, seed)
        assert rows[0] == int(np.floor(u[0] * 500)) and np.isinf(boundary[0])
        assert len(set(rows.tolist())) == 6 and np.isfinite(boundary[1:]).all()
        # c_t is the first row whose prefix sum passes u_t S: restated with a running sum
        D = np.min([KR.dist2(X, X[r]) for r in rows[:5]], axis=0)
        run, thr = 0.0, u[5] * np.cumsum(D)[-1]
        for i in range(500):
            run += D[i]
            if run > thr:
                break
        assert rows[5] == i
        same = np.tile(X[3], (50, 1))                                # every row coincides with the first centre: S = 0
        rows, boundary = KR.seed(same, 4, seed)
        np.testing.assert_array_equal(rows, np.floor(KR.uniforms(seed, 4) * 50).astype(np.int64))
        assert np.isinf(boundary).all()


def test_assign_breaks_ties_to_the_lower_index_and_update_keeps_an_empty_cluster():
    X, Cn = KR.integer_case(200, 5, 9, 3)
    labels, d2, margin = KR.assign(X, Cn)
    dup = [c for c in range(1, 9) if any((Cn[c] == Cn[b]).all() for b in range(c))]
    assert dup and not np.isin(labels, dup).any() and (margin == 0).any()
    assert (d2 == ((X - Cn[labels]) ** 2).sum(axis=1)).all()
    lab = labels.copy()
    lab[lab == labels[0]] = -1                                       # a cluster loses its rows to a label outside [0, k)
    new, counts = KR.update(X, lab, Cn)
    assert counts[labels[0]] == 0 and (new[labels[0]] == Cn[labels[0]]).all() and counts.sum() == (lab >= 0).sum()


def _header_struct():
    text = open(os.path.join(ROOT, "include", "sapca.h")).read()
    body = re.search(r"typedef struct sapca_kmeans_options \{(.*?)\} sapca_kmeans_options;", text, re.S).group(1)
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
    assert [(n, ctypes_of[t]) for n, t in _header_struct()] == list(L.KmeansOptions._fields_)
    o = L.default_kmeans_options()
    assert o.struct_size == C.sizeof(L.KmeansOptions) == 32
    got = {n: getattr(o, n) for n, _ in L.KmeansOptions._fields_}
    assert got == dict(struct_size=32, random_seed=42, n_clusters=8, init=L.KMEANS_PLUSPLUS, max_iter=300, tol=1e-4)
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    assert re.search(r"SAPCA_KMEANS_PLUSPLUS = 0, SAPCA_KMEANS_GIVEN = 1", header)
    assert int(re.search(r"#define SAPCA_KMEANS_MAX_CLUSTERS (\d+)", header).group(1)) == L.KMEANS_MAX_CLUSTERS == 1024


def test_bindings_are_present_and_the_abi_version_stays():
    lib = L.load()
    names = ["sapca_kmeans_options_default"] + [f"{n}_{s}" for s in ("f32", "f64") for n in (
        "sapca_kmeans_seed_device", "sapca_kmeans_assign_device", "sapca_kmeans_update_device", "sapca_kmeans_device", "sapca_kmeans")]
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    for n in names:
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n) and re.search(rf"\b{n}\(", header), n
    assert lib.sapca_abi_version() == 4 and re.search(r"#define SAPCA_ABI_VERSION 4\b", header)
    for method in ("kmeans_seed", "kmeans_assign", "kmeans_update", "kmeans"):
        assert callable(getattr(ops.Session, method))
    km = sapca.KMeans(n_clusters=3)
    assert callable(km.fit) and callable(km.fit_predict) and callable(km.predict) and km.labels_ is None
    hpp = open(os.path.join(ROOT, "single-algebra_amd", "host", "cpp", "sapca.hpp")).read()
    assert "kmeans_device" in hpp and "KmeansOptions" in hpp
    rust = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca", "src", "lib.rs")).read()
    assert "pub mod kmeans" in rust and "pub struct KMeansConfig" in rust


def test_host_side_argument_checks_need_no_device():
    s = ops.Session.borrow(None)               # no handle: everything below fails before one is needed
    X = torch.zeros((10, 4), dtype=torch.float32)
    for k, message in ((0, "n_clusters must be at least 1"), (1025, "n_clusters = 1025 exceeds the 1024"),
                       (11, "n_clusters = 11 exceeds the 10 rows")):
        with pytest.raises(ValueError, match=message):
            s.kmeans(X, n_clusters=k)
        with pytest.raises(ValueError, match=message):
            s.kmeans_seed(X, k)
    with pytest.raises(ValueError, match="must live on the device"):
        s.kmeans(X, n_clusters=2)
    with pytest.raises(ValueError, match="unknown init 'random'"):
        s.kmeans(X, n_clusters=2, init="random")
    with pytest.raises(ValueError, match="tol must be finite and not negative"):
        s.kmeans(X, n_clusters=2, tol=-1.0)
    with pytest.raises(ValueError, match="max_iter must not be negative"):
        s.kmeans(X, n_clusters=2, max_iter=-1)
    with pytest.raises(ValueError, match="float32 or float64"):
        s.kmeans(X.to(torch.int32), n_clusters=2)
    with pytest.raises(ValueError, match="two-dimensional float32 / float64"):
        s.kmeans(np.zeros((4, 3), dtype=np.int32), n_clusters=2)
    with pytest.raises(ValueError, match="init must have shape"):
        s.kmeans(np.zeros((40, 3)), n_clusters=2, init=np.zeros((3, 3)))
    with pytest.raises(ValueError, match=r"X has 1025 columns; 1 \.\. 1024"):
        s.kmeans(np.zeros((4, 1025)), n_clusters=2)
    with pytest.raises(ValueError, match=r"X has 0 columns; 1 \.\. 1024"):
        s.kmeans(np.zeros((4, 0)), n_clusters=2)
    with pytest.raises(ValueError, match="centroids must be a two-dimensional"):
        s.kmeans_assign(X, np.zeros((2, 4)))
    with pytest.raises(ValueError, match=r"has 1025 columns; 1 \.\. 1024"):
        s.kmeans_assign(torch.zeros((3, 1025)), torch.zeros((2, 1025)))
    with pytest.raises(RuntimeError, match="fit first"):
        sapca.KMeans(n_clusters=2).predict(X)

"""CPU tests of the neighbour search's host side: the numpy reference of the GPU tests (tests/knn_ref.py) against scipy's
cKDTree and scikit-learn's NearestNeighbors and against a literal transcription of the reference's similarity loops
(src/similarity/mod.rs), the declarations of sapca_knn_device_* in include/sapca.h, and the refusals of Session.knn that
need no device.  The sys crate and the C++ mirror are held to the header by tests/test_abi_cpu.py."""
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import knn_ref as KR
import sapca
from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clusters(rows, d, seed, n_clusters=5):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (n_clusters, d))
    return centres[rng.integers(0, n_clusters, rows)] + rng.normal(0.0, 1.0, (rows, d))


# ------------------------------------------------------------------ the reference against other implementations
def test_euclidean_reference_agrees_with_ckdtree():
    ckd = pytest.importorskip("scipy.spatial").cKDTree
    Q, Cm = _clusters(70, 6, 1), _clusters(300, 6, 2)
    idx, val = KR.knn(Q, Cm, 12, "euclidean")
    dist, want = ckd(Cm).query(Q, k=12)
    np.testing.assert_array_equal(idx, want)                      # continuous data: no ties
    np.testing.assert_allclose(val, dist, rtol=1e-13)
    idx, val = KR.knn(Cm, Cm, 9, "euclidean", exclude_self=True)
    dist, want = ckd(Cm).query(Cm, k=10)
    np.testing.assert_array_equal(want[:, 0], np.arange(300))     # a point's nearest is itself ...
    np.testing.assert_array_equal(idx, want[:, 1:])               # ... and the reference leaves exactly that one out
    np.testing.assert_allclose(val, dist[:, 1:], rtol=1e-13)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_reference_agrees_with_sklearn(metric):
    nn = pytest.importorskip("sklearn.neighbors").NearestNeighbors
    Q, Cm = _clusters(50, 8, 3), _clusters(200, 8, 4)
    idx, val = KR.knn(Q, Cm, 7, metric)
    dist, want = nn(n_neighbors=7, algorithm="brute", metric=metric).fit(Cm).kneighbors(Q)
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_allclose(val if metric == "euclidean" else 1.0 - val, dist, rtol=1e-9, atol=1e-12)


def _literal_cosine(a, b, T):
    """CosineSimilarity::calculate, src/similarity/mod.rs:14-36, in T"""
    dot, na, nb = T(0), T(0), T(0)
    for i in range(len(a)):
        dot = dot + a[i] * b[i]
        na = na + a[i] * a[i]
        nb = nb + b[i] * b[i]
    prod = np.sqrt(na * nb)
    return float(dot / prod) if prod > np.finfo(T).eps else 0.0


def _literal_pearson(a, b, T):
    """PearsonSimilarity::calculate, src/similarity/mod.rs:69-101, in T"""
    n = T(len(a))
    sa, sb, sab, saa, sbb = T(0), T(0), T(0), T(0), T(0)
    for i in range(len(a)):
        sa = sa + a[i]
        sb = sb + b[i]
        sab = sab + a[i] * b[i]
        saa = saa + a[i] * a[i]
        sbb = sbb + b[i] * b[i]
    num = sab - (sa * sb) / n
    den = np.sqrt((saa - (sa * sa) / n) * (sbb - (sb * sb) / n))
    return float(num / den) if den > np.finfo(T).eps else 0.0


@pytest.mark.parametrize("metric, literal", [("cosine", _literal_cosine), ("pearson", _literal_pearson)])
def test_similarity_values_agree_with_the_references_loops(metric, literal):
    Q, Cm = _clusters(9, 11, 5), _clusters(14, 11, 6)
    got = KR.pairwise(Q, Cm, metric)
    want = np.array([[literal(a, b, np.float64) for b in Cm] for a in Q])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)     # the raw-moment form cancels a little; values are O(1)
    Q32, C32 = Q.astype(np.float32), Cm.astype(np.float32)
    want32 = np.array([[literal(a, b, np.float32) for b in C32] for a in Q32])
    np.testing.assert_allclose(KR.pairwise(Q32, C32, metric, np.float32), want32, rtol=0, atol=2e-5)


def test_the_zero_row_rule_and_where_it_leaves_the_reference():
    Z = np.zeros((1, 5))
    X = _clusters(6, 5, 7)
    const = np.full((1, 5), 3.25)
    for T in (np.float32, np.float64):
        assert np.all(KR.pairwise(Z, X, "cosine", T) == 0) and np.all(KR.pairwise(X, Z, "cosine", T) == 0)
        assert np.all(KR.pairwise(const, X, "pearson", T) == 0)           # a constant row is the zero vector once centred
        assert np.all(KR.pairwise(const, X, "cosine", T) != 0)
    # the reference agrees on true zero rows (its norm product is 0) ...
    assert all(_literal_cosine(Z[0], b, np.float64) == 0.0 for b in X)
    assert all(_literal_pearson(const[0], b, np.float64) == 0.0 for b in X)
    # ... and differs only between the two thresholds: a row of norm 1e-5 is zero in f32 here (<= sqrt(eps) = 3.5e-4)
    # while the reference, which tests the PAIR's product against eps = 1.2e-7, still divides when the partner is long enough
    tiny = np.zeros((1, 5), np.float32)
    tiny[0, 0] = 1e-5
    big = np.zeros((1, 5), np.float32)
    big[0, 0] = 100.0
    assert KR.pairwise(tiny, big, "cosine", np.float32)[0, 0] == 0.0
    assert _literal_cosine(tiny[0], big[0], np.float32) == pytest.approx(1.0)
    assert KR.pairwise(tiny, big, "cosine", np.float64)[0, 0] == pytest.approx(1.0)   # f64: 1e-5 > sqrt(eps) = 1.5e-8


def test_ties_go_to_the_lower_index_and_self_is_excluded_by_index():
    Cm = np.array([[0.0, 0], [1, 0], [0, 1], [1, 0], [0, 0], [-1, 0]])   # rows 1 and 3, 0 and 4 are duplicates
    idx, val = KR.knn(Cm, Cm, 5, "euclidean", exclude_self=True)
    assert idx[0].tolist() == [4, 1, 2, 3, 5] and val[0].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0]
    assert idx[4].tolist() == [0, 1, 2, 3, 5]                             # the duplicate stays a neighbour at distance 0
    idx, _ = KR.knn(Cm, Cm, 6, "euclidean")
    assert idx[4].tolist() == [0, 4, 1, 2, 3, 5]                          # not excluded: 0 before 4 by index
    assert KR.is_sorted(idx, KR.pairwise(Cm, Cm, "euclidean")[np.arange(6)[:, None], idx], "euclidean")


# ------------------------------------------------------------------ the declarations
def test_the_header_declares_both_functions_and_the_constants():
    raw = open(os.path.join(ROOT, "include", "sapca.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    for suf, ct in (("f32", "float"), ("f64", "double")):
        m = re.search(r"sapca_status\s+sapca_knn_device_%s\s*\(([^()]*)\)\s*;" % suf, text)
        assert m, f"sapca_knn_device_{suf} is not declared"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == ["sapca_handle h", "uint64_t mq", f"const {ct}* d_queries", "uint64_t ldq", "uint64_t mc",
                        f"const {ct}* d_corpus", "uint64_t ldc", "uint64_t d", "int32_t metric", "uint32_t n_neighbors",
                        "uint32_t flags", "int32_t* d_indices", f"{ct}* d_values"]
    assert re.search(r"SAPCA_KNN_EUCLIDEAN\s*=\s*0\s*,\s*SAPCA_KNN_COSINE\s*=\s*1\s*,\s*SAPCA_KNN_PEARSON\s*=\s*2", text)
    assert re.search(r"#define\s+SAPCA_KNN_EXCLUDE_SELF\s+1u\b", text)
    assert re.search(r"#define\s+SAPCA_KNN_MAX_NEIGHBORS\s+128\b", text)
    assert re.search(r"#define\s+SAPCA_ABI_VERSION\s+4\b", text)
    assert "additive, ABI 4: sapca_knn_device_*" in raw


def test_the_library_exports_both_functions():
    for suf in ("f32", "f64"):
        assert f"sapca_knn_device_{suf}" in L.EXPORTED_SYMBOLS
        assert hasattr(L.load(), f"sapca_knn_device_{suf}")
    assert (L.KNN_EUCLIDEAN, L.KNN_COSINE, L.KNN_PEARSON) == (0, 1, 2)
    assert L.KNN_EXCLUDE_SELF == 1 and L.KNN_MAX_NEIGHBORS == 128
    assert sapca.KNN_METRICS == {"euclidean": 0, "cosine": 1, "pearson": 2}


# ------------------------------------------------------------------ Session.knn refuses before it touches a device
class _NoDevice:
    """a Session-shaped object without a handle: whatever reaches the library fails loudly (a null handle is SAPCA_ERR_ARG)"""
    _h = None
    knn = ops.Session.knn


def test_session_knn_is_exported():
    assert sapca.Session is ops.Session and callable(ops.Session.knn)


def test_session_knn_refuses_bad_arguments_on_the_host():
    s = _NoDevice()
    q = torch.zeros((10, 4), dtype=torch.float32)
    c = torch.zeros((20, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="unknown metric 'manhattan'"):
        s.knn(q, c, 3, metric="manhattan")
    with pytest.raises(ValueError, match="unknown metric 7"):
        s.knn(q, c, 3, metric=7)
    with pytest.raises(ValueError, match="n_neighbors must be at least 1, got 0"):
        s.knn(q, c, 0)
    with pytest.raises(ValueError, match="n_neighbors = 129 exceeds the 128"):
        s.knn(q, torch.zeros((500, 4)), 129)
    with pytest.raises(ValueError, match=r"n_neighbors = 21 exceeds the 20 corpus rows"):
        s.knn(q, c, 21)
    with pytest.raises(ValueError, match=r"n_neighbors = 10 exceeds the 9 corpus rows .*itself excluded"):
        s.knn(q, None, 10)                                         # corpus None: self-search, a row's own index left out
    with pytest.raises(ValueError, match="queries have 4 columns, the corpus 5"):
        s.knn(q, torch.zeros((20, 5)), 3)
    with pytest.raises(ValueError, match="must share dtype and device"):
        s.knn(q, c.double(), 3)
    with pytest.raises(ValueError, match="queries must be two-dimensional"):
        s.knn(q[0], c, 3)
    with pytest.raises(ValueError, match="corpus must be float32 or float64"):
        s.knn(q, c.half(), 3)
    with pytest.raises(ValueError, match=r"queries: the elements of a row must be contiguous \(stride\(1\) == 1\)"):
        s.knn(torch.zeros((4, 10)).t(), c, 3)
    with pytest.raises(ValueError, match="queries must be a torch tensor"):
        s.knn(np.zeros((10, 4), np.float32), c, 3)
    with pytest.raises(ValueError, match="1 .. 1024 are supported"):
        s.knn(torch.zeros((3, 1025)), torch.zeros((5, 1025)), 2)
    # everything else in order: only now does the device matter (a column slice of a wider buffer is a legal panel)
    wide = torch.zeros((20, 9))
    with pytest.raises(ValueError, match="queries must live on the device"):
        s.knn(wide[:10, 2:6], wide[:, 2:6], 3, metric="pearson", exclude_self=True)


def test_panel_geometry():
    wide = torch.zeros((20, 9), dtype=torch.float64)
    assert ops._knn_panel("x", wide[:, 2:6]) == (20, 4, 9, torch.float64)
    assert ops._knn_panel("x", wide) == (20, 9, 9, torch.float64)
    assert ops._knn_panel("x", wide[::2, :3]) == (10, 3, 18, torch.float64)
    assert ops._knn_panel("x", wide[:1, :5]) == (1, 5, 5, torch.float64)       # one row: the stride does not matter
    assert ops._knn_panel("x", wide[:, 4:5]) == (20, 1, 9, torch.float64)      # one column
    assert ops._knn_panel("x", wide[:0]) == (0, 9, 9, torch.float64)

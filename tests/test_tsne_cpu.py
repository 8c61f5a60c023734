"""t-SNE without a GPU: the numpy restatement (tests/tsne_ref.py) against scikit-learn's own gradient and Kullback-Leibler
divergence as recorded in tests/golden/g8_tsne.npz (tests/golden/make_golden_tsne.py), the properties the GPU tests rely
on, the options struct against the header, and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import knn_ref as KR
import tsne_ref as TR
import sapca
from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g8_tsne.npz")


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    m = g["X"].shape[0]
    g["P"] = sp.csr_matrix((g["P_data"], g["P_indices"], g["P_indptr"]), shape=(m, m))
    return g


def test_fixture_is_what_the_restatement_computes(gold):
    X, perp = gold["X"], float(gold["perplexity"])
    K = TR.neighbours_of(perp)
    assert K == gold["indices"].shape[1] == 30
    idx, dist = KR.knn(X, X, K, "euclidean", exclude_self=True)
    np.testing.assert_array_equal(idx, gold["indices"])
    np.testing.assert_array_equal(dist, gold["dist"])
    p, beta = TR.conditional(idx, dist, perp)
    np.testing.assert_array_equal(beta, gold["beta"])
    P = TR.symmetrise(idx, p)
    np.testing.assert_array_equal(P.indptr, gold["P_indptr"])
    np.testing.assert_array_equal(P.indices, gold["P_indices"])
    np.testing.assert_array_equal(P.data, gold["P_data"])


def test_affinities_have_the_stated_properties(gold):
    idx, dist, perp, P = gold["indices"], gold["dist"], float(gold["perplexity"]), gold["P"]
    m, K = idx.shape
    ok = np.ones(K, dtype=bool)
    gaps = [TR.entropy_gap(dist[i] ** 2, ok, gold["beta"][i], perp)[0] for i in range(m)]
    assert np.abs(gaps).max() < 1e-5                                    # the search's own stopping rule
    assert abs(P.sum() - 1.0) < 1e-12                                    # conditional rows sum to 1: dividing by 2 m is dividing by the total
    assert (P != P.T).nnz == 0                                           # symmetric bit for bit
    assert P.has_canonical_format
    listed = sp.csr_matrix((np.ones(m * K), (np.repeat(np.arange(m), K), idx.ravel())), shape=(m, m))
    mutual = listed.multiply(listed.T).nnz
    assert 0 < mutual < listed.nnz                                       # mutual and one-sided neighbours both occur
    assert P.nnz == 2 * listed.nnz - mutual


@pytest.mark.parametrize("name", ["Y0", "Y1"])
@pytest.mark.parametrize("e", [1, 12])
def test_gradient_and_kl_equal_scikit_learns(gold, name, e):
    g, Z, kl = TR.gradient(gold["P"], gold[name], float(e))
    want = gold[f"sk_grad_{name}_e{e}"]
    # scikit-learn's gradient / 4 is the same expression summed in another order: a few ulp of the largest term
    assert np.abs(g - want).max() <= 64 * np.finfo(np.float64).eps * np.abs(want).max()
    assert abs(kl - float(gold[f"sk_kl_{name}"])) <= 1e-13 * abs(kl)
    gr = TR.gradient(gold["P"], gold[name], float(e), reverse=True)[0]
    assert np.abs(g - gr).max() <= 64 * np.finfo(np.float64).eps * np.abs(want).max()


def test_the_f32_restatement_stays_near_the_f64_one(gold):
    g64, Z64, _ = TR.gradient(gold["P"], gold["Y1"].astype(np.float32), 1.0)
    g32, Z32, _ = TR.gradient(gold["P"], gold["Y1"].astype(np.float32), 1.0, arith=np.float32)
    assert abs(Z32 - Z64) <= 1e-5 * Z64
    assert np.abs(g32 - g64).max() <= 1e-4 * np.abs(g64).max()


def test_trajectory_fixture(gold):
    Y, kl = TR.embed(gold["P"], gold["Y0"], int(gold["epochs"]))
    np.testing.assert_array_equal(Y, gold["Y20"])
    assert kl == float(gold["kl20"])
    Yr, _, gains_r = TR.embed(gold["P"], gold["Y0"], int(gold["epochs"]), reverse=True, return_gains=True)
    assert np.array_equal(gains_r, TR.embed(gold["P"], gold["Y0"], int(gold["epochs"]), return_gains=True)[2])
    assert np.abs(Yr - Y).max() < 1e-6 * np.abs(Y).max()
    assert np.abs(Y.mean(axis=0)).max() <= 1e-12 * np.abs(Y).max()


def test_the_restatement_separates_clusters():
    X, labels = TR.clusters(600, 10, 3)
    perp = 20.0
    idx, dist = KR.knn(X, X, TR.neighbours_of(perp), "euclidean", exclude_self=True)
    P = TR.symmetrise(idx, TR.conditional(idx, dist, perp)[0])
    Y0 = 1e-4 * np.random.default_rng(0).normal(size=(600, 2))
    kl0 = TR.embed(P, Y0, 0)[1]
    Y, kl = TR.embed(P, Y0, 300)
    assert np.isfinite(kl) and kl < kl0
    nn = KR.knn(Y, Y, 1, "euclidean", exclude_self=True)[0][:, 0]
    assert (labels[nn] == labels).mean() >= 0.99


def test_double_double_exp_is_correctly_rounded(tmp_path):
    """csrc/exp_rn.h, compiled for the host, against 50-digit arithmetic (tests/tsne_ref.exp_exact): over the arguments the
    affinities meet (0 .. -60), a log-uniform sweep down to the underflow of the result, and the edges."""
    import shutil
    import subprocess
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler (the build needs one)"
    src = tmp_path / "exp_rn_main.cpp"
    src.write_text('#include <cstdio>\n#include "%s"\nint main() { double x; while (std::scanf("%%lf", &x) == 1) '
                   'std::printf("%%.17g\\n", sapca::k::exp_rn(x)); return 0; }\n'
                   % os.path.join(ROOT, "single-algebra_amd", "csrc", "exp_rn.h"))
    exe = tmp_path / "exp_rn_main"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", str(exe), str(src)], check=True)
    rng = np.random.default_rng(0)
    x = -np.concatenate([rng.uniform(0, 60, 12000), 10 ** rng.uniform(-9, np.log10(700.0), 8000), [0.0, 1e-300, 0.5, 1.0, 700.0]])
    out = subprocess.run([str(exe)], input="\n".join(repr(float(v)) for v in x), capture_output=True, text=True, check=True).stdout.split()
    got = np.array([float(o) for o in out])
    want = np.array([TR.exp_exact(float(v)) for v in x])
    assert got.shape == want.shape and (got == want).all(), f"{(got != want).sum()} of {len(x)} differ"
    deep = subprocess.run([str(exe)], input="-745.0 -746.0 -1e9", capture_output=True, text=True, check=True).stdout.split()
    assert [float(v) for v in deep] == [5e-324, 0.0, 0.0]


def _header_struct():
    text = open(os.path.join(ROOT, "include", "sapca.h")).read()
    body = re.search(r"typedef struct sapca_tsne_options \{(.*?)\} sapca_tsne_options;", text, re.S).group(1)
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
    assert [(n, ctypes_of[t]) for n, t in _header_struct()] == list(L.TsneOptions._fields_)
    o = L.default_tsne_options()
    assert o.struct_size == C.sizeof(L.TsneOptions) == 88
    got = {n: getattr(o, n) for n, _ in L.TsneOptions._fields_}
    assert got == dict(struct_size=88, random_seed=42, output_dim=2, init_given=0, perplexity=20.0, theta=0.5, epochs=1000,
                       stop_lying_epoch=250, momentum_switch_epoch=250, exaggeration=12.0, learning_rate=200.0, momentum=0.5,
                       final_momentum=0.8)
    assert {k: got[k] for k in TR.DEFAULTS} == TR.DEFAULTS


def test_bindings_are_present():
    lib = L.load()
    names = ["sapca_tsne_options_default"] + [f"{n}_{s}" for s in ("f32", "f64") for n in (
        "sapca_tsne_affinities_device", "sapca_tsne_gradient_device", "sapca_tsne_embed_device", "sapca_tsne_device", "sapca_tsne")]
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    for n in names:
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n) and re.search(rf"\b{n}\(", header), n
    for method in ("tsne_affinities", "tsne_gradient", "tsne_embed", "tsne"):
        assert callable(getattr(ops.Session, method))
    assert callable(sapca.TSNE(perplexity=5).fit_transform)
    hpp = open(os.path.join(ROOT, "single-algebra_amd", "host", "cpp", "sapca.hpp")).read()
    assert "tsne_device" in hpp and "TsneOptions" in hpp
    rust = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca", "src", "lib.rs")).read()
    assert "pub mod tsne" in rust and "pub struct TSNEConfig" in rust and "pub fn run_f32" in rust and "pub fn run_f64" in rust


def test_host_side_argument_checks_need_no_device():
    s = ops.Session.borrow(None)               # no handle: everything below fails before one is needed
    with pytest.raises(ValueError, match="unknown t-SNE constant"):
        s._tsne_options(20.0, 10, 2, False, 1, dict(learning_rat=3.0))
    with pytest.raises(ValueError, match="two-dimensional float32 / float64"):
        ops.Session.tsne(s, np.zeros((4, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="init must have shape"):
        ops.Session.tsne(s, np.zeros((40, 3)), perplexity=5, init=np.zeros((40, 3)))

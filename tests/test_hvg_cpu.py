"""CPU tests of the variable-genes operators (sapca_hvg_moments_csr_device_*, sapca_loess_f64, sapca_hvg_csr_device_*): the numpy
restatement tests/hvg_ref.py against independent code -- pandas.cut for the bins, numpy.polyfit for the local regression, a
dense two-line version of the clipped variance, a hand-made table for the rank combination -- the boundary (symbols in the
header, the Python binding and sapca-sys, the options struct, the C++ mirror) and the golden fixture."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import hvg_ref as R
from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
M, N, K = 240, 90, 3


def _dense(ptr, idx, val, m, n):
    D = np.zeros((m, n), dtype=np.float64)
    for i in range(m):
        D[i, idx[ptr[i]:ptr[i + 1]]] = val[ptr[i]:ptr[i + 1]]
    return D


@pytest.fixture(scope="module")
def case():
    ptr, idx, val = R.fixture(M, N, 141, np.float32)
    return ptr, idx, val, R.batch_labels(M, K, 142), _dense(ptr, idx, val, M, N)


def test_fixture_holds_the_edge_cases(case):
    ptr, idx, val, labels, D = case
    assert (np.diff(ptr) == 0).any()                                   # an empty row
    assert (val == 0).any()                                            # stored zeros
    stored = np.bincount(idx, minlength=N)
    assert (stored == 0).sum() == 5                                    # never-stored columns
    rows = np.diff(ptr) > 0
    assert (D[rows][:, 3] == 3).all()                                  # a constant column
    assert (labels == -1).any() and (labels == K).any()                # excluded rows, both sides
    assert (D[:, N - 2] == D[:, N - 3]).all()                          # identical columns


@pytest.mark.parametrize("kind", ["spread", "flat", "flat0", "ties"])
@pytest.mark.parametrize("n_bins", [1, 7, 20])
def test_bins_equal_pandas_cut(kind, n_bins):
    rng = np.random.default_rng(5)
    x = {"spread": rng.gamma(2.0, 1.0, 300), "flat": np.full(40, 2.5), "flat0": np.zeros(9),
         "ties": np.round(rng.gamma(2.0, 1.0, 300), 1)}[kind]
    want = pd.cut(x, bins=n_bins, labels=False)
    got = R.cut_bins(x, n_bins)
    assert np.array_equal(got, want)
    edges = pd.cut(x, bins=n_bins, retbins=True)[1]
    assert np.array_equal(R.cut_edges(x, n_bins), edges)


def test_loess_equals_weighted_polyfit_at_sampled_points():
    rng = np.random.default_rng(9)
    x = np.sort(rng.normal(0.0, 1.0, 400))
    y = np.sin(x) + rng.normal(0.0, 0.2, x.size)
    span = 0.3
    q = R.loess_window(span, x.size)
    at = [0, 1, 57, 200, 398, 399]
    got = R.loess(x, y, span, at=at)
    for g, i in zip(got, at):
        d = np.abs(x - x[i])
        h = np.sort(d)[q - 1]
        w = np.where(d < h, (1 - (d / h) ** 3) ** 3, 0.0)
        keep = w > 0
        coef = np.polyfit((x[keep] - x[i]) / h, y[keep], 2, w=np.sqrt(w[keep]))   # polyfit weights multiply the residuals
        assert abs(g - coef[2]) <= 1e-9 * max(1.0, abs(coef[2])), (i, g, coef[2])
    assert q == 120 and R.loess_window(0.3, 5) == 3 and R.loess_window(1.0, 4) == 4 and R.loess_window(0.3, 2) == 2


def test_loess_degenerate_branches():
    # h == 0: more than q points share x_i -> the mean over ALL of them; two distinct abscissae -> the weighted line
    x = np.array([0.0] * 6 + [1.0, 2.0, 3.0, 4.0])
    y = np.arange(10, dtype=np.float64)
    fit = R.loess(x, y, 0.5)          # q = 5
    assert np.allclose(fit[:6], y[:6].mean(), rtol=0, atol=1e-15)
    x2 = np.array([0.0, 0.0, 1.0, 1.0, 5.0, 9.0])
    y2 = np.array([1.0, 3.0, 4.0, 6.0, 0.0, 0.0])
    fit2 = R.loess(x2, y2, 0.7)       # q = 4: at x = 0 the window is {0, 0, 1, 1}, h = 1, only x = 0 is weighted -> mean 2
    assert fit2[0] == 2.0 and fit2[1] == 2.0
    x3 = np.array([0.0, 0.0, 1.0, 1.0, 3.0, 9.0])
    fit3 = R.loess(x3, y2, 0.85)      # q = 5: at x = 0, h = 3, weighted abscissae {0, 1}: the line through the means -> 2
    assert abs(fit3[0] - 2.0) < 1e-12
    assert np.array_equal(R.loess(np.full(7, 2.0), y[:7], 0.3), np.full(7, 3.0))   # all-equal x
    assert R.loess(np.zeros(0), np.zeros(0), 0.3).size == 0


def test_clipped_variance_equals_the_dense_two_liner(case):
    ptr, idx, val, labels, D = case
    cols = R.columns(ptr, idx, val, M, N)
    for mask in (R.included_rows(M), R.included_rows(M, labels, 1, K)):
        b = R.seurat_v3_batch(cols, mask, 0.3)
        X = D[mask]
        Nb = X.shape[0]
        assert np.allclose(b["mean"], X.mean(axis=0), rtol=1e-13, atol=0)
        assert np.allclose(b["var"], X.var(axis=0, ddof=1), rtol=1e-11, atol=1e-15)
        Xc = np.minimum(X, b["clip"][None, :])
        want = ((Xc - b["mean"][None, :]) ** 2).sum(axis=0) / ((Nb - 1) * b["reg_std"] ** 2)
        assert np.allclose(b["norm_var"], want, rtol=1e-11, atol=1e-14)
        assert np.array_equal(b["n_clipped"], (X > b["clip"][None, :]).sum(axis=0))
        small = R.columns(ptr, idx, val * np.float32(0.01), M, N)   # (expm1 of the counts themselves overflows)
        Xs = X.astype(np.float32) * np.float32(0.01)
        s, q, c = R.moments(small, mask, R.EXPM1)
        E = np.where(X != 0, np.expm1(Xs.astype(np.float64)), 0.0)
        assert np.allclose(s, E.sum(axis=0), rtol=1e-13) and np.allclose(q, (E ** 2).sum(axis=0), rtol=1e-13)
        assert not c.any()


def test_rank_combination_on_a_hand_made_table():
    nan = np.nan
    #            col: 0    1    2    3    4    5    6
    nv = np.array([[9.0, 7.0, 7.0, 1.0, nan, 3.0, 2.0],
                   [1.0, 8.0, 8.0, 9.0, 5.0, nan, 2.0],
                   [4.0, 4.0, 6.0, 5.0, nan, nan, 7.0]])
    rank, nhv, vnorm, hv = R.combine_v3(nv, 3)
    # batch ranks (ties to the lower index, NaN last):  b0: 0 > 1 = 2 -> 0, 1, 2;  b1: 3 > 1 = 2 -> 3:0, 1:1, 2:2;  b2: 6:0, 2:1, 3:2
    want_ranks = np.array([[0, 1, 2, nan, nan, nan, nan], [nan, 1, 2, 0, nan, nan, nan], [nan, nan, 1, 2, nan, nan, 0]])
    assert np.array_equal(np.stack([R.rank_desc(r, 3) for r in nv]), want_ranks, equal_nan=True)
    assert np.array_equal(rank, [0.0, 1.0, 2.0, 1.0, nan, nan, 0.0], equal_nan=True)
    assert np.array_equal(nhv, [1, 2, 3, 2, 0, 0, 1])
    # (rank asc, n_batches desc, index): 0 (0, 1), 6 (0, 1), 1 (1, 2), 3 (1, 2), 2 (2, 3), then the unranked
    assert np.array_equal(hv, [1, 1, 0, 0, 0, 0, 1])
    # n_top = 5: ranks {0, 3}, {1, 1, 4}, {2, 2, 1}, {0, 2}, {3}, {3}, {4, 4, 0} -> medians 1.5, 1, 2, 1, 3, 3, 4 in 2, 3, 3, 2, 1, 1, 3
    # batches: 1 (1, 3), 3 (1, 2), 0, 2, then 4 before 5 by index
    rank5, nhv5, _, hv5 = R.combine_v3(nv, 5)
    assert np.array_equal(rank5, [1.5, 1.0, 2.0, 1.0, 3.0, 3.0, 4.0]) and np.array_equal(nhv5, [2, 3, 3, 2, 1, 1, 3])
    assert np.array_equal(hv5, [1, 1, 1, 1, 1, 0, 0])
    assert np.isnan(vnorm[4]) and vnorm[0] == (9.0 + 1.0 + 4.0) / 3
    df = pd.DataFrame({"rank": rank, "nb": nhv})   # scanpy's own final sort
    order = df.sort_values(["rank", "nb"], ascending=[True, False], na_position="last", kind="stable").index.to_numpy()
    assert set(order[:3]) == set(np.nonzero(hv)[0])


def test_seurat_bins_one_gene_and_zero_std():
    ptr, idx, val = R.fixture(1500, 700, 131, np.float32)
    x = R.log1p_normalized(ptr, val)
    r = R.hvg(ptr, idx, x, 1500, 700, flavor=R.SEURAT, n_top=100)
    b = r["batches"][0]
    assert (b["bin_count"] == 1).any() and ((b["bin_count"] >= 2) & (b["bin_std"] == 0)).any() and (b["bin_count"] == 0).any()
    one = np.nonzero(b["bin_count"] == 1)[0][0]
    j = np.nonzero((b["bins"] == one) & ~np.isnan(b["disp"]))[0][0]
    assert r["dispersions_norm"][j] == 1.0                 # (disp - 0) / disp
    assert r["highly_variable"].sum() >= 100 and np.isnan(r["rank"]).all()
    cut = R.hvg(ptr, idx, x, 1500, 700, flavor=R.SEURAT, n_top=0)
    want = R.within_cutoffs(cut["means"], cut["dispersions_norm"], *R.DEFAULT_CUTOFFS)
    assert np.array_equal(cut["highly_variable"], want.astype(np.uint8)) and 0 < want.sum() < 700


def test_symbols_in_header_library_bindings_and_sys_crate():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    sys_rs = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca-sys", "src", "lib.rs")).read()
    names = [f"{stem}_{suf}" for stem in ("sapca_hvg_moments_csr_device", "sapca_hvg_csr_device") for suf in ("f32", "f64")]
    for n in names + ["sapca_loess_f64", "sapca_hvg_options_default"]:
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n) and re.search(rf"\b{n}\(", header), n
        assert f"pub fn {n}(" in sys_rs, n
    assert "pub struct sapca_hvg_options {" in sys_rs
    for name, value in (("MAX_BATCHES", L.HVG_MAX_BATCHES), ("CLIP", L.HVG_CLIP), ("EXPM1", L.HVG_EXPM1),
                        ("SEURAT_V3", L.HVG_SEURAT_V3), ("SEURAT", L.HVG_SEURAT)):
        assert int(re.search(rf"#define SAPCA_HVG_{name} (\d+)", header).group(1)) == value
    assert (R.CLIP, R.EXPM1, R.SEURAT_V3, R.SEURAT, R.MAX_BATCHES) == (L.HVG_CLIP, L.HVG_EXPM1, L.HVG_SEURAT_V3, L.HVG_SEURAT,
                                                                       L.HVG_MAX_BATCHES)
    assert int(re.search(r"#define\s+SAPCA_ABI_VERSION\s+(\d+)", header).group(1)) == 4
    for method in ("highly_variable", "hvg_moments"):
        assert callable(getattr(ops.ResidentCsr, method))
    assert callable(ops.Session.loess)


def test_options_default_and_struct_layout():
    o = L.default_hvg_options()
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    assert o.struct_size == C.sizeof(L.HvgOptions) == int(re.search(r"sizeof\(sapca_hvg_options\): (\d+)", header).group(1))
    assert (o.flavor, o.n_top, o.span, o.n_bins) == (L.HVG_SEURAT_V3, 2000, 0.3, 20)
    assert (o.min_mean, o.max_mean, o.min_disp, o.max_disp) == R.DEFAULT_CUTOFFS


def test_python_argument_checks_come_before_the_library():
    X = ops.ResidentCsr(None, (4, 3), 0, np.float32, 0, 0, 0)
    with pytest.raises(ValueError, match="flavor"):
        X.highly_variable(2, flavor="cell_ranger")
    with pytest.raises(ValueError, match="transform"):
        X.hvg_moments("log")
    with pytest.raises(ValueError, match="clip must hold 3"):
        X.hvg_moments("clip", clip=np.zeros(4))
    with pytest.raises(ValueError, match="labels must be 4 integers"):
        X.highly_variable(2, batch=np.zeros(5, dtype=np.int32), n_batches=2)


def test_cpp_mirror_compiles_with_the_hvg_methods(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "m.cpp"
    src.write_text('#include "%s"\n'
                   'template <typename T> size_t use(const sapca::ResidentCsr<T>& x, const int32_t* d_batch, const double* clip) {\n'
                   '  typename sapca::ResidentCsr<T>::HvgOptions o;\n'
                   '  o.n_top = 10;\n'
                   '  auto a = x.hvg_moments(SAPCA_HVG_CLIP, clip, d_batch, 1);\n'
                   '  auto b = x.highly_variable(o, d_batch, 3);\n'
                   '  return a.n_clipped.size() + a.sum_squared.size() + b.highly_variable.size() + b.rank.size();\n'
                   '}\n'
                   'template size_t use<float>(const sapca::ResidentCsr<float>&, const int32_t*, const double*);\n'
                   'template size_t use<double>(const sapca::ResidentCsr<double>&, const int32_t*, const double*);\n'
                   'int main() { return 0; }\n' % os.path.join(ROOT, "single-algebra_amd", "host", "cpp", "sapca.hpp"))
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_golden_fixture_is_what_the_restatement_writes(golden):
    import make_golden_hvg as G
    g = golden("g13_hvg.npz")
    m, n, k = (int(x) for x in g["shape"])
    ptr, idx, val = R.fixture(m, n, G.SEED, np.float32)
    labels = R.batch_labels(m, k, G.SEED + 1)
    for name, a in (("ptr", ptr), ("idx", idx), ("val", val), ("labels", labels)):
        assert np.array_equal(g[name], a), name                      # the generator has not drifted
    r = R.hvg(ptr, idx, val, m, n, labels=labels, K=k, n_top=20)
    for key in ("rank", "n_batches_hv", "highly_variable"):
        assert np.array_equal(g[f"v3_k3_{key}"], r[key], equal_nan=True), key
    assert np.allclose(g["v3_k3_variances_norm"], r["variances_norm"], rtol=1e-11, atol=0)
    assert np.array_equal(g["v3_k3_n_clipped"], np.stack([b["n_clipped"] for b in r["batches"]]))
    one = R.hvg(ptr, idx, val, m, n, n_top=20)
    for key in ("rank", "n_batches_hv", "highly_variable"):
        assert np.array_equal(g[f"v3_one_{key}"], one[key], equal_nan=True), key
    for key in ("means", "variances", "variances_norm"):
        assert np.allclose(g[f"v3_one_{key}"], one[key], rtol=1e-11, atol=0), key
        assert np.allclose(g[f"v3_k3_{key}"], r[key], rtol=1e-11, atol=0), key
    assert np.allclose(g["v3_one_clip"][0], one["batches"][0]["clip"], rtol=1e-11, atol=0)
    assert np.allclose(g["v3_k3_clip"], np.stack([b["clip"] for b in r["batches"]]), rtol=1e-11, atol=0)
    assert np.array_equal(g["v3_one_n_clipped"][0], one["batches"][0]["n_clipped"])
    x = R.log1p_normalized(ptr, val)
    cut = R.hvg(ptr, idx, x, m, n, flavor=R.SEURAT, n_top=0)
    for tag, res in (("top", R.hvg(ptr, idx, x, m, n, flavor=R.SEURAT, n_top=15)), ("cut", cut)):
        for key in ("means", "dispersions", "dispersions_norm"):
            assert np.allclose(g[f"seurat_{tag}_{key}"], res[key], rtol=1e-11, atol=1e-13, equal_nan=True), (tag, key)
        assert np.array_equal(g[f"seurat_{tag}_highly_variable"], res["highly_variable"]), tag
    s = R.hvg(ptr, idx, x, m, n, flavor=R.SEURAT, n_top=15)
    assert np.allclose(g["seurat_top_dispersions_norm"], s["dispersions_norm"], rtol=1e-11, atol=0, equal_nan=True)
    assert np.array_equal(g["seurat_top_highly_variable"], s["highly_variable"])
    assert np.allclose(g["loess_fit"], R.loess(g["loess_x"], g["loess_y"], 0.3), rtol=1e-11, atol=1e-13)
    for mm, nn, seed in G.BIG:                                         # the GPU test's matrices are what they were
        p, i, v = R.fixture(mm, nn, seed, np.float32)
        assert int(g[f"big_{nn}_crc"][0]) == G.checksum(p, i, v), nn
        nv = R.hvg(p, i, v, mm, nn, n_top=100)["batches"][0]["norm_var"]
        assert np.allclose(g[f"big_{nn}_norm_var"], nv, rtol=1e-11, atol=0), nn   # ... and so is what the restatement makes of them

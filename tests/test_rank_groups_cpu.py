"""CPU tests of the rank-groups operator (sapca_rank_sums_csr_device_*, sapca_rank_groups_csr_device_*): the numpy restatement
tests/rank_groups_ref.py against scipy on dense columns, the boundary (symbols, argument checks, the length-class constants of
csrc/rankgroups.h, the C++ mirror), the host arithmetic of the Python result object, and the golden fixture."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.stats as st
import torch  # noqa: F401  (first: one HIP runtime per process)

import rank_groups_ref as R
from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N, K = 700, 40, 5


def _dense(ptr, idx, val, m, n):
    D = np.zeros((m, n), dtype=val.dtype)
    for i in range(m):
        D[i, idx[ptr[i]:ptr[i + 1]]] = val[ptr[i]:ptr[i + 1]]
    return D


@pytest.fixture(scope="module", params=["counts", "real"])
def case(request):
    dt = np.float32 if request.param == "counts" else np.float64
    ptr, idx, val, labels = R.fixture(M, N, K, 7 if request.param == "counts" else 8, dt, request.param)
    return ptr, idx, val, labels, _dense(ptr, idx, val, M, N), R.rank_sums(ptr, idx, val, M, N, labels, K)


def test_fixture_holds_the_edge_cases(case):
    ptr, idx, val, labels, D, exact = case
    assert exact["group_rows"][K - 1] == 0 and (exact["group_rows"][:K - 1] > 0).all()     # an empty group
    assert (labels == -1).any() and (labels == K).any()                                    # excluded rows, both sides
    assert (val < 0).any() and (val == 0).any() and np.signbit(val[val == 0]).any()        # negatives, stored zeros, -0.0
    assert not D[:, 0].any() and np.unique(D[:, 2]).size == M                              # all-zero and all-distinct columns


def test_rank_sums_equal_scipy_rankdata_on_dense_columns(case):
    ptr, idx, val, labels, D, exact = case
    inc = (labels >= 0) & (labels < K)
    for j in range(N):
        ranks = st.rankdata(D[inc, j])
        for g in range(K):
            assert exact["rank_sum2"][g, j] == int(np.rint(2.0 * ranks[labels[inc] == g].sum())), (g, j)
            assert exact["nonzero"][g, j] == np.count_nonzero(D[labels == g, j])
        t = np.unique(D[inc, j], return_counts=True)[1].astype(np.int64)
        assert exact["tie_sum"][j] == float((t ** 3 - t).sum())


def test_wilcoxon_against_scipy_mannwhitneyu(case):
    """scipy's asymptotic test always corrects for ties: tie_correct = 1.  U = R_g - n_g (n_g + 1) / 2 is exact; z and p to 1e-12"""
    ptr, idx, val, labels, D, exact = case
    inc = (labels >= 0) & (labels < K)
    z1, p1 = R.wilcoxon(exact["rank_sum2"], exact["group_rows"], exact["tie_sum"], True)
    z0, p0 = R.wilcoxon(exact["rank_sum2"], exact["group_rows"], exact["tie_sum"], False)
    Mi = int(inc.sum())
    for g in range(K):
        ng = int(exact["group_rows"][g])
        if ng == 0:
            assert not z1[g].any() and not z0[g].any() and (p1[g] == 1).all() and (p0[g] == 1).all()
            continue
        for j in range(N):
            x, y = D[inc & (labels == g), j], D[inc & (labels != g), j]
            if np.unique(D[inc, j]).size == 1:     # nothing to rank: the denominator is 0 with the correction
                assert z1[g, j] == 0 and p1[g, j] == 1
                continue
            res = st.mannwhitneyu(x, y, use_continuity=False, method="asymptotic")
            assert res.statistic == exact["rank_sum2"][g, j] / 2 - ng * (ng + 1) / 2
            T = st.tiecorrect(st.rankdata(D[inc, j]))
            for z, p, corr in ((z1, p1, T), (z0, p0, 1.0)):
                zs = (res.statistic - ng * (Mi - ng) / 2) / np.sqrt(corr * ng * (Mi - ng) * (Mi + 1) / 12.0)
                assert abs(z[g, j] - zs) <= 1e-12 * max(1.0, abs(zs)), (g, j)
            assert abs(p1[g, j] - res.pvalue) <= 1e-12 * max(res.pvalue, 1e-300), (g, j, p1[g, j], res.pvalue)


def test_welch_against_scipy_ttest_ind(case):
    ptr, idx, val, labels, D, exact = case
    inc = (labels >= 0) & (labels < K)
    w = R.welch(*R.moments(ptr, idx, val, M, N, labels, K), exact["group_rows"])
    D64 = D.astype(np.float64)
    for g in range(K):
        if exact["group_rows"][g] == 0:
            assert not w["t"][g].any() and not w["df"][g].any()
            continue
        x, y = D64[inc & (labels == g)], D64[inc & (labels != g)]
        res = st.ttest_ind(x, y, equal_var=False)
        np.testing.assert_allclose(w["mean"][g], x.mean(axis=0), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(w["var"][g], x.var(axis=0, ddof=1), rtol=1e-9, atol=1e-12 * (x ** 2).mean())
        ok = np.isfinite(res.statistic)
        assert not w["t"][g][~ok].any()            # constant columns: scipy's 0 / 0, here t = 0
        np.testing.assert_allclose(w["t"][g][ok], res.statistic[ok], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(w["df"][g][ok], res.df[ok], rtol=1e-9)


def test_single_rows_and_single_groups():
    ptr, idx, val, labels = R.fixture(40, 6, 3, 3, np.float64, "real")
    labels[:] = 0
    labels[5] = 1                                   # a group of one row; group 2 empty
    res = R.rank_groups(ptr, idx, val, 40, 6, labels, 3)
    assert res["group_rows"].tolist() == [39, 1, 0]
    assert not res["t_df"][1].any() and not res["var"][1].any() and not res["z_score"][2].any()
    one = R.rank_groups(ptr, idx, val, 40, 6, np.zeros(40, dtype=np.int32), 1)   # K = 1: no rest
    assert not one["z_score"].any() and (one["z_pvalue"] == 1).all() and not one["t_score"].any()
    assert (R.rank_sums(ptr, idx, val, 40, 6, np.zeros(40, dtype=np.int32), 1)["rank_sum2"] == 40 * 41).all()


def test_symbols_in_header_library_and_bindings():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    for stem in ("sapca_rank_sums_csr_device", "sapca_rank_groups_csr_device"):
        for suf in ("f32", "f64"):
            n = f"{stem}_{suf}"
            assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n) and re.search(rf"\b{n}\(", header), n
    assert int(re.search(r"#define SAPCA_RANK_MAX_GROUPS (\d+)", header).group(1)) == L.RANK_MAX_GROUPS == R.MAX_GROUPS
    sys_rs = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca-sys", "src", "lib.rs")).read()
    assert "pub fn sapca_rank_groups_csr_device_f64(" in sys_rs


def test_class_limits_match_the_kernel_header():
    """what tests/test_gpu_rank_groups.py builds its column lengths from is what csrc/rankgroups.h says"""
    text = open(os.path.join(ROOT, "single-algebra_amd", "csrc", "rankgroups.h")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr int (kRank\w+) = (\d+);", text)}
    assert got == {"kRankWaveMax": R.WAVE_MAX, "kRankLdsMax": R.LDS_MAX, "kRankWalkChunk": R.WALK_CHUNK}
    hip = open(os.path.join(ROOT, "single-algebra_amd", "csrc", "batchstats.hip")).read()
    assert int(re.search(r"constexpr int kBatchCodesPerLaunch = (\d+);", hip).group(1)) == R.MAX_GROUPS


def test_python_argument_checks_come_before_the_library():
    X = ops.ResidentCsr(None, (4, 3), 0, np.float32, 0, 0, 0)
    lab = np.zeros(4, dtype=np.int32)
    for bad in (0, L.RANK_MAX_GROUPS + 1, 2.0, True):
        with pytest.raises(ValueError, match="n_groups"):
            X.rank_sums(lab, bad)
    with pytest.raises(ValueError, match="method"):
        X.rank_groups(lab, 2, method="logreg")
    with pytest.raises(ValueError, match="n_top"):
        X.rank_groups(lab, 2, n_top=-1)
    with pytest.raises(ValueError, match="labels must be 4 integers"):
        X.rank_groups(np.zeros(5, dtype=np.int32), 2)
    with pytest.raises(ValueError, match="labels must be 4 integers"):
        X.rank_groups(np.zeros(4), 2)
    with pytest.raises(ValueError, match="int32"):
        X.rank_groups(np.full(4, 2 ** 40), 2)

    class Unfitted:
        labels_ = None
    with pytest.raises(ValueError, match="not been fitted"):
        X.rank_groups(Unfitted(), 2)


def test_result_object_host_arithmetic():
    scores = np.array([[1.0, 3.0, 3.0, -2.0], [0.0, 0.0, 0.0, 0.0]])
    means = np.array([[0.5, 1.0, 0.0, 2.0], [1.5, 0.0, 0.0, 1.0]])
    nz = np.array([[2, 4, 0, 1], [0, 0, 0, 0]], dtype=np.uint64)
    rows = np.array([4, 0], dtype=np.uint64)
    r = ops.RankGroupsResult("wilcoxon", scores, np.ones_like(scores), means, np.zeros_like(means), nz, rows, 3)
    assert r.names.tolist() == [[1, 2, 0], [0, 1, 2]] == R.names(scores, 3).tolist()      # ties to the lower index, cut to n_top
    assert r.pct_nonzero.tolist() == [[0.5, 1.0, 0.0, 0.25], [0.0, 0.0, 0.0, 0.0]]         # an empty group: 0
    both = ops.RankGroupsResult("both", {"wilcoxon": scores, "t-test": -scores}, {}, means, means, nz, rows, None)
    assert both.names[0].tolist() == [1, 2, 0, 3]
    rows2 = np.array([4, 6], dtype=np.uint64)
    lf = ops.RankGroupsResult("t-test", scores, None, means, means, nz, rows2, None).logfoldchanges()
    rest0 = means[1]                                  # two groups: the rest of one is the other
    want = np.log2((np.expm1(means[0]) + 1e-9) / (np.expm1(rest0) + 1e-9))
    np.testing.assert_allclose(lf[0], want, rtol=1e-12)
    np.testing.assert_allclose(lf[1], -want, rtol=1e-12)


def test_cpp_mirror_compiles_with_the_rank_methods(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "m.cpp"
    src.write_text('#include "%s"\n'
                   'template <typename T> size_t use(const sapca::ResidentCsr<T>& x, const int32_t* d_labels) {\n'
                   '  auto a = x.rank_sums(d_labels, 3);\n'
                   '  auto b = x.rank_groups(d_labels, 3, true, true, true);\n'
                   '  return a.rank_sum2.size() + a.tie_sum.size() + b.z_pvalue.size() + b.t_df.size() + b.group_rows.size();\n'
                   '}\n'
                   'template size_t use<float>(const sapca::ResidentCsr<float>&, const int32_t*);\n'
                   'template size_t use<double>(const sapca::ResidentCsr<double>&, const int32_t*);\n'
                   'int main() { return 0; }\n' % os.path.join(ROOT, "single-algebra_amd", "host", "cpp", "sapca.hpp"))
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_golden_fixture_is_what_the_restatement_writes(golden):
    g = golden("g12_rank_groups.npz")
    m, n, k = (int(x) for x in g["shape"])
    for tag in ("counts", "real"):
        ptr, idx, val, labels = (g[f"{tag}_{x}"] for x in ("ptr", "idx", "val", "labels"))
        exact = R.rank_sums(ptr, idx, val, m, n, labels, k)
        for name in ("rank_sum2", "nonzero", "tie_sum"):
            np.testing.assert_array_equal(exact[name], g[f"{tag}_{name}"])
        for tc in (0, 1):
            res = R.rank_groups(ptr, idx, val, m, n, labels, k, tie_correct=bool(tc))
            np.testing.assert_array_equal(res["z_score"], g[f"{tag}_z_score_tc{tc}"])
            np.testing.assert_array_equal(res["z_pvalue"], g[f"{tag}_z_pvalue_tc{tc}"])
        np.testing.assert_array_equal(res["group_rows"], g[f"{tag}_group_rows"])
        for name in ("mean", "var", "t_score", "t_df"):
            np.testing.assert_allclose(res[name], g[f"{tag}_{name}"], rtol=1e-13, atol=1e-300)

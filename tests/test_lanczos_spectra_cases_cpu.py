"""tests/lanczos_spectra_cases.py held to what each fixture is for, without a device: ranks and multiplicities from numpy's svd
and eigh, and the branch of the driver each one takes from the numpy restatement of lanczos_fit's loop.  If a fixture is
changed so that it no longer reaches its branch, this file says so before a GPU is needed."""
import numpy as np
import pytest

import lanczos_spectra_cases as LC
import spectral_ref as SR


def _f32_exact(A):
    return np.array_equal(A.data.astype(np.float32).astype(np.float64), A.data)


def _sv(A):
    return np.linalg.svd(A.toarray(), compute_uv=False)


# ------------------------------------------------------------------ PCA fixtures
def test_flat_fixture_reaches_every_check_interval():
    A, At = LC.p_flat(False), LC.p_flat(True)
    assert A.shape == (900, 700) and At.shape == (700, 900) and abs(A.nnz / (900 * 700) - 0.05) < 1e-3 and _f32_exact(A)
    assert (At.T != A).nnz == 0                 # the wide case iterates on the same 700 x 700 Gram matrix
    s = _sv(A)
    assert np.max(s[:100] / s[1:101]) < 1.02    # flat: no two neighbours among the leading hundred are 2 % apart
    assert [LC.step_class(LC.P_FLAT_STEPS[k]) for k in LC.P_FLAT_KS] == [2, 4, 4, 8] and LC.P_FLAT_STEPS[LC.P_FLAT_KS[-1]] > 256
    for k in LC.P_FLAT_KS:
        r = LC.pca_lanczos(A, k)
        # (the recorded count is this restatement's on one numpy build; another BLAS may move it by a check, not by a class
        # where the count is a tenth of itself away from 64, 128 and 256 -- the same rule the GPU test asserts the class by)
        assert r["status"] == "ok" and abs(r["steps"] - LC.P_FLAT_STEPS[k]) <= 8, (k, r["steps"])
        if min(abs(LC.P_FLAT_STEPS[k] - b) for b in (64, 128, 256)) > LC.P_FLAT_STEPS[k] / 10:
            assert LC.step_class(r["steps"]) == LC.step_class(LC.P_FLAT_STEPS[k]), (k, r["steps"])
        np.testing.assert_allclose(r["sigma"], s[:k], rtol=LC.KAPPA)
    # every step checked: s1, and the schedule's count lies in [s1, s1 + interval - 1]
    s1, s8 = LC.pca_lanczos(A, 8, every_step=True)["steps"], LC.pca_lanczos(A, 8)["steps"]
    assert s1 <= s8 <= s1 + LC.step_class(s8) - 1


def test_all_and_tiny_fixtures():
    for wide in (False, True):
        A = LC.p_all(wide)
        assert A.shape == ((12, 30) if wide else (30, 12)) and np.linalg.matrix_rank(A.toarray()) == 12 and _f32_exact(A)
        s = _sv(A)
        for k in (11, 12):
            r = LC.pca_lanczos(A, k)
            assert r["status"] == "ok" and r["steps"] == 12 and r["right_side"] == (not wide)
            np.testing.assert_allclose(r["sigma"], s[:k], rtol=1e-12)
            np.testing.assert_allclose(r["Vt"] @ r["Vt"].T, np.eye(k), atol=1e-10)
    for shape in LC.P_TINY_SHAPES:
        A = LC.p_tiny(shape)
        assert A.shape == shape and A.nnz == shape[0] * shape[1] and _f32_exact(A)
        for k in range(1, min(shape) + 1):
            r = LC.pca_lanczos(A, k)
            assert r["status"] == "ok" and r["steps"] <= min(shape)
            np.testing.assert_allclose(r["sigma"], _sv(A)[:k], rtol=1e-12)


def test_rank_fixture_is_refused_above_its_rank_on_both_sides_whatever_the_start():
    for wide in (False, True):
        A = LC.p_rank(wide)
        D = A.toarray()
        assert np.array_equal(D, np.round(D)) and np.abs(D).max() < 2 ** 24 and np.linalg.matrix_rank(D) == LC.P_RANK
        s = _sv(A)
        assert s[LC.P_RANK] < 1e-12 * s[0]
        for seed in (42, 43, 44):
            r = LC.pca_lanczos(A, LC.P_RANK, seed=seed)
            assert r["status"] == "ok" and r["steps"] == LC.P_RANK + 1
            np.testing.assert_allclose(r["sigma"], s[:LC.P_RANK], rtol=1e-12)
            for k in (LC.P_RANK + 1, LC.P_RANK + 3):
                r = LC.pca_lanczos(A, k, seed=seed)
                assert r["status"] == "rank" and r["rank"] == LC.P_RANK, (wide, seed, k, r)


def test_zero_and_cap_fixtures_end_in_their_error_branches():
    for stored in (False, True):
        A = LC.p_zero(stored)
        assert (A.nnz > 0) == stored and not A.data.any()
        r = LC.pca_lanczos(A, 3)
        assert r["status"] == "rank" and r["rank"] == 0 and r["steps"] == 3
    A = LC.p_cap()
    n = LC.P_CAP_N
    assert A.shape == (n, n) and n <= 5000 and LC.pca_jmax(n, n, 1) == 620
    G = (A.T @ A).toarray()
    assert np.array_equal(np.diag(G)[1:], np.full(n - 1, 2.0)) and np.array_equal(np.diag(G, 1), np.ones(n - 1))
    r = LC.pca_lanczos(A, 1)
    assert r["status"] == "not converged" and r["steps"] == 620     # n = 5000 is long enough: the cap is reached


def test_repeated_and_clustered_fixtures_and_what_one_start_vector_returns():
    A = LC.p_mult()
    s = _sv(A)
    assert A.shape == (600, 240) and _f32_exact(A)
    np.testing.assert_allclose(s[0:12:2], s[1:12:2], rtol=1e-13)             # every value twice ...
    assert np.min(s[1:11:2] / s[2:12:2]) > 1 + 1e-3                          # ... and the pairs well apart
    for k in LC.P_MULT_KS:
        r = LC.pca_lanczos(A, k)
        # a single-vector run returns each distinct value once: reference behaviour (las2), pinned
        assert r["status"] == "ok"
        np.testing.assert_allclose(r["sigma"], s[0:2 * k:2], rtol=LC.KAPPA)
    B = LC.p_mult(1.0 + 1e-7)
    t = _sv(B)
    gaps = t[0:12:2] / t[1:12:2] - 1
    assert np.all(gaps > 0.5e-7) and np.all(gaps < LC.KAPPA)                 # clustered: apart, by less than kappa
    r = LC.pca_lanczos(B, 2)
    assert r["status"] == "ok" and abs(r["sigma"][1] / t[2] - 1) < LC.KAPPA  # the second copy of the first value is skipped


# ------------------------------------------------------------------ graphs
def _multiplicities(w, width=1e-12):
    return [b - a for a, b in LC.clusters(w, width)]


def test_graph_fixtures_have_the_multiplicities_they_are_for():
    for name in LC.GRAPHS:
        G = LC.graph(name)
        assert abs(G - G.T).max() == 0 and G.data.min() > 0 and G.shape[0] <= 1000
        assert _f32_exact(G) == (name != "ring64_1e-10")
    g = LC.graph_spectrum
    assert _multiplicities(g("ring64", SR.NORMALIZED)["w"])[:4] == [2, 2, 2, 2]
    assert _multiplicities(g("ring1000x6", SR.NORMALIZED)["w"])[:4] == [2, 2, 2, 2]
    assert _multiplicities(g("grid12", SR.NORMALIZED)["w"])[:2] == [2, 1] and _multiplicities(g("grid30", SR.NORMALIZED)["w"])[:2] == [2, 1]
    k16 = g("k16", SR.NORMALIZED)
    assert k16["U"].shape[1] == 1 and _multiplicities(k16["w"]) == [15] and abs(k16["w"][0] + 1 / 15) < 1e-15
    star = g("star200", SR.NORMALIZED)
    assert _multiplicities(star["w"]) == [199, 1] and abs(star["w"][-1] + 1) < 1e-14 and np.max(np.abs(star["w"][:-1])) < 1e-14
    two = g("two_rings64", SR.NORMALIZED)
    assert two["n_components"] == 2 and two["U"].shape[1] == 2 and _multiplicities(two["w"])[:2] == [4, 4]
    for kind in (SR.NORMALIZED, SR.DIFFMAP):
        near = g("ring64_1e-6", kind)["w"]
        split = near[0:8:2] - near[1:8:2]
        assert np.all(split > 10 * 1e-11) and np.all(split < 10 * LC.TOL)      # one cluster (10 tol) at tol = 1e-8, two at 1e-12
        nearer = g("ring64_1e-10", kind)["w"]
        assert np.all(nearer[0:8:2] - nearer[1:8:2] < LC.TOL / 100)    # far below tol: either order is right
    # float32 cannot hold the 1e-10 perturbation: the f32 variant of that graph is the exact ring
    assert np.array_equal(LC.graph("ring64_1e-10").data.astype(np.float32), np.ones(128, dtype=np.float32))


@pytest.mark.parametrize("name", LC.DEGENERATE)
def test_one_run_misses_the_copies_the_rounds_find(name):
    """the restatement of ONE run returns too few copies of a repeated value on every degenerate fixture (or fewer pairs than
    were asked for); the rounds return the exact values counted with multiplicity"""
    for kind in (SR.NORMALIZED, SR.DIFFMAP):
        g = LC.graph_spectrum(name, kind)
        c = g["U"].shape[1]
        k = 9 - c
        r = SR.lanczos_rounds(g["S"], g["U"], k)
        first = r["first"]
        assert len(first) < k or np.max(np.abs(first - g["w"][:k])) > 1e-3, (name, kind)
        assert r["rounds"] >= 3
        np.testing.assert_allclose(r["evals"], g["w"][:k], rtol=0, atol=1e-12)

"""The cases of tests/sharded_fit_cases.py are what they claim and its reference is right, checked without a GPU: the partition
restated there equals the library's (sapca_partition_rows is host code) plus the fallback of shard_bounds, every case has the
property it is listed for, the sharded restatement of the randomized fit agrees with the oracle's unsharded one to 1e-12, and
the operator of every case has the gap the tolerances of tests/test_gpu_sharded_fit.py presuppose."""
import numpy as np
import pytest

import sapca_oracle as O
import sharded_fit_cases as C
from sapca import ops

IDS = [c.name for c in C.CASES]


def _library_partition(indptr, nd):
    b = ops.partition_rows(np.asarray(indptr), nd).astype(np.int64)
    m = len(indptr) - 1
    return C.even_bounds(m, nd) if np.any(np.diff(b) == 0) else b


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_partition_equals_the_librarys_on_every_case(c):
    ptr = c.A.indptr
    assert np.array_equal(C.nnz_bounds(ptr, c.nd), ops.partition_rows(ptr, c.nd).astype(np.int64))
    assert np.array_equal(c.bounds, _library_partition(ptr, c.nd))
    assert c.bounds[0] == 0 and c.bounds[-1] == c.A.shape[0] and np.all(np.diff(c.bounds) > 0)


def test_partition_equals_the_librarys_on_random_offsets():
    rng = np.random.default_rng(5)
    kinds = {"empty": 0, "short": 0, "long_row": 0, "empty_runs": 0, "fallback": 0}
    for trial in range(400):
        kind = ("empty", "short", "long_row", "empty_runs", "plain")[trial % 5]
        nd = int(rng.integers(1, 9))
        m = int(rng.integers(nd, 2 * nd)) if kind == "short" else int(rng.integers(nd, 200))
        lens = rng.integers(0, 12, size=m)
        if kind == "empty":
            lens[:] = 0
        if kind == "long_row":
            lens[int(rng.integers(0, m))] = int(rng.integers(1, 6)) * max(1, int(lens.sum()))
        if kind == "empty_runs":
            for _ in range(3):
                a = int(rng.integers(0, m))
                lens[a:a + int(rng.integers(1, m))] = 0
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        if trial % 7 == 0:
            ptr = ptr + 11                                    # (offsets of a slice: they need not start at 0)
        got = C.nnz_bounds(ptr, nd)
        assert np.array_equal(got, ops.partition_rows(ptr, nd).astype(np.int64)), (kind, nd, ptr.tolist())
        assert np.array_equal(C.partition(ptr, nd), _library_partition(ptr, nd))
        assert np.all(np.diff(C.partition(ptr, nd)) > 0)      # m >= nd: every member gets a row
        if kind in kinds:
            kinds[kind] += 1
        kinds["fallback"] += int(np.any(np.diff(got) == 0))
    assert min(kinds.values()) >= 20, kinds


def test_every_edge_is_listed():
    assert {c.edge for c in C.CASES} == set("abcdefghij")
    assert sorted(c.nd for c in C.CASES if c.edge == "a") == [2, 3, 4, 7]
    assert sorted(c.nd for c in C.CASES if c.edge == "b") == [3, 4]
    assert {c.normalizer for c in C.CASES if c.edge == "f"} == {"LU", "NONE"}
    assert all(not c.center for c in C.CASES if c.edge == "e")
    assert all(c.mask is not None and abs(c.mask.mean() - 0.6) < 0.08 for c in C.CASES if c.edge == "g")
    assert all(c.scale == "unit_variance" for c in C.CASES if c.edge == "h")
    two = [c for c in C.TWO_PIECE]
    assert {(c.l <= 64, c.nd, c.mask is not None, c.center) for c in two} == {(a, b, d, e) for a in (True, False) for b in (2, 3)
                                                                               for d in (True, False) for e in (True, False)}
    assert all(64 < c.l <= 128 or c.l <= 64 for c in two) and all(1300 <= c.n_used <= 2600 for c in two)
    lz = C.LANCZOS
    assert {(dt, c.mask is not None) for c in lz if not c.lanczos_center for dt in c.dtypes} == {(d, mk) for d in ("float64", "float32")
                                                                                                  for mk in (True, False)}
    assert any(c.lanczos_center for c in lz)


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_values_are_small_integers_with_exact_sums(c):
    A = c.A
    assert A.has_canonical_format and np.array_equal(A.data, np.rint(A.data)) and A.data.min() >= 1 and A.data.max() <= 12
    # every column sum of squares stays below 2^24: exact in f32 as well, in any order
    assert float(A.multiply(A).sum(0).max()) < 2 ** 24


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_case_has_the_property_it_is_listed_for(c):
    A, b = c.A, c.bounds
    m, n = A.shape
    rows = np.diff(b)
    entries = np.diff(A.indptr[b])
    fallback = bool(np.any(np.diff(C.nnz_bounds(A.indptr, c.nd)) == 0))
    assert fallback == (c.edge == "d")
    if c.edge == "a":
        assert (m, n) == (1500, 260) and 28000 <= A.nnz <= 38000 and entries.max() - entries.min() <= 2 * np.diff(A.indptr).max()
    if c.edge == "b":                  # a boundary falls behind the last row that holds anything: rows, and no entry
        assert not fallback and entries[-1] == 0 and rows[-1] == 1439 and np.all(entries[:-1] > 0)
    if c.name == "d_m_equals_nd":      # one row per member, and the last member's holds nothing
        assert m == c.nd and np.array_equal(b, np.arange(m + 1)) and entries[-1] == 0 and rows[-1] == 1
    if c.name == "d_long_first_row":
        assert np.array_equal(C.nnz_bounds(A.indptr, 3), [0, 0, 1, m]) and np.array_equal(b, [0, m // 3, 2 * m // 3, m])
        assert np.diff(A.indptr)[0] > 2 * A.nnz / 3
    if c.edge == "c":
        assert rows.max() < c.l and c.l == min(c.l_req, m)
    if c.name == "c_l_cut_to_m_global":
        assert c.l_req > m and c.l == m
    if c.edge == "i":
        assert c.dtypes == ("float32",) and c.natural_order and (c.l == 12 or c.l == 70)
    if c.edge == "j":
        assert c.n_used <= m and rows.max() < c.n_used and c.method == "LANCZOS"     # tall overall, every shard wide
    assert c.k <= min(m, c.n_used) and c.omega.shape == (c.n_used, c.l_req)


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_gap_condition(c):
    """sigma_k / sigma_{k+1} of the dense operator (centred, masked, scaled as the fit sees it): at least 1.25, Lanczos 1.05.
    A condition on the inputs: a case that misses it gets another matrix."""
    g = C.gap(c)
    print(f"{c.name}: gap {g:.3f}")
    assert g >= (1.05 if c.method == "LANCZOS" else 1.25)
    s, _ = C.exact_svd(c.name)
    if c.scale is None:                                       # (unit variance levels the clusters: the subspace alone is compared there)
        assert np.all(s[:c.k - 1] / s[1:c.k] >= 1.02)         # the leading directions are vectors of their own, too


def _distinct(cases):
    seen, out = set(), []
    for c in cases:
        key = (c.mat, c.k, c.p, c.q, c.center, c.normalizer, c.mask_seed, c.scale, tuple(c.bounds))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("c", _distinct(C.RANDOMIZED), ids=lambda c: c.name)
def test_sharded_restatement_agrees_with_the_unsharded_oracle(c):
    got, want = C.reference_fit(c), C.oracle_fit(c)
    ds = float(np.max(np.abs(got.singular_values / want.singular_values - 1)))
    ang = O.subspace_angle(got.components, want.components)
    print(f"{c.name}: sigma {ds:.2e}  angle {ang:.2e}")
    assert ds <= 1e-12 and ang <= 1e-12
    np.testing.assert_allclose(got.components, want.components, atol=1e-10)                 # signs included
    m = c.A.shape[0]
    if c.scale is None:
        assert np.array_equal(got.mean, want.mean)                                          # exact sums, one division
        np.testing.assert_allclose(got.total_var, float(want.total_var), rtol=1e-12)
    else:
        assert abs(got.total_var - np.count_nonzero(got.scale)) <= 1e-10 * c.n_used          # unit variance: one per live column
    # the projection: rows [b_i, b_i+1) of the whole matrix's, in both semantics
    A = c.A
    mu = got.mean
    D = A.toarray() - (mu[None, :] if c.center else 0.0)
    D = D if c.mask is None else D[:, c.mask]
    D = D if got.scale is None else D * got.scale
    np.testing.assert_allclose(got.scores_centered, D @ got.components.T, atol=1e-11 * np.abs(got.scores_centered).max())
    if c.scale is None and c.mask is None:
        want_t = O.transform_sparse(A.indptr, A.indices, A.data, m, A.shape[1], got.components, mu, c.center)
        np.testing.assert_allclose(got.scores, want_t, atol=1e-11 * np.abs(want_t).max())
    elif c.scale is None:
        want_t = O.transform_masked(A.indptr, A.indices, A.data, m, A.shape[1], got.components, mu, c.center, c.mask)
        np.testing.assert_allclose(got.scores, want_t, atol=1e-11 * np.abs(want_t).max())
    else:
        assert got.scores is None


def test_restatement_does_not_depend_on_the_member_count():
    fits = [C.reference_fit(C.BY_NAME[f"a_balanced_nd{nd}"]) for nd in (2, 3, 4, 7)]
    for f in fits[1:]:
        assert f.mean.tobytes() == fits[0].mean.tobytes() and f.total_var == fits[0].total_var
        assert O.subspace_angle(f.components, fits[0].components) <= 1e-12

"""CPU tests of the reference for the implicit column scaling (tests/column_scaling_ref.py): the oracle run on the prescaled
CSR -- what the GPU tests compare the library with -- is pinned against a dense SVD of the scaled operator, so that the
reference itself cannot drift."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import column_scaling_ref as R
import sapca_oracle as O
from sapca import synth

K = R.K
SHAPES = [(320, 208), (385, 250), (513, 257)]


def _dense_leading(S, k):
    _, s, vt = np.linalg.svd(S, full_matrices=False)
    return s, vt[:k]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("seed", [3, 4, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_on_the_prescaled_csr_is_the_svd_of_the_scaled_operator(shape, seed, center, masked):
    """Total variance (centred; under UNIT_VARIANCE the number of live columns to 1e-12 n_used), singular values and the
    leading subspace.  The oracle's randomized SVD (p = 6, q = 4) of an operator with sigma_4 / sigma_5 = g leaves the
    subspace within about (1 / g)^(2 q + 1) of the exact one: g >= 2 is asserted, 2^-9 = 2e-3 is the bound used."""
    m, n = shape
    A = R.scaled_case(m, n, seed, centred=center)
    mask = synth.bernoulli_mask(n, 0.7, seed).numpy() if masked else None
    d = R.unit_variance_factors(A)[0]
    S = R.scaled_operator(A, d, center, mask)
    n_used = S.shape[1]
    sv, vt = _dense_leading(S, K)
    g = sv[K - 1] / sv[K]
    assert g >= 2.0, f"gap {g:.2f}"
    assert 3.0 <= g <= 4.7, f"gap {g:.2f} outside the range computed for these matrices"
    # the unscaled operator has no such gap: a fit that ignored the scaling lands somewhere else
    plain = np.linalg.svd(R.scaled_operator(A, np.ones(n), center, mask), compute_uv=False)
    assert plain[K - 1] / plain[K] < 2.0
    om = synth.gaussian_panel(n_used, K + 6, seed + 7).numpy()
    want = R.expected_fit(A, d, center=center, n_components=K, n_oversamples=6, n_power_iterations=4, normalizer="QR", omega=om, mask=mask)
    np.testing.assert_allclose(want.singular_values, sv[:K], rtol=1e-6)
    assert O.subspace_angle(want.components, vt) < 2.0 ** -9
    if center:
        tv = (S ** 2).sum() / (m - 1)
        np.testing.assert_allclose(want.total_var, tv, rtol=1e-10)
        used = slice(None) if mask is None else mask
        assert abs(want.total_var - np.count_nonzero(d[used])) <= 1e-12 * n_used
    np.testing.assert_allclose(want.mean, (A.toarray().mean(axis=0) * d) if center else np.zeros(n), atol=1e-12)


@pytest.mark.parametrize("masked", [False, True])
def test_edge_matrix(masked):
    """an empty column, two constant ones and a single-entry column: the zero rule, the live count and the gap"""
    A = R.edge_case()
    m, n = A.shape
    D = A.toarray()
    assert A[:, 3].nnz == 0 and A[:, 10].nnz == m and A[:, 11].nnz == m and A[:, 12].nnz == 1 and D[17, 12] == 2.5
    d, ss, s2 = R.unit_variance_factors(A)
    assert not d[[3, 10, 11]].any() and np.isfinite(d).all() and d[12] > 0
    assert np.count_nonzero(d) == 205
    # numpy's own sums leave a NEGATIVE ss for 320 copies of 0.1f: `ss == 0` would be the wrong test, 1 / sqrt(ss) a NaN
    assert ss[11] < 0 and abs(ss[11]) < 4 * m * R.EPS64 * s2[11]
    mask = synth.bernoulli_mask(n, 0.7, 4).numpy() if masked else None
    S = R.scaled_operator(A, d, True, mask)
    assert abs((S ** 2).sum() / (m - 1) - np.count_nonzero(d if mask is None else d[mask])) < 1e-10
    assert abs(R.gap(S, K) - (3.25 if masked else 3.79)) < 0.01


def test_factor_rule_and_bound():
    """d against an extended-precision evaluation stays within the derived bound; the threshold keeps constant columns out"""
    A = R.scaled_case(320, 208, 4)
    d, ss, s2 = R.unit_variance_factors(A)
    D = A.toarray().astype(np.longdouble)
    m = D.shape[0]
    ssx = (D * D).sum(axis=0) - D.sum(axis=0) ** 2 / m
    dx = (1.0 / np.sqrt(ssx / (m - 1))).astype(np.float64)
    assert (np.abs(d / dx - 1) <= R.factor_bound(m, ss, s2)).all()
    const = np.full((320, 3), [3.0, float(np.float32(0.1)), 1e-30])
    assert not R.unit_variance_factors(const)[0].any()
    assert R.prescaled(A, d).nnz == A.nnz

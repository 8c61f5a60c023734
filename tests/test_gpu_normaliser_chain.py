"""The chain between two sweeps of a randomized fit -- Gram (gramv / gram_reduce), Cholesky, panel GEMM -- at the shapes where
its kernels take another path: one tile, tile remainders, fewer tiles than workgroups, panels still lying in the un-summed
slabs of an A^T sweep whose tile range was split over workgroups, and Omega generated on the device."""
import numpy as np
import pytest
import torch

import sapca
import sapca_oracle as O
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def session():
    return ops.Session()


# ------------------------------------------------------------------ plain panels
@pytest.mark.parametrize("l", [60, 64, 110])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 63, 64, 65, 4099, 16400])
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 5e-6)])
def test_plain_panels_orthonormal_same_span_same_bytes(session, dtype, tol, rows, l):
    """normalize_panel(P, QR) on Gaussian panels: two calls return the same bytes; Q^T Q = I and the subspace angle to
    numpy.linalg.qr at the bounds of test_normalizer_qr_orthonormal_same_span (20 tol; 1e-9 / 2e-3 rad).  l = 60 / 64 take the
    64-column kernels, l = 110 the 112-column ones.  1 to 65 rows are one to five row tiles with and without a remainder;
    4099 rows are 257 tiles, four to a workgroup; 16400 rows are 1025 tiles, past the 1024 from which 64-column panels are
    multiplied by workgroups of eight waves.
    A panel with fewer rows than columns has rank `rows`: no l orthonormal columns exist, whatever computes them, and the
    Cholesky factor's floored pivots (dense.hip, chol_inv) leave directions that are not meant to be read.  Those panels
    are run -- tile remainders do not depend on the width -- and their bytes compared; the two numerical properties are
    asserted where they can hold, rows >= l."""
    P = synth.gaussian_panel(rows, l, 100 + l).numpy().astype(dtype)
    Q = session.normalize_panel(P, PIN.QR)
    Q2 = session.normalize_panel(P, PIN.QR)
    assert Q.shape == P.shape and Q.dtype == P.dtype
    assert Q.tobytes() == Q2.tobytes()
    if rows < l:
        return
    Q64 = Q.astype(np.float64)
    err = float(np.abs(Q64.T @ Q64 - np.eye(l)).max())
    q_ref, _ = np.linalg.qr(P.astype(np.float64))
    ang = float(O.subspace_angle(Q.T, q_ref.T))
    print(f"rows {rows} l {l} {np.dtype(dtype).name}: |Q^T Q - I| {err:.3e} (bound {tol * 20:.1e}), angle {ang:.3e}")
    assert err <= tol * 20
    assert ang < (1e-9 if dtype == np.float64 else 2e-3)


# ------------------------------------------------------------------ panels in the slabs of a split A^T sweep
K, OVER, Q_IT, N_COLS, DENSITY = 10, 6, 2, 600, 0.05
_cases = {}


def _case(m):
    """matrix, Omega and the oracle's fit for one height: made once, shared, never modified"""
    if m not in _cases:
        dev = synth.gapped_csr(m, N_COLS, DENSITY, K, seed=42, dtype=torch.float32, device="cuda:0")
        ptr, idx, val = (x.cpu().numpy() for x in dev)
        idx = idx.astype(np.int64)
        om = synth.gaussian_panel(N_COLS, K + OVER, 42).numpy()
        want = O.fit(ptr.astype(np.int64), idx, val.astype(np.float64), m, N_COLS, n_components=K, n_oversamples=OVER,
                     n_power_iterations=Q_IT, omega=om)
        _cases[m] = (dev, om, want)
    return _cases[m]


def _fit(m, dev, om, variant, seed=42):
    b = (sapca.SparsePCABuilder.new().n_components(K).random_seed(seed).spmm_variant(variant).collect_timings(True)
         .svd_method(SVDMethod.Random(OVER, Q_IT, PIN.QR)).build())
    if om is not None:
        b = b.set_omega(om)
    b.fit(sapca.DeviceCsr(*dev, (m, N_COLS)))
    return b


@pytest.mark.parametrize("m", [900, 1300, 20000, 33000, 50000])
def test_fit_through_unsummed_slabs(m):
    """A centred f32 fit through the DPP-fed sweep (spmm_variant 2) on a tall thin matrix: A^T has 600 rows, two row blocks
    of 512, so its tile range (320 columns of A^T a tile) is split over workgroups and the Gram of every normalisation of X
    sums the slabs on its way through.  quad_geometry gives nsplit = min(tiles, 512 / 2):
        m = 20000: 63 tiles, nsplit 63 -- 62 further slabs = 4 with the chunk's head + 14 x 4 + a remainder of 2
        m = 33000: 104 tiles, nsplit 104 -- 103 = 4 + 24 x 4 + a remainder of 3
        m = 50000: 157 tiles, nsplit 157 -- 156 = 4 + 38 x 4, no remainder
    and, beyond what the three heights reach, the short ends of the same loop:
        m = 900: 3 tiles, nsplit 3 -- the head alone, not full;  m = 1300: 5 tiles, nsplit 5 -- the head alone, full.
    Singular values and subspace angle against the oracle and against the row kernel (spmm_variant 1) at the 1e-4 bounds of
    test_random_configurations_against_the_oracle; two runs give the same bytes."""
    dev, om, want = _case(m)
    a = _fit(m, dev, om, 2)
    assert int(a.timings().sweep_kernel) == 2, "the DPP-fed sweep did not run"
    s_a, c_a = a.singular_values_(np.float64), a.components_(np.float64)
    ang = float(O.subspace_angle(c_a, want.components))
    rel = float(np.abs(s_a / want.singular_values - 1).max())
    row = _fit(m, dev, om, 1)
    s_r, c_r = row.singular_values_(np.float64), row.components_(np.float64)
    ang_r = float(O.subspace_angle(c_a, c_r))
    rel_r = float(np.abs(s_a / s_r - 1).max())
    print(f"m {m}: oracle sigma {rel:.3e} angle {ang:.3e}; row kernel sigma {rel_r:.3e} angle {ang_r:.3e}")
    np.testing.assert_allclose(s_a, want.singular_values, rtol=1e-4)
    assert ang < 1e-4
    np.testing.assert_allclose(s_a, s_r, rtol=1e-4)
    assert ang_r < 1e-4
    b = _fit(m, dev, om, 2)
    assert a.singular_values_(np.float32).tobytes() == b.singular_values_(np.float32).tobytes()
    assert a.components_(np.float32).tobytes() == b.components_(np.float32).tobytes()


# ------------------------------------------------------------------ Omega generated on the device
def test_generated_omega_equals_the_injected_one():
    """random_seed(42) and no injection is the fit with synth.gaussian_panel(n, l, 42) injected: 1e-6 relative on the singular
    values (an Omega queued into the wrong buffer, or before its buffer exists, is another panel altogether)"""
    m = 20000
    dev, om, _ = _case(m)
    gen = _fit(m, dev, None, 2, seed=42)
    inj = _fit(m, dev, om, 2, seed=42)
    s_g, s_i = gen.singular_values_(np.float64), inj.singular_values_(np.float64)
    print(f"generated vs injected Omega: sigma {float(np.abs(s_g / s_i - 1).max()):.3e}")
    np.testing.assert_allclose(s_g, s_i, rtol=1e-6)

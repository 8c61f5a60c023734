"""The spectral solve on graphs with repeated, nearly repeated and few distinct eigenvalues (-m gpu): rings, grids, a complete
graph, a star, two disjoint rings and rings with perturbed weights (tests/lanczos_spectra_cases.py).  One Lanczos run from one
start vector returns every distinct value once; the rounds of stage 5 (include/sapca.h) find the further copies.

The reference is numpy's eigh of the dense f64 operator in the complement of the locked vectors (lanczos_spectra_cases.
graph_spectrum), with the weights rounded to the dtype under test.  Bounds, with tol = 1e-8, steps the n_steps the call returned
(the sum over its rounds) and k = n_eigen - c pairs iterated:
  rb       = tol + 64 steps eps: the acceptance bound of a run plus the rounding of its steps (test_gpu_spectral.py's).
  residual r_i = |S v_i - theta_i v_i| <= sqrt(1 + 2 k) tol + 64 steps eps.  A run's own bound is tol; a later round iterates on
           S in the complement of the held vectors X (at most 2 k, each with residual <= tol), and for a Ritz vector y of that
           round S y - theta y = (P S P y - theta y) + X X^T S y, whose second term is |(S X - X Theta)^T y| <= sqrt(2 k) tol.
  value    |theta_i - lambda_i| <= rb + m eps, lambda_i the i-th exact eigenvalue COUNTED WITH MULTIPLICITY.
  vector   a cluster is a run of exact eigenvalues within 10 tol of their neighbours; v_i is within 4 r_i / gap of the
           eigenspace of lambda_i's cluster, gap the distance from the cluster to the rest of the spectrum, plus eigh's own
           error 64 m eps / gap, plus what of v_i lies along the locked vectors (the columns bound below), plus 2^-23 for a
           vector rounded to float32.  A cluster that is the whole spectrum has gap = inf.
  columns  |v_i . v_j - delta_ij| <= 64 steps eps + m eps (+ 2^-22 in float32: two roundings of unit vectors)."""
import numpy as np
import pytest
import torch

import lanczos_spectra_cases as LC
import spectral_ref as SR
from sapca import _lib as L
from sapca import ops

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TOL = LC.TOL
DTYPES = [np.float32, np.float64]
IDS = dict(ids=["f32", "f64"])
KINDS = (SR.NORMALIZED, SR.DIFFMAP)
N_EIGEN = (2, 3, 5, 9)
ALSO_16 = ("k16", "ring64", "ring1000x6", "two_rings64")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def sess():
    return ops.Session()


def _resident(sess, G, data):
    return ops.ResidentCsr.from_torch(sess, _dev(G.indptr.astype(np.int64)), _dev(G.indices.astype(np.int32)), _dev(data), G.shape)


def _check(name, kind, dt, n_eigen, ref, evals, E, E64, ncomp, steps, tol=TOL):
    LD = np.longdouble
    m = ref["S"].shape[0]
    U, w, Q = ref["U"], ref["w"], ref["Q"]
    c = min(U.shape[1], n_eigen)
    k = n_eigen - c
    assert ncomp == ref["n_components"]
    assert E.dtype == dt and E.shape == (m, n_eigen) and np.all(np.isfinite(E)) and np.all(np.isfinite(evals))
    assert np.all(evals[:c] == 1.0)
    ulp4 = 4 * np.spacing(np.abs(U[:, :c]).astype(dt)).astype(np.float64)
    assert np.all(np.abs(E[:, :c].astype(np.float64) - U[:, :c].astype(dt).astype(np.float64)) <= ulp4)
    if k == 0:
        assert steps == 0
        return
    assert steps > 0 and np.all(np.diff(evals[c:]) <= 0)
    rb = tol + 64 * steps * EPS
    rmax = np.sqrt(1 + 2 * k) * tol + 64 * steps * EPS
    S = ref["S"].astype(LD)
    V64 = E64.astype(LD)
    groups = LC.clusters(w, 10 * tol)
    f32 = dt == np.float32
    worst = dict(r=0.0, dth=0.0, dv=0.0)
    for i in range(k):
        theta, v = LD(evals[c + i]), V64[:, c + i]
        ri = float(np.sqrt(np.sum((S @ v - theta * v) ** 2)))
        dth = abs(float(evals[c + i]) - w[i])
        a, b = next(g for g in groups if g[0] <= i < g[1])
        gap = min(w[a - 1] - w[a] if a > 0 else np.inf, w[b - 1] - w[b] if b < len(w) else np.inf)
        Qc = Q[:, a:b]
        x = E[:, c + i].astype(np.float64)
        dv = float(np.linalg.norm(x - Qc @ (Qc.T @ x)))
        bound_v = 4 * ri / gap + 64 * m * EPS / gap + 64 * steps * EPS + m * EPS + (2.0 ** -23 if f32 else 0.0)
        worst = dict(r=max(worst["r"], ri / rmax), dth=max(worst["dth"], dth / (rb + m * EPS)), dv=max(worst["dv"], dv / bound_v))
        assert ri <= rmax, (i, ri, rmax)
        assert dth <= rb + m * EPS, (i, float(evals[c + i]), w[i], dth, rb)
        assert dv <= bound_v, (i, dv, bound_v, gap, (a, b))
        at = int(np.argmax(np.abs(E64[:, c + i])))
        assert E64[at, c + i] > 0, i
    print(f"{name} {kind} {np.dtype(dt).name} n_eigen {n_eigen}: steps {steps}, worst r / bound {worst['r']:.3e}, "
          f"|theta - lambda| / bound {worst['dth']:.3e}, distance / bound {worst['dv']:.3e}")
    X = E.astype(np.float64)
    assert np.max(np.abs(X.T @ X - np.eye(n_eigen))) <= 64 * steps * EPS + m * EPS + (2.0 ** -22 if f32 else 0.0)


# The 64-ring with weights off by 1e-6 relative once more at tol = 1e-12: a relative change d of the weights moves 1 - lambda
# by at most d (1 - lambda), so its pairs are split by some 1e-9 -- one cluster each at the default tol, two at this one.
CASES = [(name, TOL) for name in LC.GRAPHS] + [("ring64_1e-6", 1e-12)]


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,tol", CASES, ids=[f"{n}-tol{t:g}" for n, t in CASES])
def test_pairs_are_counted_with_multiplicity(sess, name, tol, kind, dt):
    G = LC.graph(name)
    data = G.data.astype(dt)
    ref = LC.graph_spectrum(name, kind, np.dtype(dt).name)
    R = _resident(sess, G, data)
    R64 = _resident(sess, G, data.astype(np.float64)) if dt == np.float32 else R
    for n_eigen in N_EIGEN + ((16,) if name in ALSO_16 else ()):
        evals, Et, ncomp, steps = sess.spectral(R, n_eigen=n_eigen, kind=kind, tol=tol)
        E = Et.cpu().numpy()
        E64 = E
        if dt == np.float32:   # every sum is f64 from the stored values: the f64 variant runs the same iteration and rounds at the end
            ev64, E64t, _, st64 = sess.spectral(R64, n_eigen=n_eigen, kind=kind, tol=tol)
            E64 = E64t.cpu().numpy()
            assert ev64.tobytes() == evals.tobytes() and st64 == steps and E64.astype(np.float32).tobytes() == E.tobytes()
        _check(name, kind, dt, n_eigen, ref, evals, E, E64, ncomp, steps, tol)
        # the same bytes from call to call, and from the host route
        ev2, E2, nc2, st2 = sess.spectral(R, n_eigen=n_eigen, kind=kind, tol=tol)
        assert ev2.tobytes() == evals.tobytes() and E2.cpu().numpy().tobytes() == E.tobytes() and (nc2, st2) == (ncomp, steps)
        ev3, E3, nc3, st3 = sess.spectral_host(G.indptr, G.indices, data, n_eigen=n_eigen, kind=kind, tol=tol)
        assert ev3.tobytes() == evals.tobytes() and E3.tobytes() == E.tobytes() and (nc3, st3) == (ncomp, steps)
        if name == "two_rings64":
            assert ncomp == 2 and np.all(evals[:2] == 1.0)


@pytest.mark.parametrize("kind", KINDS)
def test_perturbed_ring_resolves_both_members_of_every_pair(sess, kind):
    """weights off by 1e-6 relative split the pairs of the ring by some 1e-9: at tol = 1e-12 that is far above the value bound,
    and each returned value is its own exact eigenvalue, not its partner's"""
    name, tol = "ring64_1e-6", 1e-12
    G = LC.graph(name)
    ref = LC.graph_spectrum(name, kind, "float64")
    evals, _, _, steps = sess.spectral(_resident(sess, G, G.data), n_eigen=9, kind=kind, tol=tol)
    w = ref["w"][:8]
    rb = tol + 64 * steps * EPS + 64 * EPS
    for p in range(0, 8, 2):
        assert w[p] - w[p + 1] > max(10 * tol, 2 * rb), (p, w[p] - w[p + 1])      # (the fixture: the split can be seen)
        assert abs(evals[1 + p] - w[p]) <= rb and abs(evals[2 + p] - w[p + 1]) <= rb, p


def test_single_round_returns_one_copy_and_is_refused_above_1(sess):
    """single_round = 1 is the single run: on the 64-ring it returns distinct values only (which is why it is not the default)"""
    G = LC.graph("ring64")
    ref = LC.graph_spectrum("ring64", SR.NORMALIZED, "float64")
    R = _resident(sess, G, G.data)
    ev1, _, _, st1 = sess.spectral(R, n_eigen=5, tol=TOL, single_round=True)
    ev, _, _, st = sess.spectral(R, n_eigen=5, tol=TOL)
    distinct = ref["w"][[0, 2, 4, 6]]
    assert np.max(np.abs(ev1[1:] - distinct)) <= TOL + 64 * st1 * EPS + 64 * EPS
    assert np.max(np.abs(ev[1:] - ref["w"][:4])) <= TOL + 64 * st * EPS + 64 * EPS and st > st1
    o = L.default_spectral_options()
    assert o.single_round == 0
    o.single_round = 2
    ev = np.zeros(16)
    E = torch.empty((64, 16), dtype=torch.float64, device="cuda")
    import ctypes as C
    st = L.load().sapca_spectral_device_f64(sess._h, C.c_uint64(64), C.c_uint64(R.nnz), C.c_void_p(R.d_ptr), C.c_void_p(R.d_idx),
                                            C.c_void_p(R.d_val), C.byref(o), ev.ctypes.data_as(C.POINTER(C.c_double)),
                                            C.c_void_p(E.data_ptr()), None, None)
    assert st == 1 and b"single_round = 2 is neither 0 nor 1" in L.load().sapca_last_error(sess._h)

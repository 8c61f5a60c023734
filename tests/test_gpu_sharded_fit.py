"""Row-sharded fits (sapca_multi_*: one process, one thread per member, the in-process transport) at their partition, panel and
collective edges, against a plain f64 reference -- tests/sharded_fit_cases.py: the numpy restatement of the sharded algorithm,
which tests/test_sharded_fit_cases_cpu.py ties to the oracle, and for Lanczos the exact dense SVD.  Never against an unsharded
fit by the library itself, except where a statistic must be the same BYTES on one handle and on any number of members.

Tolerances are the ones the single-handle fits are held to (test_gpu_parity.py):
  f64 randomized   sigma 1e-10   angle 1e-9   scores 1e-9 max|t|   components 1e-8   (test_g4_randomized_fit_injected_omega, test_g7_...)
  f32 randomized   sigma 1e-4    angle 1e-4   scores 2e-3 max|t|
  Lanczos          sigma 1e-5    angle 1e-4   against the exact SVD                  (test_g6_lanczos_uncentred)
Every case has sigma_k / sigma_k+1 >= 1.25 (Lanczos 1.05) by the CPU test, so none of them needs an escape clause.  Each test
prints the figures it asserts."""
import ctypes as C_
import functools

import numpy as np
import pytest

import sapca
import sapca_oracle as O
import sharded_fit_cases as C
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod
from sapca import _lib as L
from sapca._lib import _SUF, _p, as_u64

pytestmark = pytest.mark.gpu

TOL = {"float64": dict(s=1e-10, ang=1e-9, t=1e-9), "float32": dict(s=1e-4, ang=1e-4, t=2e-3)}
VABS64 = 1e-8
LANCZOS_TOL = dict(s=1e-5, ang=1e-4)
GUARD = 64            # sentinel elements either side of a guarded output buffer
SENTINEL = -12345.0


# ------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _matrix(mat, dtype):
    return C.matrix(mat).astype(np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """computed once per operator and partition, shared (and left alone) by every test that needs it"""
    return C.reference_fit(C.BY_NAME[name])


def _estimator(c, centered=False):
    b = sapca.SparsePCABuilder.new() if c.mask is None else sapca.MaskedSparsePCABuilder.new().mask(c.mask)
    b = b.n_components(c.k).center(c.center)
    if c.method == "RANDOM":
        b = b.svd_method(SVDMethod.Random(c.p, c.q, PIN[c.normalizer]))
    else:
        b = b.svd_method(SVDMethod.Lanczos()).lanczos_center(c.lanczos_center)
    if centered or c.scale is not None:
        b = b.transform_semantics(L.TRANSFORM_CENTERED)
    if c.natural_order:
        b = b.spmm_variant(2).collect_timings(True)
    return b.build()


def _prime(est, c):
    if c.method == "RANDOM":
        est.set_omega(c.omega)
    if c.scale is not None:
        est.set_column_scaling(c.scale)
    return est


def _multi(c, nd=None, centered=False):
    return _prime(sapca.MultiDevice(_estimator(c, centered), [0] * (nd or c.nd)), c)


def _guarded(md, op, A):
    """sapca_multi_<op>_csr_* itself into a buffer of NaN between sentinels: every score is written, nothing around them is"""
    m, n = A.shape
    k = md.n_components
    dt = np.dtype(A.dtype)
    suf, ct = _SUF[dt]
    buf = np.full(GUARD + m * k + GUARD, np.nan, dtype=dt)
    buf[:GUARD] = buf[GUARD + m * k:] = SENTINEL
    out = buf[GUARD:GUARD + m * k]
    ro, ci, va = as_u64(A.indptr), as_u64(A.indices), np.ascontiguousarray(A.data)
    md._resident = None
    md._check(getattr(L.load(), f"sapca_multi_{op}_csr_{suf}")(
        md._mh, C_.c_uint64(m), C_.c_uint64(n), C_.c_uint64(va.size), _p(ro, C_.c_uint64), _p(ci, C_.c_uint64), _p(va, ct), _p(out, ct)))
    for mem in md._members:
        mem._dtype64 = dt == np.float64
    assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[GUARD + m * k:] == SENTINEL), "written outside the m x k scores"
    unwritten = np.flatnonzero(np.isnan(out.reshape(m, k)).any(axis=1))
    assert unwritten.size == 0, f"rows never written: {unwritten[:8].tolist()} ..."
    return out.reshape(m, k).copy()


def _state(md, c, dt):
    """the fitted state of every member, as bytes; all members must hold the same"""
    states = []
    for i in range(len(md.devices)):
        mem = md.member(i)
        st = [mem.components_(dt).tobytes(), mem.singular_values_(dt).tobytes(), mem.mean_(dt).tobytes(), mem.mean_(np.float64).tobytes(),
              mem.explained_variance_(dt).tobytes(), np.float64(mem.total_variance_()).tobytes()]
        if c.mask is not None:
            cols, o2m = mem.mask_index_maps()
            st += [cols.tobytes(), o2m.tobytes()]
        states.append(tuple(st))
    for i, st in enumerate(states[1:], 1):
        assert st == states[0], f"member {i} holds another model than member 0"
    return states[0]


def _fit_errors(est, s_ref, vt_ref):
    ds = float(np.max(np.abs(est.singular_values_(np.float64) / s_ref - 1)))
    return ds, O.subspace_angle(est.components_(np.float64), vt_ref)


def _expected_scores(c, A, est, ref, centered):
    """the projection of the WHOLE matrix with the fitted components and mean (as test_g7_transform_reference_semantics does)"""
    comps, mean = est.components_(np.float64), est.mean_(np.float64)
    A64 = A.astype(np.float64)
    m, n = A64.shape
    ptr, idx = A64.indptr.astype(np.int64), A64.indices.astype(np.int64)
    if centered or c.scale is not None:
        D = A64.toarray() - (mean[None, :] if c.center else 0.0)
        D = D if c.mask is None else D[:, c.mask]
        return (D if ref.scale is None else D * ref.scale) @ comps.T
    if c.mask is None:
        return O.transform_sparse(ptr, idx, A64.data, m, n, comps, mean, c.center)
    return O.transform_masked_fast(ptr, idx, A64.data, m, n, comps, mean, c.center, c.mask)


def _score_error(t, want):
    return float(np.abs(t - want).max() / max(1.0, np.abs(want).max()))


def _check_statistics(md, c, ref, dt):
    """what must be exact: the inputs are integers whose sums are exact in f64 and f32, so no summation order changes them"""
    mean = md.mean_(np.float64)
    want = ref.mean if dt == np.float64 else ref.mean.astype(np.float32).astype(np.float64)
    assert mean.tobytes() == want.tobytes(), "mean_: not the one division of an exact sum"
    if c.mask is not None:
        cols, o2m = md.mask_index_maps()
        wc, wo = O.mask_index_maps(c.mask)
        assert np.array_equal(cols, wc) and np.array_equal(o2m, wo)
    tv = md.total_variance_()
    if not c.center:
        # engine.cpp, finish_fit: the f64 sum, in order, of the k explained variances the getter returns -- the same bytes; against
        # the reference it carries twice the relative error of sigma.  (No byte identity with one handle here: its sigma differ
        # in rounding, the panels of a sharded fit have another leading dimension.)
        assert np.float64(tv).tobytes() == np.float64(functools.reduce(lambda a, b: a + b, md.explained_variance_(np.float64), 0.0)).tobytes()
        np.testing.assert_allclose(tv, ref.total_var, rtol=2 * TOL[dt.name]["s"])
    elif c.scale is None:
        np.testing.assert_allclose(tv, ref.total_var, rtol=1e-12)
    else:
        # sum_j d_j^2 var_j on the device, from sums that are exact here.  ss_j = sumsq - sum^2 / m loses sumsq / ss to the one
        # subtraction, in d_j and in var_j alike: a term is within (3 + 3 * 2) eps sumsq / ss of its value for those, plus 8 eps
        # for the divisions, the root and the products; adding n_used terms in any order costs at most n_used eps of the sum
        D = c.A.toarray()
        s1, s2 = D.sum(0), (D * D).sum(0)
        ss = s2 - s1 * s1 / D.shape[0]
        live = ref.scale > 0
        bound = (9 * float((s2[live] / ss[live]).max()) + 8 + c.n_used) * C.EPS64
        print(f"  total variance (scaled): {tv!r} against {ref.total_var!r}, bound {bound:.2e} relative")
        assert abs(tv - ref.total_var) <= bound * ref.total_var and abs(ref.total_var - np.count_nonzero(live)) <= bound * ref.total_var


# ------------------------------------------------------------------------------------------ the partition
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("mat,nd", sorted({(c.mat, c.nd) for c in C.CASES}))
def test_resident_shards_are_the_partition(mat, nd, dtype):
    A = _matrix(mat, dtype)
    md = sapca.MultiDevice(sapca.SparsePCABuilder.new().n_components(2).svd_method(SVDMethod.Random(2, 1)).build(), [0] * nd)
    md.upload(A)
    b = C.partition(A.indptr, nd)
    got = [md.resident_shard(i) for i in range(nd)]
    want = [(int(b[i]), int(b[i + 1] - b[i]), int(A.indptr[b[i + 1]] - A.indptr[b[i]])) for i in range(nd)]
    assert got == want


# ------------------------------------------------------------------------------------------ randomized fits
@pytest.mark.parametrize("name,dtype", [(c.name, dt) for c in C.PLAIN for dt in c.dtypes])
def test_randomized_sharded_fit(name, dtype):
    c, dt, tol = C.BY_NAME[name], np.dtype(dtype), TOL[dtype]
    A, ref = _matrix(c.mat, dtype), _reference(name)
    md = _multi(c)
    assert not md.uses_rccl()
    t = _guarded(md, "fit_transform", A)
    state = _state(md, c, dt)
    ds, ang = _fit_errors(md, ref.singular_values, ref.components)
    want_t = _expected_scores(c, A, md, ref, False)
    et = _score_error(t, want_t)
    print(f"\n{name} {dtype}: sigma {ds:.2e} (tol {tol['s']:.0e})  angle {ang:.2e} ({tol['ang']:.0e})  scores {et:.2e} ({tol['t']:.0e})")
    assert ds <= tol["s"] and ang < tol["ang"] and et <= tol["t"]
    if dt == np.float64 and c.scale is None:
        np.testing.assert_allclose(md.components_(np.float64), ref.components, atol=VABS64)     # signs: svd_flip
    np.testing.assert_allclose(md.explained_variance_(np.float64), ref.singular_values ** 2 / (A.shape[0] - 1), rtol=2 * tol["s"])
    _check_statistics(md, c, ref, dt)

    # the same bytes on one handle that fits the whole matrix: mean and total variance
    one = _prime(_estimator(c), c)
    one.fit(A)
    assert md.mean_(np.float64).tobytes() == one.mean_(np.float64).tobytes()
    if c.center:        # (scaled, too: the same reduction over the same all-reduced, exact sums.  Uncentred: see _check_statistics)
        assert np.float64(md.total_variance_()).tobytes() == np.float64(one.total_variance_()).tobytes()

    # the same call again: the same bytes
    t_again = _guarded(md, "fit_transform", A)
    assert t_again.tobytes() == t.tobytes() and _state(md, c, dt) == state

    # fit, then transform (f32: the small SVD is not held back here)
    md.fit(A)
    ds2, ang2 = _fit_errors(md, ref.singular_values, ref.components)
    t_sep = _guarded(md, "transform", A)
    e_sep = _score_error(t_sep, want_t)
    _state(md, c, dt)
    print(f"  fit + transform: sigma {ds2:.2e}  angle {ang2:.2e}  scores {e_sep:.2e}  against fit_transform {_score_error(t_sep, t):.2e}")
    assert ds2 <= tol["s"] and ang2 < tol["ang"] and e_sep <= tol["t"] and _score_error(t_sep, t) <= tol["t"]

    # resident shards of the same MultiDevice
    md.upload(A)
    t_res = md.fit_transform_resident()
    ds3, ang3 = _fit_errors(md, ref.singular_values, ref.components)
    same = t_res.tobytes() == t.tobytes() and _state(md, c, dt) == state
    print(f"  resident: sigma {ds3:.2e}  angle {ang3:.2e}  scores {_score_error(t_res, want_t):.2e}  bytes of the host call: {same}")
    assert ds3 <= tol["s"] and ang3 < tol["ang"] and _score_error(t_res, want_t) <= tol["t"]
    assert md.mean_(np.float64).tobytes() == one.mean_(np.float64).tobytes()
    md.fit_resident()
    assert _score_error(md.transform_resident(), want_t) <= tol["t"]

    # the centred projection (A - 1 mu^T) V^T
    if c.scale is None:
        mdc = _multi(c, centered=True)
        tc = _guarded(mdc, "fit_transform", A)
        ec = _score_error(tc, _expected_scores(c, A, mdc, ref, True))
        print(f"  centred semantics: scores {ec:.2e}")
        assert ec <= tol["t"] and _state(mdc, c, dt)[1] == state[1]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_statistics_are_the_same_bytes_for_every_member_count(dtype):
    c = C.BY_NAME["a_balanced_nd2"]
    A, ref = _matrix(c.mat, dtype), _reference(c.name)
    one = _prime(_estimator(c), c)
    one.fit(A)
    want = (one.mean_(np.float64).tobytes(), np.float64(one.total_variance_()).tobytes())
    for nd in (1, 2, 3, 4, 7):
        md = _multi(c, nd)
        md.fit(A)
        assert (md.mean_(np.float64).tobytes(), np.float64(md.total_variance_()).tobytes()) == want, f"{nd} members"
        _check_statistics(md, c, ref, np.dtype(dtype))


# ------------------------------------------------------------------------------------------ the A^T sweep in two pieces
@pytest.mark.parametrize("name", [c.name for c in C.TWO_PIECE])
def test_two_piece_transposed_sweep(name, debug_switches, monkeypatch):
    """f32, the DPP-fed sweep, rows in natural order.  A panel of ld 64 is swept in two pieces and the members agree on the cut
    by vote; a panel of ld 128 (l in (64, 128]) is not the format's own width (spmm_tiled_pieces_ok), every member votes 0 and
    the sweep stays whole -- both against the same reference."""
    c, dt, tol = C.BY_NAME[name], np.dtype(np.float32), TOL["float32"]
    A, ref = _matrix(c.mat, "float32"), _reference(name)
    monkeypatch.setenv("SAPCA_NO_ROWSORT", "1")
    expect = 2 if c.l <= 64 else 1
    res = {}
    for overlap in ("1", "0"):
        monkeypatch.setenv("SAPCA_AT_OVERLAP", overlap)
        md = _multi(c)
        t = _guarded(md, "fit_transform", A)
        pieces = [int(md.member(i).timings().at_sweep_pieces) for i in range(c.nd)]
        kernel = [int(md.member(i).timings().sweep_kernel) for i in range(c.nd)]
        assert kernel == [2] * c.nd, kernel
        assert pieces == [expect if overlap == "1" else 1] * c.nd, pieces
        _state(md, c, dt)
        ds, ang = _fit_errors(md, ref.singular_values, ref.components)
        et = _score_error(t, _expected_scores(c, A, md, ref, False))
        print(f"\n{name} overlap {overlap}: pieces {pieces}  sigma {ds:.2e} ({tol['s']:.0e})  angle {ang:.2e} ({tol['ang']:.0e})  scores {et:.2e} ({tol['t']:.0e})")
        assert ds <= tol["s"] and ang < tol["ang"] and et <= tol["t"]
        _check_statistics(md, c, ref, dt)
        res[overlap] = md.singular_values_(np.float64)
    np.testing.assert_allclose(res["1"], res["0"], rtol=tol["s"])


# ------------------------------------------------------------------------------------------ Lanczos
@pytest.mark.parametrize("name,dtype", [(c.name, dt) for c in C.LANCZOS for dt in c.dtypes])
def test_lanczos_with_wide_shards_of_a_tall_matrix(name, dtype):
    c, dt = C.BY_NAME[name], np.dtype(dtype)
    A = _matrix(c.mat, dtype)
    s, vt = C.exact_svd(name)
    md = _multi(c)
    t = _guarded(md, "fit_transform", A)
    state = _state(md, c, dt)
    ds, ang = _fit_errors(md, s[:c.k], vt[:c.k])
    print(f"\n{name} {dtype}: sigma {ds:.2e} (tol {LANCZOS_TOL['s']:.0e})  angle {ang:.2e} ({LANCZOS_TOL['ang']:.0e})  "
          f"steps {md.member(0).timings().lanczos_steps}")
    assert ds <= LANCZOS_TOL["s"] and ang < LANCZOS_TOL["ang"]
    comps = md.components_(np.float64)
    assert np.all(comps[np.arange(c.k), np.argmax(np.abs(comps), 1)] > 0)                    # svd_flip
    D = A.astype(np.float64).toarray()
    mean = D.mean(0)
    assert md.mean_(np.float64).tobytes() == (mean if dt == np.float64 else mean.astype(np.float32).astype(np.float64)).tobytes()
    if c.mask is not None:
        cols, o2m = md.mask_index_maps()
        wc, wo = O.mask_index_maps(c.mask)
        assert np.array_equal(cols, wc) and np.array_equal(o2m, wo)
    assert _guarded(md, "fit_transform", A).tobytes() == t.tobytes() and _state(md, c, dt) == state


# ------------------------------------------------------------------------------------------ refusals
def test_sharded_lanczos_refuses_a_wide_matrix_and_fits_the_next():
    """n > m_global: every member reaches the same check behind the same collectives (lanczos.hip, "row-sharded Lanczos needs
    n_features <= n_samples"), so nobody is left in one"""
    c = C.BY_NAME["j_lanczos_float64_all"]
    wide = _matrix("short_30", "float64")
    md = _multi(c)
    with pytest.raises(L.SapcaError, match=r"row-sharded Lanczos needs n_features <= n_samples \(iteration on A\^T A\)") as e:
        md.fit(wide)
    assert e.value.status == L.ERR_ARG
    A = _matrix(c.mat, "float64")
    md.fit(A)
    s, vt = C.exact_svd(c.name)
    ds, ang = _fit_errors(md, s[:c.k], vt[:c.k])
    assert ds <= LANCZOS_TOL["s"] and ang < LANCZOS_TOL["ang"]


def test_fewer_rows_than_members_is_refused():
    c = C.BY_NAME["a_balanced_nd3"]
    md = _multi(c)
    A = _matrix(c.mat, "float64")
    for op in ("fit", "fit_transform", "upload"):
        with pytest.raises(L.SapcaError, match="fewer rows than devices") as e:
            getattr(md, op)(A[:2])
        assert e.value.status == L.ERR_ARG
    assert _guarded(md, "fit_transform", A).shape == (A.shape[0], c.k)


def test_resident_transform_in_the_other_value_type_is_refused():
    c = C.BY_NAME["a_balanced_nd2"]
    md = _multi(c)
    A = _matrix(c.mat, "float32")
    md.upload(A)
    t = md.fit_transform_resident()
    lib = L.load()
    out = np.full((A.shape[0], c.k), np.nan)
    for fn in (lib.sapca_multi_transform_resident_f64, lib.sapca_multi_fit_transform_resident_f64):
        st = fn(md._mh, _p(out, C_.c_double))
        assert st == L.ERR_ARG and b"the resident matrix has the other value type" in lib.sapca_multi_last_error(md._mh)
    assert np.isnan(out).all()
    assert _score_error(md.transform_resident(), t) <= TOL["float32"]["t"]

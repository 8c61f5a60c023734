"""One handle, many calls (-m gpu): every step of the chains of tests/handle_reuse_cases.py runs on ONE estimator, in buffers,
flags and streams that the steps before it have used, and must give what a fresh handle gives for that step alone.

Primary check: the oracle -- O.fit with the same injected Omega, the covariate and column-scaling restatements, the exact dense
SVD for Lanczos -- at the tolerances of test_gpu_parity.py (sigma 1e-4 / 1e-7, angle 1e-4 / 1e-5, mean 1e-5 / 1e-12,
projection 2e-4 / 1e-9 of its scale), test_gpu_covariates.py / test_gpu_column_scaling.py (explained variance 3 sigma-rtol,
total variance 1e-5 / 1e-12 of the raw second moment, the factor bound) and test_gpu_lanczos_centred.py (sigma 1e-5 / 2e-4,
angle 1e-4 / 2e-3).  None is new and none is loosened, with two things said in full.  The bound on a mean is that of
test_gpu_covariates.py and test_gpu_column_scaling.py, max(1e-5 / 1e-12, 2^-24 / 2^-53 of |mean|): the second term is half an
ulp of the stored mean and only exceeds the first for |mean| > 167 in f32, i.e. in the columns of 1000 +- 0.01 of chain M's
heavy step (6e-5 there), where f32 cannot hold the mean to 1e-5; its absolute term is multiplied by the step's power-of-two
scale (2^40 for the early big matrix: the scaling is exact in f32 and f64, so every error scales with it).  And the heavy
step's scores are held to the 1e-5 of their scale of the fixture it is scaled down from
(test_masked_projection_keeps_its_digits_in_well_filled_columns_of_small_spread), not to the general 2e-4: that is the bar
a stale q3_cancels flag -- the two-sweep projection where the entry loop is due -- would miss.
Secondary check: the bytes of everything the model exposes equal the fresh handle's (fits are reproducible: fixed-order
reductions throughout).  tests/test_handle_reuse_cases_cpu.py certifies the gaps and the widths the chains walk."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import column_scaling_ref as SR
import covariates_ref as CR
import handle_reuse_cases as H
import sapca
import sapca_oracle as O
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod, synth
from sapca import _lib as L
from sapca import ops

pytestmark = pytest.mark.gpu

EPS = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
SIGMA_RTOL = {np.float32: 1e-4, np.float64: 1e-7}
ANGLE = {np.float32: 1e-4, np.float64: 1e-5}
MEAN_ATOL = {np.float32: 1e-5, np.float64: 1e-12}
TV_RTOL = {np.float32: 1e-5, np.float64: 1e-12}
PROJ_ATOL = {np.float32: 2e-4, np.float64: 1e-9}
FI_ATOL = {np.float32: 5e-4, np.float64: 1e-8}                    # test_g4_randomized_fit_injected_omega
LANCZOS_TOL = {np.float64: (1e-5, 1e-4), np.float32: (2e-4, 2e-3)}
NORM = {"QR": PIN.QR, "LU": PIN.LU, "NONE": PIN.NONE}
ENV = ("SAPCA_NO_ROWSORT", "SAPCA_ROWSORT_ALWAYS", "SAPCA_TILED_MIN_ENTRIES", "SAPCA_LANCZOS_TRANSPOSE")


# ------------------------------------------------------------------ running a step
def _estimator(cfg, mask=None, collect_timings=False):
    b = sapca.MaskedSparsePCABuilder.new().mask(mask) if cfg["masked"] else sapca.SparsePCABuilder.new()
    method = SVDMethod.Lanczos() if cfg["method"] == "lanczos" else SVDMethod.Random(cfg["p"], cfg["q"], NORM[cfg["norm"]])
    b = b.n_components(cfg["k"]).center(cfg["center"]).spmm_variant(cfg["variant"]).svd_method(method)
    if cfg["semantics"] == "centred":
        b = b.transform_semantics(L.TRANSFORM_CENTERED)
    if cfg["lanczos_center"]:
        b = b.lanczos_center()
    if collect_timings:
        b = b.collect_timings(True)
    return b.build()


def _set_mask(est, mask):
    m8 = np.ascontiguousarray(mask, dtype=np.uint8)
    L.check(est._h, L.load().sapca_set_mask(est._h, m8.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(m8.size)))
    est._mask = np.asarray(mask, dtype=bool).copy()


def _device(A):
    t = torch.float64 if A.dtype == np.float64 else torch.float32
    return sapca.DeviceCsr(torch.from_numpy(A.indptr.astype(np.int64)).cuda(), torch.from_numpy(A.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(A.data.copy()).to(t).cuda(), A.shape)


def _input(est, A, entry, keep):
    if entry == "host":
        return A
    if entry == "device":
        x = _device(A)
        keep.append(x)
        return x
    s = est.session()                          # resident: the estimator's own handle holds the matrix
    res = s.upload(A.indptr, A.indices, A.data, *A.shape)
    keep.append((s, res))
    return res.as_device_csr()


def _host(t):
    return None if t is None else t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _run(est, name, i, monkeypatch, state):
    """step i on `est`: setters, then the call.  Returns {"scores": ..., "scores_other": ...} (host arrays or None).
    state: what outlives a step (the resident input a later step reuses, tensors that must stay alive)."""
    ch = H.CHAINS[name]
    st, cfg, mk = ch.steps[i], ch.cfg, H.made(name, i)
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    for key, v in st.env.items():
        monkeypatch.setenv(key, v)
    if cfg["masked"]:
        _set_mask(est, mk.mask)
    if cfg["method"] == "random":
        est.set_omega(mk.omega)
    if st.call != "remask_transform":
        est.set_covariates(mk.Z)
        est.set_column_scaling(mk.scaling_arg)
    if st.reuse_input and state.get("x") is not None:
        x = state["x"]
    else:
        x = _input(est, mk.A, st.entry, state.setdefault("keep", []))
    state["x"] = x
    out = {"scores": None, "scores_other": None}
    if st.call == "fit":
        est.fit(x)
    elif st.call == "fit_transform":
        out["scores"] = _host(est.fit_transform(x))
    elif st.call == "fit+transform":
        est.fit(x)
        out["scores"] = _host(est.transform(x))
    elif st.call == "fit+transform_other":
        est.fit(x)
        out["scores_other"] = _host(est.transform(_input(est, mk.other, "host" if st.entry == "host" else "device", state["keep"])))
    elif st.call == "remask_transform":
        out["scores"] = _host(est.transform(x))
    else:
        raise ValueError(st.call)
    return out


def _fresh(name, i, monkeypatch, collect_timings=False):
    """a new handle that runs only step i (a remask_transform needs the fit before it)"""
    ch = H.CHAINS[name]
    first = i - 1 if ch.steps[i].call == "remask_transform" else i
    est = _estimator(ch.cfg, H.made(name, first).mask, collect_timings)
    state, out = {}, None
    for j in range(first, i + 1):
        out = _run(est, name, j, monkeypatch, state)
    return est, out, state


def _model(est, cfg):
    """everything the fitted model exposes, as arrays"""
    dt = est._fitted_dtype()
    out = {
        "components": est.components_(), "singular_values": est.singular_values_(), "explained_variance": est.explained_variance_(),
        "explained_variance_ratio": est.explained_variance_ratio(), "cumulative_ratio": est.cumulative_explained_variance_ratio(),
        "mean": est.mean_(), "mean64": est.mean_(np.float64), "total_variance": np.float64(est.total_variance_()),
        "feature_importances": est.feature_importances(), "covariate_rank": np.int64(est.covariate_rank_),
    }
    assert out["components"].dtype == dt
    d = est.column_scale_
    out["column_scale"] = np.zeros(0) if d is None else d
    out["has_column_scale"] = np.bool_(d is not None)
    if cfg["masked"]:
        out["cols_to_use"], out["orig_to_masked"] = est.mask_index_maps()
    return out


def _same_bytes(got, want, note):
    for key in want:
        a, b = got[key], want[key]
        if a is None and b is None:
            continue
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, f"{note}: {key} {a.shape} {a.dtype} against {b.shape} {b.dtype}"
        if a.tobytes() != b.tobytes():
            diff = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
            first = int(diff[0]) if diff.size else -1
            raise AssertionError(f"{note}: {key} differs from the fresh handle's in {diff.size} of {a.size} elements; first at {first}: "
                                 f"{a.reshape(-1)[first]!r} against {b.reshape(-1)[first]!r}")


# ------------------------------------------------------------------ the oracle
@functools.lru_cache(maxsize=None)
def _expected(name, i):
    """the reference of step i, computed once and shared (read-only): a FitResult-like tuple"""
    ch = H.CHAINS[name]
    st, cfg, mk = ch.steps[i], ch.cfg, H.made(name, i)
    k = cfg["k"]
    if cfg["method"] == "lanczos":
        _, s, vt = np.linalg.svd(H.operator_seen(name, i), full_matrices=False)
        return s[:k], vt[:k], None, None, None
    B = mk.A64 if mk.d is None else SR.prescaled(mk.A64, mk.d)
    kw = dict(n_components=k, n_oversamples=cfg["p"], n_power_iterations=cfg["q"], normalizer=cfg["norm"], center=cfg["center"],
              omega=mk.omega, mask=mk.mask)
    rank = 0
    if mk.Z is not None:
        want, _, rank, _ = CR.expected_fit(B.toarray(), mk.Z, **kw)
    else:
        m, n = B.shape
        want = O.fit(B.indptr.astype(np.int64), B.indices.astype(np.int64), B.data, m, n, **kw)
    return want.singular_values[:k], want.components, want, rank, O.explained_variance_ratio(want.explained_variance)


def _scores_want(name, i, model, other=False):
    """the projection the semantics of the chain define, from the FITTED components and mean (as test_gpu_parity.py does)"""
    ch = H.CHAINS[name]
    cfg, mk = ch.cfg, H.made(name, i)
    comps, mean = model["components"].astype(np.float64), model["mean64"]
    A = mk.other64 if other else mk.A64
    m, n = A.shape
    ptr, idx, val = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data
    if cfg["semantics"] == "centred":          # (A - 1 mu^T) D V^T, the design regressed out: the operator of the fit, projected
        assert not other
        return H.operator_seen(name, i) @ comps.T
    if cfg["masked"]:
        if ch.steps[i].call != "remask_transform" and i == H.M_HEAVY_STEP and name == "M":
            mean = mean.astype(np.float32).astype(np.float64)          # (the entry loop subtracts the f32 means: as the fixture's test)
        # (a mask re-set after the fit does not reach the model: the projection keeps the columns the fit kept)
        mask = H.made(name, i - 1).mask if ch.steps[i].call == "remask_transform" else mk.mask
        return O.transform_masked_fast(ptr, idx, val, m, n, comps, mean, cfg["center"], mask)
    return O.transform_sparse(ptr, idx, val, m, n, comps, mean, cfg["center"])


def _check_oracle(name, i, model, out, note):
    ch = H.CHAINS[name]
    st, cfg, mk = ch.steps[i], ch.cfg, H.made(name, i)
    dtype, k = st.dtype, cfg["k"]
    m, n = mk.A.shape
    for key in ("scores", "scores_other"):
        if out[key] is not None:
            want = _scores_want(name, i, model, key == "scores_other")
            assert out[key].shape == want.shape and out[key].dtype == dtype, note
            heavy = name == "M" and i == H.M_HEAVY_STEP
            tol = (1e-5 if heavy else PROJ_ATOL[dtype]) * max(1.0, float(np.abs(want).max()))
            print(f"{note} {key}: error / bound {np.abs(out[key] - want).max() / tol:.3f}")
            np.testing.assert_allclose(out[key], want, atol=tol, rtol=0, err_msg=f"{note} {key}")
    if st.call == "remask_transform":
        return
    s_want, vt_want, want, rank, ratio_want = _expected(name, i)
    s_got, comps = model["singular_values"].astype(np.float64), model["components"].astype(np.float64)
    assert comps.shape == (k, mk.n_used) and model["mean"].shape == (n,), note
    ang = O.subspace_angle(comps, vt_want)
    print(f"{note}: sigma rel {np.abs(s_got / s_want - 1).max():.2e} angle {ang:.2e}")
    A64 = mk.A64.toarray()
    mean = A64.mean(axis=0) if cfg["center"] else np.zeros(n)
    bound = np.maximum(MEAN_ATOL[dtype] * mk.scale, (EPS[dtype] * (1 + 1e-6)) * np.abs(mean))
    assert (np.abs(model["mean64"] - mean) <= bound).all(), f"{note} mean"
    np.testing.assert_allclose(model["feature_importances"].astype(np.float64), comps ** 2, atol=FI_ATOL[dtype], err_msg=note)
    if cfg["method"] == "lanczos":
        srel, amax = LANCZOS_TOL[dtype]
        np.testing.assert_allclose(s_got, s_want, rtol=srel, err_msg=note)
        assert ang < amax, (note, ang)
        np.testing.assert_allclose(model["explained_variance"].astype(np.float64), s_want ** 2 / (m - 1), rtol=2 * srel, err_msg=note)
        return
    np.testing.assert_allclose(s_got, s_want, rtol=SIGMA_RTOL[dtype], err_msg=note)
    assert ang < ANGLE[dtype], (note, ang)
    np.testing.assert_allclose(model["feature_importances"].astype(np.float64), vt_want ** 2, atol=FI_ATOL[dtype], err_msg=note)
    np.testing.assert_allclose(model["explained_variance"].astype(np.float64), s_want ** 2 / (m - 1), rtol=3 * SIGMA_RTOL[dtype], err_msg=note)
    np.testing.assert_allclose(model["explained_variance_ratio"].astype(np.float64), ratio_want, atol=1e-5 if dtype == np.float32 else 1e-7,
                               err_msg=note)
    used = slice(None) if mk.mask is None else mk.mask
    d = np.ones(n) if mk.d is None else mk.d
    raw = ((A64[:, used] * d[used]) ** 2).sum() / (m - 1)
    assert abs(float(model["total_variance"]) - want.total_var) <= TV_RTOL[dtype] * raw, f"{note} total variance"
    assert int(model["covariate_rank"]) == rank, note
    if cfg["masked"]:
        assert np.array_equal(model["cols_to_use"], want.cols_to_use) and np.array_equal(model["orig_to_masked"], want.orig_to_masked), note
    if st.scaling is None:
        assert not model["has_column_scale"], note
    elif st.scaling == "weights":
        assert model["column_scale"].tobytes() == np.ascontiguousarray(mk.d[used]).tobytes(), note
    else:
        d_ref, ss, s2 = SR.unit_variance_factors(mk.A64)
        live = d_ref[used] > 0
        got = model["column_scale"]
        assert not got[~live].any(), note
        assert (np.abs(got[live] / d_ref[used][live] - 1) <= SR.factor_bound(m, ss[used][live], s2[used][live])).all(), note


def _chain_estimator(name, collect_timings=False):
    ch = H.CHAINS[name]
    return _estimator(ch.cfg, H.made(name, 0).mask, collect_timings)


# ------------------------------------------------------------------ 1. every step against a fresh handle
@pytest.mark.parametrize("name", list(H.CHAINS))
def test_every_step_of_a_chain_equals_a_fresh_handle(name, request, monkeypatch):
    ch = H.CHAINS[name]
    if ch.debug:                                   # the chains whose steps set a route switch run in the debug build of the library
        request.getfixturevalue("debug_switches")
    est, state = _chain_estimator(name), {}
    for i, st in enumerate(ch.steps):
        note = f"{name}[{i}] {st.recipe} {np.dtype(st.dtype).name} {st.entry} {st.call}"
        out = _run(est, name, i, monkeypatch, state)
        model = _model(est, ch.cfg)
        _check_oracle(name, i, model, out, note)                       # first: the fresh handle may itself get recycled memory
        fresh, fresh_out, fresh_state = _fresh(name, i, monkeypatch)
        _same_bytes(out, fresh_out, note)
        if st.call != "remask_transform":
            _same_bytes(model, _model(fresh, ch.cfg), note)
        del fresh, fresh_state


# ------------------------------------------------------------------ 2. nothing read between the steps
@pytest.mark.parametrize("collect_timings", [False, True])
@pytest.mark.parametrize("name", ["R-row-f32", "M"])
def test_results_not_read_between_steps(name, collect_timings, monkeypatch):
    """fit_transform on every step and no getter until the last one, so that nothing but the calls themselves completes a
    fit.  (In the present engine a fit_transform holds its host tail and, for small unmasked f32 fits, its small SVD back only
    until its own projection is queued -- transform() ends with finish_fit() -- so none outlives the call; the test holds
    whichever way that is arranged.)  collect_timings changes the event bookkeeping, so once more with it."""
    ch = H.CHAINS[name]
    steps = [i for i, st in enumerate(ch.steps) if st.call != "remask_transform"]
    est, state, scores = _chain_estimator(name, collect_timings), {}, {}
    for i in steps:
        st, mk = ch.steps[i], H.made(name, i)
        if ch.cfg["masked"]:
            _set_mask(est, mk.mask)
        est.set_omega(mk.omega)
        x = state["x"] if st.reuse_input else _input(est, mk.A, st.entry, state.setdefault("keep", []))
        state["x"] = x
        scores[i] = _host(est.fit_transform(x))
    last = steps[-1]
    model = _model(est, ch.cfg)
    fresh_model = None
    for i in steps:
        note = f"{name}[{i}] timings {collect_timings}"
        mk = H.made(name, i)
        fresh = _estimator(ch.cfg, mk.mask, collect_timings)
        fresh.set_omega(mk.omega)
        keep = []
        t = _host(fresh.fit_transform(_input(fresh, mk.A, ch.steps[i].entry, keep)))
        fm = _model(fresh, ch.cfg)
        _check_oracle(name, i, fm, {"scores": scores[i], "scores_other": None}, note)     # the chain's scores, the step's own model
        assert scores[i].tobytes() == t.tobytes(), f"{note}: scores differ from a fresh handle's"
        if i == last:
            fresh_model = fm
    _check_oracle(name, last, model, {"scores": None, "scores_other": None}, f"{name}[{last}] model")
    _same_bytes(model, fresh_model, f"{name}[{last}] model")


# ------------------------------------------------------------------ 3. a failed call in the middle
def _good_step(est, name, i, monkeypatch):
    state = {}
    out = _run(est, name, i, monkeypatch, state)
    return out, _model(est, H.CHAINS[name].cfg), state


def _rank_deficient():
    rng = np.random.default_rng(3)          # the panel of test_rank_deficient_panel_keeps_the_leading_components
    m, n, r = 1500, 200, 5
    U = rng.standard_normal((m, r)) * np.array([9.0, 7.0, 5.0, 3.0, 2.0])
    A = sp.csr_matrix((U @ rng.standard_normal((r, n))).astype(np.float32))
    A.sort_indices()
    return A


@pytest.mark.parametrize("failure", ["l_below_k", "non_finite_value", "rank_deficient", "empty_mask", "wrong_columns", "disordered_rows"])
def test_a_failed_call_in_the_middle(failure, monkeypatch):
    """a good step, a troublesome call, then a good step that must equal a fresh handle's bytes and pass the oracle.
    Four of the calls are refused, each with the status and message pinned here: l_below_k (after prepare() queued the formats
    and statistics), non_finite_value (after the sweeps, at the small eigenproblem), empty_mask (in prepare()) and
    wrong_columns (in transform(), before any work).  Two are NOT failures and are here for what they leave behind:
    rank_deficient is a fit the library completes -- the Cholesky floors the dead pivots -- and all its k singular values are
    checked; disordered_rows is input outside the contract, for which include/sapca.h promises numbers or a refusal but no
    stray access, exactly as test_rows_whose_columns_do_not_ascend_give_numbers_not_stray_accesses takes it."""
    name = "M" if failure == "empty_mask" else "R-staged-f32" if failure == "disordered_rows" else "R-row-f32"
    ch = H.CHAINS[name]
    before, after = (0, 2) if name == "M" else (0, 1)
    est = _chain_estimator(name)
    _good_step(est, name, before, monkeypatch)
    if failure == "l_below_k":                                          # 9 x 300 with k = 12
        A = sp.csr_matrix(H._recipe(("gapped", 9, 300, 0.5, 7), 12, True)[0].astype(np.float32))
        est.set_omega(synth.gaussian_panel(300, 20, 1).numpy())
        with pytest.raises(L.SapcaError, match="Randomized SVD computation failed") as e:
            est.fit_transform(A)
        assert e.value.status == L.ERR_SVD
    elif failure == "non_finite_value":                                 # one stored inf: every sweep runs, the eigenproblem is refused
        A = sp.csr_matrix(H.made(name, 3).A, copy=True)
        A.data[A.nnz // 2] = np.inf
        est.set_omega(synth.gaussian_panel(A.shape[1], 20, 2).numpy())
        with pytest.raises(L.SapcaError, match="Randomized SVD computation failed: eigensolver did not converge") as e:
            est.fit_transform(A)
        assert e.value.status == L.ERR_SVD
    elif failure == "rank_deficient":                                   # rank 5, k = 12 of l = 20: a fit that succeeds
        A = _rank_deficient()
        est.set_omega(synth.gaussian_panel(200, 20, 2).numpy())
        t = est.fit_transform(A)
        D = A.toarray().astype(np.float64)
        s_ex = np.linalg.svd(D - D.mean(axis=0), compute_uv=False)
        s_got = est.singular_values_(np.float64)
        assert np.isfinite(t).all() and np.isfinite(est.components_(np.float64)).all()
        # the five live values at the f32 figure of test_rank_deficient_panel_keeps_the_leading_components; the seven dead ones
        # are rounding noise on both sides, so they are held to the same figure of the norm (Weyl: a perturbation E of the
        # matrix moves every singular value by at most |E|_2)
        np.testing.assert_allclose(s_got[:5], s_ex[:5], rtol=2e-4)
        assert (np.abs(s_got - s_ex[:12]) <= 2e-4 * s_ex[0]).all(), s_got
    elif failure == "empty_mask":
        mk = H.made(name, 1)
        _set_mask(est, np.zeros(mk.A.shape[1], dtype=bool))
        with pytest.raises(L.SapcaError, match="the mask selects no feature") as e:
            est.fit_transform(mk.A)
        assert e.value.status == L.ERR_SVD
    elif failure == "wrong_columns":                                    # refused on entry: the fitted model must survive it
        A = sp.csr_matrix(H._recipe(("gapped", 50, 333, 0.3, 8), 12, True)[0].astype(np.float32))
        with pytest.raises(L.SapcaError, match="transform: column count differs from the fitted matrix") as e:
            est.transform(A)
        assert e.value.status == L.ERR_ARG
    else:                                                               # rows whose columns descend (test_rows_whose_columns_do_not_ascend)
        m, n = 40_000, 2600
        ptr, idx, val = synth.gapped_csr(m, n, 0.03, 6, seed=11, dtype=torch.float32, device="cuda")
        bad_idx, bad_val, p = idx.clone(), val.clone(), ptr.cpu().numpy()
        for r in (17, 4242, m - 1):
            lo, hi = int(p[r]), int(p[r + 1])
            bad_idx[lo:hi] = torch.flip(idx[lo:hi], dims=[0])
            bad_val[lo:hi] = torch.flip(val[lo:hi], dims=[0])
        est.set_omega(synth.gaussian_panel(n, 43, 3).numpy())
        try:
            t_bad = est.fit_transform(sapca.DeviceCsr(ptr, bad_idx, bad_val, (m, n)))
            assert t_bad.shape == (m, ch.cfg["k"])
            torch.cuda.synchronize()
        except L.SapcaError as err:                                     # (the contract allows a refusal too; a fault it does not)
            assert err.status in (L.ERR_ARG, L.ERR_SVD)
    note = f"{name}[{after}] after {failure}"
    out, model, _ = _good_step(est, name, after, monkeypatch)
    _check_oracle(name, after, model, out, note)
    fresh, fresh_out, _ = _fresh(name, after, monkeypatch)
    _same_bytes(out, fresh_out, note)
    _same_bytes(model, _model(fresh, ch.cfg), note)


# ------------------------------------------------------------------ 4. the same addresses, other contents
def _other_contents(A, seed):
    """a matrix of A's shape and entry count per row, with other columns and other values: A's columns mirrored (the planted
    blocks move with them) and its values redrawn within +-20 %"""
    rng = np.random.default_rng(seed)
    m, n = A.shape
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    B = sp.csr_matrix((A.data * rng.uniform(0.8, 1.2, A.nnz).astype(A.dtype), (rows, n - 1 - A.indices)), shape=(m, n))
    B.sort_indices()
    assert B.nnz == A.nnz and np.array_equal(np.diff(B.indptr), np.diff(A.indptr))
    return B


@pytest.mark.parametrize("case", ["resident", "caller_owned", "mask"])
def test_same_addresses_other_contents(case, monkeypatch):
    """the key of the handle's preparation holds addresses, shape and entry count: other contents under the same key must be
    seen.  Each second fit against the oracle run on what the arrays hold then."""
    k, p, q = 8, 6, 2
    A = sp.csr_matrix(H._recipe(("gapped", 2500, 600, 0.17, 41), k, True)[0].astype(np.float32))
    B = _other_contents(A, 5)
    m, n = A.shape
    masks = [synth.bernoulli_mask(n, 0.6, s).numpy() for s in (3, 9)] if case == "mask" else [None, None]
    b = sapca.MaskedSparsePCABuilder.new().mask(masks[0]) if case == "mask" else sapca.SparsePCABuilder.new()
    est = b.n_components(k).spmm_variant(2).svd_method(SVDMethod.Random(p, q, PIN.QR)).build()

    def check(M, mask, t):
        n_used = n if mask is None else int(mask.sum())
        M64 = M.astype(np.float64)
        ptr, idx, val = M64.indptr.astype(np.int64), M64.indices.astype(np.int64), M64.data
        want = O.fit(ptr, idx, val, m, n, n_components=k, n_oversamples=p, n_power_iterations=q, omega=om(n_used), mask=mask)
        comps, mean = est.components_(np.float64), est.mean_(np.float64)
        np.testing.assert_allclose(est.singular_values_(np.float64), want.singular_values, rtol=1e-4)
        assert O.subspace_angle(comps, want.components) < 1e-4
        np.testing.assert_allclose(mean, want.mean, atol=1e-5)
        tw = (O.transform_sparse(ptr, idx, val, m, n, comps, mean, True) if mask is None
              else O.transform_masked_fast(ptr, idx, val, m, n, comps, mean, True, mask))
        np.testing.assert_allclose(_host(t), tw, atol=2e-4 * max(1.0, float(np.abs(tw).max())))

    def om(n_used):
        return synth.gaussian_panel(n_used, k + p, 77).numpy()

    if case == "resident":
        s = est.session()
        ra = s.upload(A.indptr, A.indices, A.data, m, n)
        check(A, None, est.set_omega(om(n)).fit_transform(ra.as_device_csr()))
        rb = s.upload(B.indptr, B.indices, B.data, m, n)
        assert (rb.d_ptr, rb.d_idx, rb.d_val) == (ra.d_ptr, ra.d_idx, ra.d_val)            # the same addresses
        check(B, None, est.fit_transform(rb.as_device_csr()))
    elif case == "caller_owned":
        x = _device(A)
        check(A, None, est.set_omega(om(n)).fit_transform(x))
        y = _device(B)
        addresses = (x.row_offsets.data_ptr(), x.col_indices.data_ptr(), x.values.data_ptr())
        x.row_offsets.copy_(y.row_offsets)
        x.col_indices.copy_(y.col_indices)
        x.values.copy_(y.values)
        torch.cuda.synchronize()
        assert addresses == (x.row_offsets.data_ptr(), x.col_indices.data_ptr(), x.values.data_ptr())
        check(B, None, est.fit_transform(x))
    else:
        s = est.session()
        ra = s.upload(A.indptr, A.indices, A.data, m, n)
        x = ra.as_device_csr()
        check(A, masks[0], est.set_omega(om(int(masks[0].sum()))).fit_transform(x))
        _set_mask(est, masks[1])
        check(A, masks[1], est.set_omega(om(int(masks[1].sum()))).fit_transform(x))
        cols, o2m = est.mask_index_maps()
        want_cols, want_o2m = O.mask_index_maps(masks[1])
        assert np.array_equal(cols, want_cols) and np.array_equal(o2m, want_o2m)


# ------------------------------------------------------------------ 5. a fit after every other operator family
def test_a_fit_after_every_other_operator_family(monkeypatch):
    """everything on est.session(), which borrows the estimator's handle and its scratch buffers: the operators' own results
    are tested elsewhere; here only that they leave nothing behind that a fit reads"""
    name = "R-row-f32"
    ch = H.CHAINS[name]
    k = ch.cfg["k"]
    first = sp.csr_matrix(H._recipe(("gapped", 1500, 400, 0.12, 71), k, True)[0].astype(np.float32))
    small = sp.csr_matrix(H._recipe(("gapped", 700, 150, 0.15, 72), k, True)[0].astype(np.float32))
    oms = {id(first): synth.gaussian_panel(400, 20, 5).numpy(), id(small): synth.gaussian_panel(150, 20, 6).numpy()}

    def fit(est, M):
        est.set_omega(oms[id(M)])
        t = est.fit_transform(_device(M))
        return _host(t), _model(est, ch.cfg)

    def oracle(M, t, model, note):
        m, n = M.shape
        M64 = M.astype(np.float64)
        ptr, idx, val = M64.indptr.astype(np.int64), M64.indices.astype(np.int64), M64.data
        want = O.fit(ptr, idx, val, m, n, n_components=k, n_oversamples=ch.cfg["p"], n_power_iterations=ch.cfg["q"], omega=oms[id(M)])
        comps = model["components"].astype(np.float64)
        np.testing.assert_allclose(model["singular_values"].astype(np.float64), want.singular_values, rtol=1e-4, err_msg=note)
        assert O.subspace_angle(comps, want.components) < 1e-4, note
        np.testing.assert_allclose(model["mean64"], want.mean, atol=1e-5, err_msg=note)
        tw = O.transform_sparse(ptr, idx, val, m, n, comps, model["mean64"], True)
        np.testing.assert_allclose(t, tw, atol=2e-4 * max(1.0, float(np.abs(tw).max())), err_msg=note)

    est = _estimator(ch.cfg)
    est.set_omega(oms[id(first)])
    scores = est.fit_transform(_device(first))                          # stays on the device: the operators search it in place
    s = est.session()
    idx, dist = s.knn(scores, n_neighbors=10)[:2]
    s.kmeans(scores, n_clusters=4, max_iter=5)
    s.tsne(scores, perplexity=5.0, epochs=20)
    s.umap(scores, n_neighbors=10, n_epochs=20)
    G = s.umap_graph(idx, dist, 11)[0]
    s.louvain(G, max_sweeps=8)
    s.spectral(G, n_eigen=4)
    res = s.upload(first.indptr, first.indices, first.data, *first.shape)
    labels = np.arange(first.shape[0]) % 3
    res.rank_groups(labels, n_groups=3)
    res.highly_variable(n_top=50)
    res.masked_stats(ops.COLUMN, np.arange(first.shape[0]) % 2 == 0)
    res.batch_stats(0, labels, 3)
    res.canonicalize()
    for M, note in ((small, "smaller matrix"), (first, "the first matrix again")):
        t, model = fit(est, M)
        oracle(M, t, model, note)
        t_fresh, model_fresh = fit(_estimator(ch.cfg), M)
        assert t.tobytes() == t_fresh.tobytes(), f"{note}: scores differ from a fresh handle's"
        _same_bytes(model, model_fresh, note)

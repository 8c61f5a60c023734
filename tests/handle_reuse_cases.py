"""Chains of calls on ONE handle, as data: what tests/test_gpu_handle_reuse.py runs and tests/test_handle_reuse_cases_cpu.py
certifies (no GPU needed here: numpy, scipy and the synthetic generators only).

A chain is a handle configuration, fixed at sapca_create, and an ordered list of steps.  A step is a matrix recipe, a
dtype, the entry point (host: scipy CSR; device: caller-owned DeviceCsr; resident: Session.upload on the estimator's own
handle), a call (fit, fit_transform, fit then transform of the same matrix, fit then transform of another matrix, or a
transform under a re-set mask) and the setters in force (Omega always; mask, covariates, column scaling).

Matrices are synth.gapped_csr with its planted clusters, sometimes edited (empty rows, a full row, thinned rows, stored
zeros, fully stored columns of small spread); the CPU test asserts sigma_k / sigma_{k+1} >= 2 of the operator each fit sees.
One early matrix of every chain is multiplied by 2^40 (exact in f32 and f64): what it leaves in the handle's buffers is
gross, not subtle, where a later and smaller step reads it.

panel_geometry() and staged_floor() RESTATE single-algebra_amd/csrc/engine.cpp:34-44 (staged_sweep_ldp), :128 (panel_ld),
:234-235 (the entries a masked fit counts) and :785-788 (plan_randomized: l and ld).  Whoever changes those lines changes
these two functions, and the walks the chains declare, with them."""
import functools
import math
from collections import namedtuple

import numpy as np
import scipy.sparse as sp
import torch

import column_scaling_ref as SR
import covariates_ref as CR
from sapca import synth

BIG = 2.0 ** 40
F32, F64 = np.float32, np.float64

# call: "fit" | "fit_transform" | "fit+transform" (same matrix) | "fit+transform_other" | "remask_transform" (the mask is
# re-set to another one that keeps as many columns, then the fitted matrix is projected: no fit in this step; the model
# keeps the columns it was fitted on, and the preparation the handle held of the matrix is dropped and made again)
Step = namedtuple("Step", "recipe scale dtype entry call mask cov scaling env other reuse_input")
Chain = namedtuple("Chain", "name cfg steps walk debug")


def step(recipe, dtype=F32, entry="host", call="fit_transform", *, scale=1.0, mask=None, cov=False, scaling=None, env=None, other=None,
         reuse_input=False):
    return Step(tuple(recipe), float(scale), dtype, entry, call, mask, bool(cov), scaling, dict(env or {}), other, bool(reuse_input))


def config(k, p, q=2, *, method="random", norm="QR", center=True, variant=0, masked=False, semantics="reference", lanczos_center=False):
    return dict(k=k, p=p, q=q, method=method, norm=norm, center=center, variant=variant, masked=masked, semantics=semantics,
                lanczos_center=lanczos_center)


# ------------------------------------------------------------------ matrices
def _gapped(m, n, dens, seed, k, centred):
    ptr, idx, val = (x.numpy() for x in synth.gapped_csr(m, n, dens, k, seed=seed, centred=centred, dtype=torch.float64))
    return sp.csr_matrix((val, idx.astype(np.int64), ptr.astype(np.int64)), shape=(m, n))


def _from_dense(D, S):
    r, c = np.nonzero(S)
    A = sp.csr_matrix((D[r, c], (r, c)), shape=D.shape)
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def _recipe(recipe, k, centred):
    """the f64 scipy CSR of a recipe (and the covariates that belong to it, or None)"""
    kind = recipe[0]
    Z = None
    if kind == "gapped":                      # (m, n, density, seed)
        A = _gapped(*recipe[1:5], k, centred)
    elif kind == "solid":                     # every entry of the planted blocks stored: the clusters stand out at tiny shapes too
        m, n, dens, seed = recipe[1:5]
        A = _gapped(m, n, dens, seed, k, centred)
        c = max(1, min(k + 1 if centred else k, n))          # the generator's own cluster rule (synth.gapped_csr)
        rows = torch.arange(m, dtype=torch.int64)
        row_cluster = (synth.hash_u01(seed, 1, rows) * c).to(torch.int64).clamp_(max=c - 1).numpy()
        col_cluster = (np.arange(n) * c) // n
        w = 12.0 * (7.0 / 12.0) ** (np.arange(c) / max(1, c - 1))
        D = A.toarray()
        add = (row_cluster[:, None] == col_cluster[None, :]) & (D == 0)
        fill = w[row_cluster][:, None] * (0.5 + np.random.default_rng(seed).random((m, n)))
        D[add] = fill[add]
        A = _from_dense(D, D != 0)
    elif kind == "ragged":                  # about 5 % empty rows and one row that stores every column
        m, n, dens, seed = recipe[1:5]
        A = _gapped(m, n, dens, seed, k, centred)
        rng = np.random.default_rng(seed)
        D, S = A.toarray(), A.toarray() != 0
        empty = rng.choice(m, m // 20, replace=False)
        full = int(np.setdiff1d(np.arange(m), empty)[m // 3])
        S[empty] = False
        D[full] = np.where(S[full], D[full], 0.25)
        S[full] = True
        A = _from_dense(D, S)
    elif kind == "lognormal":                 # log-normal row lengths: the planted blocks stay, the background entries (damped
        m, n, dens, seed = recipe[1:5]        # by 1 / 16) are thinned row by row by a log-normal depth
        A, _ = _recipe(("solid", m, n, dens, seed), k, centred)
        rng = np.random.default_rng(seed)
        depth = np.exp(1.5 * rng.standard_normal(m))
        keep = np.minimum(1.0, depth / np.quantile(depth, 0.98))
        rows = np.repeat(np.arange(m), np.diff(A.indptr))
        c = max(1, min(k + 1 if centred else k, n))
        row_cluster = (synth.hash_u01(seed, 1, torch.arange(m, dtype=torch.int64)) * c).to(torch.int64).clamp_(max=c - 1).numpy()
        inblk = row_cluster[rows] == (A.indices.astype(np.int64) * c) // n
        sel = inblk | (rng.random(A.nnz) < keep[rows])
        A = sp.csr_matrix((np.where(inblk, A.data, A.data / 16.0)[sel], (rows[sel], A.indices[sel])), shape=(m, n))
        A.sort_indices()
    elif kind == "heavy":                     # a few columns stored in every row, 1000 + 0.01 N(0, 1): well filled, small spread
        m, n, dens, seed, ncols = recipe[1:6]
        A = _gapped(m, n, dens, seed, k, centred)
        rng = np.random.default_rng(seed)
        D, S = A.toarray(), A.toarray() != 0
        for j in heavy_columns(n, ncols):
            D[:, j] = 1000.0 + 0.01 * rng.standard_normal(m)
            S[:, j] = True
        A = _from_dense(D, S)
    elif kind == "zeros":                     # some stored +0.0 and -0.0
        m, n, dens, seed, count = recipe[1:6]
        A = _gapped(m, n, dens, seed, k, centred)
        z = np.random.default_rng(seed).choice(A.nnz, count, replace=False)
        A.data[z[: count // 2]] = 0.0
        A.data[z[count // 2:]] = -0.0
    elif kind == "covariate":                 # covariates_ref.covariate_case: (m, n, seed, batches, continuous)
        m, n, seed, nb, nc = recipe[1:6]
        A, Z, _ = CR.covariate_case(m, n, seed, nb, nc, centred=centred)
    elif kind == "scaled":                    # column_scaling_ref.scaled_case: (m, n, seed)
        A = SR.scaled_case(*recipe[1:4], centred=centred)
    else:
        raise ValueError(kind)
    A = sp.csr_matrix(A)
    A.sort_indices()
    for x in (A.data, A.indices, A.indptr):
        x.setflags(write=False)
    if Z is not None:
        Z.setflags(write=False)
    return A, Z


def heavy_columns(n, count):
    return [int(j) for j in np.linspace(3, n - 4, count).astype(int)]


Made = namedtuple("Made", "A A64 mask n_used omega Z d scaling_arg other other64 scale")


@functools.lru_cache(maxsize=None)
def _made(chain_name, i):
    ch = CHAINS[chain_name]
    st, cfg = ch.steps[i], ch.cfg
    gen_centred = cfg["center"] if cfg["method"] == "random" else cfg["lanczos_center"]
    base, Z = _recipe(st.recipe, cfg["k"], gen_centred)
    A = sp.csr_matrix(((base.data * st.scale).astype(st.dtype), base.indices.copy(), base.indptr.copy()), shape=base.shape)
    assert A.nnz == base.nnz                  # (stored zeros stay stored)
    A64 = A.astype(np.float64)
    m, n = A.shape
    mask = None
    if st.mask is not None:
        mask = synth.bernoulli_mask(n, st.mask[0], st.mask[1]).numpy().copy()
        if st.call == "remask_transform":     # another mask of as many columns: the fitted one rotated by one kept column
            prev = _made(chain_name, i - 1).mask
            mask = equal_count_mask(prev)
    n_used = int(mask.sum()) if mask is not None else n
    omega = synth.gaussian_panel(n_used, cfg["k"] + cfg["p"], 100 + i).numpy()
    d = scaling_arg = None
    if st.scaling == "unit_variance":         # the library derives d from the values as stored
        d, scaling_arg = SR.unit_variance_factors(A64)[0], "unit_variance"
    elif st.scaling == "weights":             # explicit weights: numpy's factors of the f64 matrix, as the column-scaling tests pass them
        d = SR.unit_variance_factors(sp.csr_matrix(base * st.scale))[0]
        scaling_arg = d
    other = other64 = None
    if st.other is not None:
        ob, _ = _recipe(tuple(st.other), cfg["k"], gen_centred)
        other = sp.csr_matrix((ob.data.astype(st.dtype), ob.indices.copy(), ob.indptr.copy()), shape=ob.shape)
        other64 = other.astype(np.float64)
    return Made(A, A64, mask, n_used, omega, Z if st.cov else None, d, scaling_arg, other, other64, st.scale)


def made(chain_name, i):
    """everything step i of the chain needs, built once and shared (treat as read-only)"""
    return _made(chain_name, i)


def equal_count_mask(mask):
    """a mask that keeps as many columns as `mask`, other ones: its first kept column goes, its first dropped column comes"""
    out = np.array(mask, dtype=bool, copy=True)
    out[np.flatnonzero(mask)[0]] = False
    out[np.flatnonzero(~np.asarray(mask, dtype=bool))[0]] = True
    return out


def operator_seen(chain_name, i):
    """the dense operator the fit of step i factors: kept columns, scaled by d, the design regressed out or the means removed"""
    ch = CHAINS[chain_name]
    cfg, mk = ch.cfg, made(chain_name, i)
    D = mk.A64.toarray()
    centred = cfg["center"] and (cfg["method"] == "random" or cfg["lanczos_center"])
    if mk.d is not None:
        D = D * mk.d
    if mk.Z is not None:
        Q, _ = CR.basis(CR.design(mk.Z, cfg["center"]))
        D = CR.residual(D, Q)
    elif centred:
        D = D - D.mean(axis=0)
    return D if mk.mask is None else D[:, mk.mask]


# ------------------------------------------------------------------ engine.cpp restated
def staged_floor(rows, cols, entries, itemsize, min_entries=None):
    """engine.cpp:34-44 without the variant: is the operator dense and large enough for the LDS-staged sweep?
    min_entries: SAPCA_TILED_MIN_ENTRIES of the debug library (None: 1e7 for f32, 5e6 for f64)"""
    row_bytes = 64.0 * itemsize
    tile_bytes, block_rows = 80.0 * 1024.0, (512.0 if row_bytes == 256.0 else 256.0)
    chunks = math.ceil(rows / block_rows) * math.ceil(cols * row_bytes / tile_bytes)
    floor_entries = (1e7 if itemsize == 4 else 5e6) if min_entries is None else float(min_entries)
    return entries * (64.0 if itemsize == 4 else 96.0) >= chunks * tile_bytes and entries >= floor_entries


def panel_geometry(chain_name, i):
    """(l, ld, route) of step i's randomized fit: engine.cpp:785-788 with :128 and :234-235.  route: "row" or "staged"."""
    ch = CHAINS[chain_name]
    cfg, st, mk = ch.cfg, ch.steps[i], made(chain_name, i)
    m, n = mk.A.shape
    l = min(cfg["k"] + cfg["p"], m, mk.n_used)
    itemsize = np.dtype(st.dtype).itemsize
    entries = mk.A.nnz * (mk.n_used / n)
    floor = st.env.get("SAPCA_TILED_MIN_ENTRIES")
    if cfg["variant"] == 1 or l < 1 or l > 1024:
        tiled = False
    else:
        tiled = cfg["variant"] == 2 or staged_floor(m, mk.n_used, entries, itemsize, floor)
    if l > 128:
        ld = 64 * math.ceil(l / 64)
    elif tiled:
        ld = max(64, 64 if l <= 64 else 128)
    else:
        ld = 16 * math.ceil(l / 16)
    return l, ld, "staged" if tiled else "row"


def lanczos_route(chain_name, i):
    """engine.cpp:250-251: "scatter" (no transposed operator) or "transposed"; and the side the iteration runs on"""
    ch = CHAINS[chain_name]
    st, mk = ch.steps[i], made(chain_name, i)
    m, n = mk.A.shape
    scatter = 0 < mk.n_used <= m and m >= 4096 and mk.A.nnz > 0 and "SAPCA_LANCZOS_TRANSPOSE" not in st.env
    return "scatter" if scatter else "transposed"


def q3_statistic(chain_name, i):
    """max over the kept columns of (sum a)^2 / (m sum a^2): engine.cpp:628 sets q3_cancels where it exceeds 1/4"""
    mk = made(chain_name, i)
    D = mk.A64.toarray()[:, mk.mask]
    s, q = D.sum(axis=0), (D * D).sum(axis=0)
    ok = q > 0
    return float((s[ok] ** 2 / (D.shape[0] * q[ok])).max())


# ------------------------------------------------------------------ the chains
def _r_row(dtypes):
    g = ("gapped", 3000, 700, 0.12, 1)
    d = lambda j: dtypes[j % len(dtypes)]     # noqa: E731
    return [step(g, d(0), "host", "fit_transform", scale=BIG),
            step(("solid", 900, 14, 0.5, 23), d(1), "resident", "fit+transform"),
            step(("solid", 40, 300, 0.5, 12), d(2), "device", "fit_transform"),
            step(("ragged", 2500, 500, 0.12, 4), d(3), "host", "fit+transform_other", other=("gapped", 700, 500, 0.12, 5)),
            step(("solid", 900, 17, 0.5, 15), d(4), "device", "fit"),
            step(g, d(5), "resident", "fit_transform")]


_ROW_WALK = [(20, 32, "row"), (14, 16, "row"), (20, 32, "row"), (20, 32, "row"), (17, 32, "row"), (20, 32, "row")]


def _r_staged(dtype):
    a, b, c, e = ("gapped", 2051, 65, 0.4, 11), ("gapped", 1027, 333, 0.4, 12), ("solid", 37, 1200, 0.2, 13), ("solid", 5, 70, 0.5, 6)
    nosort, sort = {"SAPCA_NO_ROWSORT": "1"}, {"SAPCA_ROWSORT_ALWAYS": "1"}
    return [step(b, dtype, "host", "fit_transform", scale=BIG),          # entry counts descend ...
            step(a, dtype, "device", "fit_transform"),
            step(c, dtype, "resident", "fit+transform"),
            step(e, dtype, "host", "fit_transform"),
            step(c, dtype, "device", "fit_transform"),                   # ... and ascend again
            step(a, dtype, "resident", "fit_transform", env=nosort),
            step(("lognormal", 1000, 300, 0.8, 15), dtype, "host", "fit_transform", env=sort),   # the row sort, between two fits without
            step(b, dtype, "device", "fit+transform", env=nosort)]


_STAGED_WALK = [(43, 64, "staged"), (43, 64, "staged"), (37, 64, "staged"), (5, 64, "staged"), (37, 64, "staged"), (43, 64, "staged"),
                (43, 64, "staged"), (43, 64, "staged")]


def _r_auto():
    env = {"SAPCA_TILED_MIN_ENTRIES": "30000"}
    above, below = ("gapped", 3000, 700, 0.12, 1), ("solid", 700, 260, 0.03, 21)
    return [step(above, F32, "host", "fit_transform", scale=BIG, env=env), step(below, F32, "device", "fit_transform", env=env),
            step(above, F32, "resident", "fit+transform", env=env), step(below, F32, "host", "fit+transform", env=env),
            step(above, F32, "device", "fit_transform", env=env)]


def _r_wide():
    first = ("gapped", 2000, 400, 0.12, 31)
    return [step(first, F32, "host", "fit_transform", scale=BIG), step(("solid", 1500, 50, 0.3, 32), F32, "device", "fit_transform"),
            step(first, F32, "resident", "fit+transform")]


def _masked():
    first = ("gapped", 2500, 600, 0.17, 41)
    return [step(first, F32, "resident", "fit_transform", scale=BIG, mask=(0.9, 1)),
            step(first, F32, "resident", "fit_transform", scale=BIG, mask=(0.2, 2), reuse_input=True),   # the same resident matrix, another mask
            step(("gapped", 1800, 500, 0.17, 42), F32, "host", "fit+transform", mask=(0.6, 3)),
            step(("heavy", 1500, 300, 0.17, 43, 12), F32, "device", "fit_transform", mask=(0.7, 4)),          # sets q3_cancels
            step(("zeros", 1200, 400, 0.17, 44, 300), F32, "host", "fit_transform", mask=(0.6, 5)),
            step(("solid", 1500, 30, 0.3, 9), F32, "device", "fit_transform", mask=(0.45, 4)),                 # 13 kept columns: l = 13 < k + p
            step(("zeros", 1200, 400, 0.17, 44, 300), F32, "resident", "fit_transform", mask=(0.6, 5)),
            step(("zeros", 1200, 400, 0.17, 44, 300), F32, "resident", "remask_transform", mask=(0.6, 5), reuse_input=True)]


def _lanczos(dtype):
    tall = ("gapped", 4500, 600, 0.25, 51)
    return [step(tall, dtype, "device", "fit_transform", scale=BIG, env={"SAPCA_LANCZOS_TRANSPOSE": "1"}),   # a transposed operator ...
            step(("gapped", 5000, 500, 0.25, 52), dtype, "device", "fit_transform"),                           # ... then the scatter route
            step(("gapped", 3500, 700, 0.25, 53), dtype, "host", "fit+transform"),                             # below 4096 rows: row kernel
            step(("gapped", 600, 3000, 0.25, 54), dtype, "resident", "fit_transform"),                         # wide: the small side
            step(tall, dtype, "host", "fit")]


def _setters(dtype):
    return [step(("gapped", 600, 300, 0.3, 61), dtype, "host", "fit_transform", scale=BIG),
            step(("covariate", 513, 257, 4, 8, 7), dtype, "resident", "fit_transform", cov=True),
            step(("covariate", 385, 250, 4, 0, 2), dtype, "host", "fit+transform", cov=True, scaling="weights"),
            step(("scaled", 320, 208, 4), dtype, "device", "fit_transform", scaling="unit_variance"),
            step(("gapped", 250, 150, 0.3, 62), dtype, "host", "fit_transform"),
            step(("solid", 200, 8, 0.5, 6), dtype, "resident", "fit+transform"),      # 8 columns: l = 8 < k + p
            step(("solid", 30, 40, 0.5, 1), dtype, "device", "fit_transform")]


def _chains():
    out = []
    row = config(12, 8, variant=1)
    for name, dts in (("R-row-f32", (F32,)), ("R-row-f64", (F64,)), ("R-row-mixed", (F32, F64))):
        out.append(Chain(name, row, _r_row(dts), _ROW_WALK, False))
    for name, dt in (("R-staged-f32", F32), ("R-staged-f64", F64)):
        # k = 3: the 5 x 70 matrix delivers no more; p = 40 so that l follows the small side of every shape (43, 37, 5)
        out.append(Chain(name, config(3, 40, variant=2), _r_staged(dt), _STAGED_WALK, True))
    out.append(Chain("R-auto", config(12, 8, variant=0), _r_auto(),
                     [(20, 64, "staged"), (20, 32, "row"), (20, 64, "staged"), (20, 32, "row"), (20, 64, "staged")], True))
    # l = 90 takes two column passes of the sweep.  (k = 12, p = 78, not k = 70: a matrix of 50 columns delivers at most 50
    # components, so l = 50 is only reachable with k <= 50)
    out.append(Chain("R-wide-v1", config(12, 78, variant=1), _r_wide(), [(90, 96, "row"), (50, 64, "row"), (90, 96, "row")], False))
    out.append(Chain("R-wide-v2", config(12, 78, variant=2), _r_wide(), [(90, 128, "staged"), (50, 64, "staged"), (90, 128, "staged")], False))
    out.append(Chain("M", config(8, 6, variant=2, masked=True), _masked(),
                     [(14, 64, "staged")] * 5 + [(13, 64, "staged")] + [(14, 64, "staged")] * 2, False))
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        out.append(Chain(f"L-{tag}-uncentred", config(6, 0, 0, method="lanczos", center=False), _lanczos(dt), None, True))
        out.append(Chain(f"L-{tag}-centred", config(6, 0, 0, method="lanczos", center=True, lanczos_center=True), _lanczos(dt), None, True))
    for dt, tag in ((F32, "f32"), (F64, "f64")):
        out.append(Chain(f"S-{tag}", config(SR.K, 6, variant=0, semantics="centred"), _setters(dt),
                     [(10, 16, "row")] * 5 + [(8, 16, "row"), (10, 16, "row")], False))
    return {c.name: c for c in out}


CHAINS = _chains()
M_HEAVY_STEP = 3            # the step of chain M whose kept columns set q3_cancels

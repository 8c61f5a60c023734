"""Host-side mirror of single-algebra's sparse-PCA API over the C ABI.

Same names, argument meaning and error behaviour as the reference so the parity tests read
like the reference's own (paths relative to /root/reference):

  SVDMethod, PowerIterationNormalizer      src/dimred/pca/mod.rs:41-68
  SparsePCABuilder / SparsePCA             src/dimred/pca/sparse/mod.rs:33-484
  MaskedSparsePCABuilder / MaskedSparsePCA src/dimred/pca/sparse_masked/mod.rs:37-620

Inputs are either a scipy.sparse.csr_matrix (host; indices are widened to the usize layout of
nalgebra_sparse::CsrMatrix and go through the sapca_*_csr_* entry points) or a DeviceCsr of
torch CUDA tensors (HBM-resident; sapca_*_csr_device_* entry points, outputs are torch tensors).
All compute happens in libsapca.so; this module only marshals.
"""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from ._lib import _SUF, _p, as_u64


class PowerIterationNormalizer(enum.IntEnum):
    QR = L.NORM_QR
    LU = L.NORM_LU
    NONE = L.NORM_NONE


@dataclass(frozen=True)
class SVDMethod:
    """enum SVDMethod { Lanczos, Random { n_oversamples, n_power_iterations, normalizer } }"""
    kind: str = "Lanczos"                       # Default: Lanczos (pca/mod.rs:64-68)
    n_oversamples: int = 10
    n_power_iterations: int = 4
    normalizer: PowerIterationNormalizer = PowerIterationNormalizer.QR

    @staticmethod
    def Lanczos() -> "SVDMethod":
        return SVDMethod("Lanczos")

    @staticmethod
    def Random(n_oversamples: int, n_power_iterations: int,
               normalizer: PowerIterationNormalizer = PowerIterationNormalizer.QR) -> "SVDMethod":
        return SVDMethod("Random", int(n_oversamples), int(n_power_iterations), PowerIterationNormalizer(normalizer))


class DeviceCsr:
    """HBM-resident CSR: row_offsets int64 [m+1], col_indices int32 [nnz], values f32/f64 [nnz]
    (torch CUDA tensors), columns ascending and unique per row.  Arrays of another origin go through
    ops.ResidentCsr.from_torch(...).check() / .canonicalize() first (sapca_canonicalize_csr_device_*)."""

    def __init__(self, row_offsets, col_indices, values, shape):
        import torch
        assert row_offsets.dtype == torch.int64 and col_indices.dtype == torch.int32
        assert values.dtype in (torch.float32, torch.float64)
        assert row_offsets.is_cuda and col_indices.is_cuda and values.is_cuda
        self.row_offsets = row_offsets.contiguous()
        self.col_indices = col_indices.contiguous()
        self.values = values.contiguous()
        self.shape = (int(shape[0]), int(shape[1]))
        assert self.row_offsets.numel() == self.shape[0] + 1

    @property
    def nnz(self):
        return int(self.values.numel())

    def nrows(self):
        return self.shape[0]

    def ncols(self):
        return self.shape[1]


class _Estimator:
    """State and marshalling shared by SparsePCA and MaskedSparsePCA."""

    def __init__(self, n_components, alpha, tolerance, random_seed, center, verbose, svdmethod, mask=None,
                 device=None, transform_semantics=L.TRANSFORM_REFERENCE, spmm_variant=0, collect_timings=False, lanczos_center=False):
        self.n_components = int(n_components)
        self.alpha = float(alpha)
        self.tolerance = float(tolerance)
        self.random_seed = int(random_seed)
        self.center = bool(center)
        self.verbose = bool(verbose)
        self.svdmethod = svdmethod
        self._mask = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=bool))
        self._h = C.c_void_p()
        lib = L.load()
        o = L.default_options()
        o.n_components = self.n_components
        o.alpha, o.tolerance = self.alpha, self.tolerance
        o.random_seed = self.random_seed & 0xFFFFFFFF
        o.center, o.verbose = int(self.center), int(self.verbose)
        o.collect_timings = int(bool(collect_timings))
        self.lanczos_center = bool(lanczos_center)
        o.lanczos_center = int(self.lanczos_center)
        o.method = L.RANDOM if svdmethod.kind == "Random" else L.LANCZOS
        o.n_oversamples = svdmethod.n_oversamples
        o.n_power_iterations = svdmethod.n_power_iterations
        o.normalizer = int(svdmethod.normalizer)
        o.transform_semantics = int(transform_semantics)
        o.spmm_variant = int(spmm_variant)
        o.device_id = -1 if device is None else int(device)
        try:
            import torch
            if torch.cuda.is_available():
                if device is not None:
                    torch.cuda.set_device(int(device))
                o.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        except ImportError:
            pass
        self._opts = o
        self._borrowed = False     # (a member of a sapca_multi: the multi handle owns it)
        st = lib.sapca_create(C.byref(o), C.byref(self._h))
        if st != L.OK:
            raise L.SapcaError(st, (lib.sapca_last_error(None) or b"").decode())
        if self._mask is not None and self._mask.size:
            m8 = self._mask.astype(np.uint8)
            L.check(self._h, lib.sapca_set_mask(self._h, _p(m8, C.c_uint8), C.c_size_t(m8.size)))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and not getattr(self, "_borrowed", False):
                L.load().sapca_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    # -- test hook -----------------------------------------------------------------------
    def session(self):
        """An ops.Session on THIS estimator's handle (not owned): `est.session().knn(scores)`, `est.session().tsne(scores)` run
        the steps behind the fit in the estimator's own stream and buffers, and leave the fitted model as it is."""
        from .ops import Session
        s = Session.borrow(self._h, self.random_seed & 0xFFFFFFFF)
        s._keep = self      # the handle lives as long as the estimator
        return s

    def set_omega(self, omega):
        """Inject the Gaussian test matrix of the next randomized fit (parity tests)."""
        om = np.ascontiguousarray(omega, dtype=np.float64)
        L.check(self._h, L.load().sapca_set_omega_f64(self._h, _p(om, C.c_double),
                                                      C.c_size_t(om.shape[0]), C.c_size_t(om.shape[1])))
        return self

    # -- per-row covariates, regressed out implicitly (no reference counterpart) ---------------
    def set_covariates(self, Z=None, batch=None):
        """Per-row covariates of the next fit / transform (sapca_set_covariates): SVDMethod.Random fits then factor the
        residual (I - Q Q^T) A of the regression on the design [1 | batch one-hot | Z] (the intercept with center(True))
        without forming it, and transform (TRANSFORM_CENTERED) scores A V^T - Q_rows C.  Z: (m, c) or (m,) floats; batch:
        m labels of any hashable kind, expanded to one-hot columns in order of first appearance.  At most 16 design columns,
        the intercept included; collinear designs are fine.  No arguments clears.  ValueError, before any library call, for
        a wrong row count (Z against batch), too many columns or a non-finite value."""
        from .ops import _dense_codes
        cols = []
        if batch is not None:
            labels, codes = _dense_codes(batch)
            cols.append(np.eye(len(labels), dtype=np.float64)[codes] if len(labels) else np.zeros((0, 0)))
        if Z is not None:
            z = np.asarray(Z, dtype=np.float64)
            if z.ndim == 1:
                z = z[:, None]
            if z.ndim != 2:
                raise ValueError(f"Z must be one- or two-dimensional, got shape {z.shape}")
            if cols and cols[0].shape[0] != z.shape[0]:
                raise ValueError(f"covariates have {z.shape[0]} rows, batch {cols[0].shape[0]} labels")
            cols.append(z)
        d = np.ascontiguousarray(np.hstack(cols)) if cols else np.zeros((0, 0))
        if d.size:
            design = d.shape[1] + int(self.center)
            if design > L.MAX_DESIGN_COLUMNS:
                raise ValueError(f"covariates: {design} design columns{' (the intercept included)' if self.center else ''}, "
                                 f"at most {L.MAX_DESIGN_COLUMNS} are supported")
            if not np.isfinite(d).all():
                i, j = np.argwhere(~np.isfinite(d))[0]
                raise ValueError(f"covariates: non-finite value at row {i}, column {j}")
        self._covariates = d if d.size else None
        L.check(self._h, L.load().sapca_set_covariates(self._h, _p(d, C.c_double) if d.size else None,
                                                       C.c_uint64(d.shape[0] if d.size else 0), C.c_uint64(d.shape[1] if d.size else 0)))
        return self

    @property
    def covariate_rank_(self):
        """rank of the covariate basis of the fitted model (0: fitted without covariates, or a design of rank 0)"""
        dc, r = C.c_uint64(), C.c_uint64()
        L.check(self._h, L.load().sapca_get_covariate_rank(self._h, C.byref(dc), C.byref(r)))
        return int(r.value)

    # -- column scaling, applied implicitly (no reference counterpart) -------------------------
    def set_column_scaling(self, scaling=None):
        """Column scaling of the next fit (sapca_set_column_scaling): SVDMethod.Random fits then factor (A - 1 mu^T) diag(d)
        without forming it, and transform (TRANSFORM_CENTERED) scores with the fitted d and mu.  "unit_variance": d_j =
        1 / std_j from the fit's own column statistics (0 for empty and constant columns) -- the PCA of standardised
        features; an array of one non-negative weight per column of the matrix (0 drops the column); None clears.
        ValueError, before any library call, for an unknown name, a wrong shape or a negative or non-finite weight."""
        lib = L.load()
        if scaling is None:
            self._scale_weights = None
            L.check(self._h, lib.sapca_set_column_scaling(self._h, C.c_int32(L.SCALE_NONE), None, C.c_uint64(0)))
            return self
        if isinstance(scaling, str):
            if scaling != "unit_variance":
                raise ValueError(f"column scaling: unknown mode {scaling!r} (\"unit_variance\", an array of weights or None)")
            self._scale_weights = None
            L.check(self._h, lib.sapca_set_column_scaling(self._h, C.c_int32(L.SCALE_UNIT_VARIANCE), None, C.c_uint64(0)))
            return self
        w = np.ascontiguousarray(scaling, dtype=np.float64)
        if w.ndim != 1:
            raise ValueError(f"column scaling: weights must be one-dimensional, got shape {w.shape}")
        bad = ~(np.isfinite(w) & (w >= 0))
        if bad.any():
            j = int(np.argmax(bad))
            raise ValueError(f"column scaling: weight {w[j]:g} at column {j}")
        self._scale_weights = w
        L.check(self._h, lib.sapca_set_column_scaling(self._h, C.c_int32(L.SCALE_WEIGHTS), _p(w, C.c_double) if w.size else None,
                                                      C.c_uint64(w.size)))
        return self

    @property
    def column_scale_(self):
        """the factors d the fitted model applied, one per column the fit used (aligned with components_); None for a model
        fitted without scaling"""
        mode = C.c_int32()
        L.check(self._h, L.load().sapca_get_column_scale(self._h, C.byref(mode), None, C.c_size_t(0)))
        if mode.value == L.SCALE_NONE:
            return None
        _, nu, _ = self._dims()
        out = np.empty(nu, dtype=np.float64)
        L.check(self._h, L.load().sapca_get_column_scale(self._h, C.byref(mode), _p(out, C.c_double), C.c_size_t(out.size)))
        return out

    def _scale_check(self, n):
        w = getattr(self, "_scale_weights", None)
        if w is not None and w.size != n:
            raise ValueError(f"column scaling has {w.size} weights, the matrix {n} columns")

    # -- marshalling ---------------------------------------------------------------------
    def _covariate_check(self, m):
        z = getattr(self, "_covariates", None)
        if z is not None and z.shape[0] != m:
            raise ValueError(f"covariates have {z.shape[0]} rows, the matrix {m}")

    def _mask_check(self, ncols):
        # MaskedSparsePCA raises on ANY length mismatch, including an empty mask (masked :258-262)
        if self._mask is not None and self._mask.size != ncols:
            raise L.SapcaError(L.ERR_MASK_LEN,
                               "The mask vector length and the number of features (columns) have to be the same!")

    def _call(self, op, x, want_out):
        lib = L.load()
        if isinstance(x, DeviceCsr):
            import torch
            suf = "f32" if x.values.dtype == torch.float32 else "f64"
            m, n = x.shape
            self._mask_check(n)
            self._covariate_check(m)
            if op != "transform":
                self._scale_check(n)
            args = [self._h, C.c_uint64(m), C.c_uint64(n), C.c_uint64(x.nnz),
                    C.c_void_p(x.row_offsets.data_ptr()), C.c_void_p(x.col_indices.data_ptr()),
                    C.c_void_p(x.values.data_ptr())]
            out = None
            if want_out:
                out = torch.empty((m, self.n_components), dtype=x.values.dtype, device=x.values.device)
                args.append(C.c_void_p(out.data_ptr()))
            torch.cuda.current_stream().synchronize()
            L.check(self._h, getattr(lib, f"sapca_{op}_csr_device_{suf}")(*args))
            return out
        import scipy.sparse as sp
        if not sp.isspmatrix_csr(x):
            raise TypeError("expected a scipy.sparse.csr_matrix or a sapca.DeviceCsr")
        if not x.has_sorted_indices:
            x = x.sorted_indices()
        dt = np.dtype(x.dtype)
        if dt not in _SUF:
            raise TypeError("values must be float32 or float64")
        suf, ct = _SUF[dt]
        m, n = x.shape
        self._mask_check(n)
        self._covariate_check(m)
        if op != "transform":
            self._scale_check(n)
        ro = as_u64(x.indptr)     # nalgebra_sparse usize layout
        ci = as_u64(x.indices)
        va = np.ascontiguousarray(x.data)
        args = [self._h, C.c_uint64(m), C.c_uint64(n), C.c_uint64(va.size), _p(ro, C.c_uint64),
                _p(ci, C.c_uint64), _p(va, ct)]
        out = None
        if want_out:
            out = np.empty((m, self.n_components), dtype=dt)
            args.append(_p(out, ct))
        L.check(self._h, getattr(lib, f"sapca_{op}_csr_{suf}")(*args))
        return out

    # -- reference API ---------------------------------------------------------------------
    def fit(self, x):
        self._call("fit", x, False)
        return self

    def transform(self, x):
        return self._call("transform", x, True)

    def fit_transform(self, x):
        return self._call("fit_transform", x, True)

    def _dims(self):
        k, nu, nc = C.c_uint64(), C.c_uint64(), C.c_uint64()
        L.check(self._h, L.load().sapca_get_dims(self._h, C.byref(k), C.byref(nu), C.byref(nc)))
        return k.value, nu.value, nc.value

    def _get(self, name, shape_fn, dtype=None):
        k, nu, nc = self._dims()
        dtype = np.dtype(dtype or self._fitted_dtype())
        suf, ct = _SUF[dtype]
        shape = shape_fn(k, nu, nc)
        out = np.empty(shape, dtype=dtype)
        L.check(self._h, getattr(L.load(), f"sapca_get_{name}_{suf}")(self._h, _p(out, ct), C.c_size_t(out.size)))
        return out

    def _fitted_dtype(self):
        return np.float64 if getattr(self, "_dtype64", False) else np.float32

    def feature_importances(self, dtype=None):
        return self._get("feature_importances", lambda k, nu, nc: (k, nu), dtype)

    def explained_variance_ratio(self, dtype=None):
        return self._get("explained_variance_ratio", lambda k, nu, nc: (k,), dtype)

    def cumulative_explained_variance_ratio(self, dtype=None):
        return self._get("cumulative_explained_variance_ratio", lambda k, nu, nc: (k,), dtype)

    # -- fitted fields (private in the reference; exposed for wrappers and tests) ----------------
    def components_(self, dtype=None):
        return self._get("components", lambda k, nu, nc: (k, nu), dtype)

    def explained_variance_(self, dtype=None):
        return self._get("explained_variance", lambda k, nu, nc: (k,), dtype)

    def singular_values_(self, dtype=None):
        return self._get("singular_values", lambda k, nu, nc: (k,), dtype)

    def mean_(self, dtype=None):
        return self._get("mean", lambda k, nu, nc: (nc,), dtype)

    def total_variance_(self):
        v = C.c_double()
        L.check(self._h, L.load().sapca_get_total_variance(self._h, C.byref(v)))
        return v.value

    def mask_index_maps(self):
        n = 0 if self._mask is None else self._mask.size
        cols = np.zeros(max(n, 1), dtype=np.uint64)
        o2m = np.zeros(max(n, 1), dtype=np.int64)
        L.check(self._h, L.load().sapca_get_mask_index_maps(
            self._h, _p(cols, C.c_uint64), C.c_size_t(cols.size), _p(o2m, C.c_int64), C.c_size_t(o2m.size)))
        n_used = int(self._mask.sum()) if self._mask is not None else 0
        return cols[:n_used], o2m[:n]

    def timings(self):
        t = L.Timings()
        L.check(self._h, L.load().sapca_get_timings(self._h, C.byref(t)))
        return t

    # -- multi-GPU ---------------------------------------------------------------------------
    def comm_init_rank(self, nranks, rank, unique_id: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        L.check(self._h, L.load().sapca_comm_init_rank(self._h, C.c_uint32(nranks), C.c_uint32(rank), buf))

    def comm_set_callback(self, nranks, rank, fn):
        self._cb = L.ALLREDUCE_FN(fn)     # keep alive
        L.check(self._h, L.load().sapca_comm_set_callback(self._h, C.c_uint32(nranks), C.c_uint32(rank), self._cb, None))

    def comm_abort(self):
        """End every collective of this handle (a peer rank failed): sapca_comm_abort; callable from another thread."""
        L.check(self._h, L.load().sapca_comm_abort(self._h))

    def comm_async_error(self):
        st = C.c_int32(0)
        L.check(self._h, L.load().sapca_comm_async_error(self._h, C.byref(st)))
        return int(st.value)

    def comm_has_side_lane(self):
        return bool(L.load().sapca_comm_has_side_lane(self._h))

    def measure_copy_gbs(self, nbytes=1 << 30, reps=5):
        """GB/s (read + write) of the library's 16-byte-per-lane streaming copy on this handle's device"""
        g = C.c_double(0.0)
        L.check(self._h, L.load().sapca_measure_copy_gbs(self._h, C.c_uint64(nbytes), C.c_uint32(reps), C.byref(g)))
        return float(g.value)


def _note_dtype(est, x):
    if isinstance(x, DeviceCsr):
        import torch
        est._dtype64 = x.values.dtype == torch.float64
    else:
        est._dtype64 = np.dtype(x.dtype) == np.float64


class SparsePCA(_Estimator):
    """SparsePCA<T> (sparse/mod.rs:33-359)."""

    def __init__(self, n_components, alpha, tollerance=None, random_seed=None, center=True, verbose=False,
                 svdmethod=SVDMethod(), **ext):
        super().__init__(n_components, alpha, 1e-6 if tollerance is None else tollerance,      # :75
                         42 if random_seed is None else random_seed, center, verbose, svdmethod, None, **ext)  # :76

    def fit(self, x):
        _note_dtype(self, x)
        return super().fit(x)

    def fit_transform(self, x):
        _note_dtype(self, x)
        return super().fit_transform(x)


class MaskedSparsePCA(_Estimator):
    """MaskedSparsePCA<T> (sparse_masked/mod.rs:179-620)."""

    def __init__(self, n_components, alpha, tollerance=None, random_seed=None, mask=(), center=True, verbose=False,
                 svd_method=SVDMethod(), **ext):
        super().__init__(n_components, alpha, 1e-6 if tollerance is None else tollerance,
                         42 if random_seed is None else random_seed, center, verbose, svd_method,
                         np.asarray(mask, dtype=bool), **ext)

    def fit(self, x):
        _note_dtype(self, x)
        return super().fit(x)

    def fit_transform(self, x):
        _note_dtype(self, x)
        return super().fit_transform(x)


class _BuilderBase:
    def __init__(self):
        # defaults: sparse/mod.rs:392-401, sparse_masked/mod.rs:55-66
        self._n_components = 50
        self._alpha = 1.0
        self._tolerance = 1e-6
        self._random_seed: Optional[int] = 42
        self._center = True
        self._verbose = False
        self._svdmethod = SVDMethod()
        self._ext = {}

    @classmethod
    def new(cls):
        return cls()

    @classmethod
    def default(cls):
        return cls()

    def n_components(self, n):
        self._n_components = int(n)
        return self

    def alpha(self, a):
        self._alpha = float(a)
        return self

    def tolerance(self, t):
        self._tolerance = float(t)
        return self

    def random_seed(self, seed):
        self._random_seed = int(seed)
        return self

    def center(self, c):
        self._center = bool(c)
        return self

    def verbose(self, v):
        self._verbose = bool(v)
        return self

    def svd_method(self, m: SVDMethod):
        self._svdmethod = m
        return self

    # extensions that have no reference counterpart (device placement, diagnostics)
    def device(self, ordinal):
        self._ext["device"] = int(ordinal)
        return self

    def transform_semantics(self, sem):
        self._ext["transform_semantics"] = int(sem)
        return self

    def lanczos_center(self, on=True):
        """SVDMethod.Lanczos with center(True): factor the centred operator A - 1 mu^T (a real PCA) instead of the raw
        matrix (the reference's behaviour, the default).  No effect with center(False) or SVDMethod.Random."""
        self._ext["lanczos_center"] = bool(on)
        return self

    def spmm_variant(self, v):
        self._ext["spmm_variant"] = int(v)
        return self

    def collect_timings(self, on=True):
        self._ext["collect_timings"] = bool(on)
        return self


class SparsePCABuilder(_BuilderBase):
    """SparsePCABuilder<T> (sparse/mod.rs:375-484)."""

    def build(self) -> SparsePCA:
        return SparsePCA(self._n_components, self._alpha, self._tolerance,
                         42 if self._random_seed is None else self._random_seed,       # :475
                         self._center, self._verbose, self._svdmethod, **self._ext)


class MaskedSparsePCABuilder(_BuilderBase):
    """MaskedSparsePCABuilder<T> (sparse_masked/mod.rs:37-160)."""

    def __init__(self):
        super().__init__()
        self._mask = np.zeros(0, dtype=bool)                                            # :62

    def mask(self, mask):
        self._mask = np.asarray(mask, dtype=bool)
        return self

    def build(self) -> MaskedSparsePCA:
        return MaskedSparsePCA(self._n_components, self._alpha, self._tolerance,
                               42 if self._random_seed is None else self._random_seed, self._mask,
                               self._center, self._verbose, self._svdmethod, **self._ext)


class TSNE:
    """t-SNE of dense rows on the GPU (sapca_tsne_*): the reference's dimred::tsne -- TSNEConfig { output_dim, perplexity,
    epochs, theta } with run_f32 / run_f64 (src/dimred/tsne/mod.rs:7-66) -- as an estimator.  The repulsive term is evaluated
    exactly: theta is kept for drop-in and not read (include/sapca.h, deviation 1).

        emb = sapca.TSNE(perplexity=30, epochs=500).fit_transform(scores)      # a torch device tensor, or a numpy array

    `scores` is usually what SparsePCA.fit_transform left on the device; it is searched in place.  After the call
    `embedding_` holds the result and `kl_divergence_` its Kullback-Leibler divergence.  constants: stop_lying_epoch,
    momentum_switch_epoch, exaggeration, learning_rate, momentum, final_momentum."""

    def __init__(self, output_dim=2, perplexity=20.0, epochs=1000, theta=0.5, random_seed=42, **constants):
        self.output_dim, self.perplexity, self.epochs, self.theta = int(output_dim), float(perplexity), int(epochs), float(theta)
        self.random_seed = int(random_seed)
        self.constants = dict(constants)
        self.embedding_ = None
        self.kl_divergence_ = None
        self._session = None

    def fit_transform(self, X, init=None):
        from .ops import Session
        if self._session is None:
            self._session = Session(seed=self.random_seed)
        self.embedding_, self.kl_divergence_ = self._session.tsne(
            X, perplexity=self.perplexity, epochs=self.epochs, output_dim=self.output_dim, init=init, seed=self.random_seed,
            theta=self.theta, **self.constants)
        return self.embedding_

    def fit(self, X, init=None):
        self.fit_transform(X, init)
        return self


class UMAP:
    """UMAP of dense rows on the GPU (sapca_umap_*): umap-learn's fuzzy simplicial set and a synchronous, deterministic
    restatement of its layout (include/sapca.h states the algorithm and the deviations), as an estimator.

        emb = sapca.UMAP(n_neighbors=15, min_dist=0.1).fit_transform(scores)   # a torch device tensor, or a numpy array

    `scores` is usually what SparsePCA.fit_transform left on the device; it is searched in place.  init: "panel" (the first
    output_dim columns of X, scaled to 0 .. 10), "random", or an m x output_dim array to start from.  n_epochs None:
    umap-learn's rule (500 for at most 10000 rows, else 200).  a, b None: fitted from (spread, min_dist).  After the call
    `embedding_` holds the result."""

    def __init__(self, n_neighbors=15, min_dist=0.1, spread=1.0, n_epochs=None, output_dim=2, init="panel", negative_sample_rate=5,
                 learning_rate=1.0, repulsion_strength=1.0, a=None, b=None, random_seed=42):
        self.n_neighbors, self.min_dist, self.spread, self.n_epochs = int(n_neighbors), float(min_dist), float(spread), n_epochs
        self.output_dim, self.init, self.negative_sample_rate = int(output_dim), init, int(negative_sample_rate)
        self.learning_rate, self.repulsion_strength = float(learning_rate), float(repulsion_strength)
        self.a, self.b, self.random_seed = a, b, int(random_seed)
        self.embedding_ = None
        self._session = None

    def fit_transform(self, X):
        from .ops import Session
        if self._session is None:
            self._session = Session(seed=self.random_seed)
        self.embedding_ = self._session.umap(
            X, n_neighbors=self.n_neighbors, min_dist=self.min_dist, spread=self.spread, n_epochs=self.n_epochs,
            output_dim=self.output_dim, init=self.init, negative_sample_rate=self.negative_sample_rate,
            learning_rate=self.learning_rate, repulsion_strength=self.repulsion_strength, a=self.a, b=self.b, seed=self.random_seed)
        return self.embedding_

    def fit(self, X):
        self.fit_transform(X)
        return self


class KMeans:
    """K-means clustering of dense rows on the GPU (sapca_kmeans_*): Lloyd's iteration under scikit-learn's stopping rule with
    k-means++ seeding, deterministic under `seed`; a cluster that loses all its rows keeps its centroid.

        km = sapca.KMeans(n_clusters=12).fit(scores)       # a torch device tensor (clustered in place), or a numpy array
        km.labels_, km.cluster_centers_, km.inertia_, km.n_iter_
        km.predict(other_scores)

    `scores` is usually what SparsePCA.fit_transform left on the device.  init: "k-means++" or an n_clusters x d array of
    centroids.  One run per fit: callers who want scikit-learn's n_init loop over seeds and keep the least inertia_."""

    def __init__(self, n_clusters=8, init="k-means++", max_iter=300, tol=1e-4, seed=42):
        self.n_clusters, self.init, self.max_iter, self.tol, self.seed = int(n_clusters), init, int(max_iter), float(tol), int(seed)
        self.labels_ = self.cluster_centers_ = self.inertia_ = self.n_iter_ = None
        self._session = None

    def _ops(self):
        from .ops import Session
        if self._session is None:
            self._session = Session(seed=self.seed)
        return self._session

    def fit(self, X):
        self.labels_, self.cluster_centers_, self.inertia_, self.n_iter_ = self._ops().kmeans(
            X, n_clusters=self.n_clusters, init=self.init, max_iter=self.max_iter, tol=self.tol, seed=self.seed)
        return self

    def fit_predict(self, X):
        return self.fit(X).labels_

    def predict(self, X):
        """the nearest of cluster_centers_ for every row of X: a device tensor (labels on the device), or a numpy array (labels
        as a numpy array)"""
        if self.cluster_centers_ is None:
            raise RuntimeError("KMeans.predict: fit first")
        import torch
        ops = self._ops()
        host = isinstance(X, np.ndarray)
        Xd = torch.as_tensor(np.ascontiguousarray(X), device=ops._device()) if host else X
        cen = torch.as_tensor(self.cluster_centers_, device=Xd.device).to(Xd.dtype)
        labels = ops.kmeans_assign(Xd, cen)[0]
        return labels.cpu().numpy() if host else labels


class Harmony:
    """Harmony batch integration of dense score rows on the GPU (sapca_harmony_*): what scanpy.external.pp.harmony_integrate does
    between the PCA and `neighbors`, restated deterministically (include/sapca.h lists the deviations from harmonypy).

        hm = sapca.Harmony(theta=2.0).fit(scores, batch)   # a torch device tensor (read in place), or a numpy array
        hm.Z_corr_, hm.R_, hm.cluster_centers_, hm.objectives_, hm.passes_, hm.n_iter_, hm.converged_
        corrected = sapca.Harmony().fit_transform(scores, batch)

    `batch` holds one integer label per row; an int32 device tensor -- what KMeans or the user left on the device -- is taken as
    it is.  n_clusters defaults to min(round(m / 30), 100)."""

    def __init__(self, n_clusters=None, theta=2.0, sigma=0.1, lam=1.0, n_blocks=20, max_iter_harmony=10, max_iter_cluster=20,
                 epsilon_cluster=1e-5, epsilon_harmony=1e-4, init="kmeans", seed=42):
        self.n_clusters, self.theta, self.sigma, self.lam, self.n_blocks = n_clusters, float(theta), float(sigma), float(lam), int(n_blocks)
        self.max_iter_harmony, self.max_iter_cluster = int(max_iter_harmony), int(max_iter_cluster)
        self.epsilon_cluster, self.epsilon_harmony, self.init, self.seed = float(epsilon_cluster), float(epsilon_harmony), init, int(seed)
        self.Z_corr_ = self.R_ = self.cluster_centers_ = self.objectives_ = self.passes_ = self.n_iter_ = self.converged_ = None
        self._session = None

    def _ops(self):
        from .ops import Session
        if self._session is None:
            self._session = Session(seed=self.seed)
        return self._session

    def fit(self, X, batch, n_batches=None):
        self.Z_corr_, res = self._ops().harmony(
            X, batch, n_clusters=self.n_clusters, n_batches=n_batches, init=self.init, theta=self.theta, sigma=self.sigma, lam=self.lam,
            n_blocks=self.n_blocks, max_iter_harmony=self.max_iter_harmony, max_iter_cluster=self.max_iter_cluster,
            epsilon_cluster=self.epsilon_cluster, epsilon_harmony=self.epsilon_harmony, seed=self.seed)
        self.R_, self.cluster_centers_, self.objectives_, self.passes_ = res.R, res.centroids, res.objectives, res.passes
        self.n_iter_, self.converged_ = res.n_iter, res.converged
        return self

    def fit_transform(self, X, batch, n_batches=None):
        return self.fit(X, batch, n_batches).Z_corr_


class Louvain:
    """Louvain communities of the neighbour graph on the GPU (sapca_louvain_*): what scanpy runs after `neighbors`, restated as
    deterministic synchronous sweeps (include/sapca.h).

        lv = sapca.Louvain(resolution=1.0)
        labels = lv.fit_predict(scores)          # an m x d device tensor: knn -> fuzzy union -> communities; or a ResidentCsr graph
        lv.labels_, lv.modularity_, lv.n_communities_, lv.n_levels_

    The number of clusters is found, not given; `resolution` above 1 gives more and smaller communities."""

    def __init__(self, resolution=1.0, tol=1e-7, max_sweeps=256, max_levels=None, n_neighbors=15, seed=42):
        self.resolution, self.tol, self.max_sweeps, self.max_levels = float(resolution), float(tol), int(max_sweeps), max_levels
        self.n_neighbors, self.seed = int(n_neighbors), int(seed)
        self.labels_ = self.modularity_ = self.n_communities_ = self.n_levels_ = None
        self._session = None

    def _ops(self):
        from .ops import Session
        if self._session is None:
            self._session = Session(seed=self.seed)
        return self._session

    def fit(self, G_or_X):
        from .ops import ResidentCsr
        ops = G_or_X._s if isinstance(G_or_X, ResidentCsr) else self._ops()   # (a resident graph is clustered by the Session that owns it)
        self.labels_, self.n_communities_, self.modularity_, self.n_levels_ = ops.louvain(
            G_or_X, resolution=self.resolution, tol=self.tol, max_sweeps=self.max_sweeps, max_levels=self.max_levels, seed=self.seed,
            n_neighbors=self.n_neighbors)
        return self

    def fit_predict(self, G_or_X):
        return self.fit(G_or_X).labels_

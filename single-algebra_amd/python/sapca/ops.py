"""Stage-level operators of the C ABI (host buffers in and out) for the parity tests:
sum_col / sum_col_squared (src/sparse/csr.rs:259-312, 558-608), the two sweeps and the
normaliser inside randomized_svd, the Omega generator, the row partitioner."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import _SUF, _p, as_u64

def _knn_panel(name, t):
    """(rows, d, row stride, torch dtype) of a panel for Session.knn: a two-dimensional tensor of float32 / float64 whose
    rows are contiguous (stride(1) == 1, or a single column) and at least d elements apart -- a slice of a wider buffer
    is fine.  Pure host checks: ValueError otherwise."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor on the device, got {type(t).__name__}")
    if t.dim() != 2:
        raise ValueError(f"{name} must be two-dimensional (rows x d), got shape {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be float32 or float64, got {t.dtype}")
    rows, d = int(t.shape[0]), int(t.shape[1])
    if d > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: the elements of a row must be contiguous (stride(1) == 1), got strides {tuple(t.stride())}")
    ld = int(t.stride(0)) if rows > 1 else d
    if ld < d:
        raise ValueError(f"{name}: rows overlap (row stride {ld} < d = {d})")
    return rows, d, ld, t.dtype


class HarmonyResult:
    """What Session.harmony returns beside the corrected panel: R (m x K soft assignment) and centroids (K x d, unit rows) where
    the rows live, and on the host the last objective and the number of clustering passes of every outer iteration, n_iter and
    converged."""

    def __init__(self, R, centroids, objectives, passes, n_iter, converged):
        self.R, self.centroids, self.objectives, self.passes, self.n_iter, self.converged = R, centroids, objectives, passes, n_iter, converged

    def __repr__(self):
        return f"HarmonyResult(n_iter={self.n_iter}, converged={self.converged}, passes={list(self.passes)})"


class Session:
    """A bare handle (default options) to run stage-level operators on."""

    def __init__(self, seed=42, spmm_variant=0, stream=None):
        self._h = C.c_void_p()
        o = L.default_options()
        o.random_seed = seed
        self._seed, self._owned = seed, True
        o.spmm_variant = spmm_variant
        if stream is not None:   # a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream): the handle's work goes there
            o.stream = C.c_void_p(int(stream))
        st = L.load().sapca_create(C.byref(o), C.byref(self._h))
        if st != L.OK:
            raise L.SapcaError(st, (L.load().sapca_last_error(None) or b"").decode())

    @classmethod
    def borrow(cls, handle, seed=42):
        """A Session on a handle that something else owns (an estimator's: `SparsePCA.session()`): the stage-level operators
        run on that handle, in its stream and buffers; it is not destroyed with this object."""
        self = cls.__new__(cls)
        self._h, self._seed, self._owned = handle, int(seed), False
        return self

    def _device(self):
        """the torch device of the handle's GPU (a handle is created on the current device)"""
        import torch
        return torch.device("cuda", torch.cuda.current_device())

    def __del__(self):
        try:
            if self._h and getattr(self, "_owned", False):
                L.load().sapca_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def _csr_args(self, indptr, indices, data, m, n):
        ro = as_u64(indptr)
        ci = as_u64(indices)
        va = np.ascontiguousarray(data)
        suf, ct = _SUF[va.dtype]
        keep = (ro, ci, va)
        return suf, ct, keep, [self._h, C.c_uint64(m), C.c_uint64(n), C.c_uint64(va.size), _p(ro, C.c_uint64),
                               _p(ci, C.c_uint64), _p(va, ct)]

    def colstats(self, indptr, indices, data, m, n):
        suf, ct, keep, args = self._csr_args(indptr, indices, data, m, n)
        s = np.zeros(n, dtype=data.dtype)
        sq = np.zeros(n, dtype=data.dtype)
        cnt = np.zeros(n, dtype=np.uint64)
        L.check(self._h, getattr(L.load(), f"sapca_colstats_csr_{suf}")(*args, _p(s, ct), _p(sq, ct), _p(cnt, C.c_uint64)))
        return s, sq, cnt

    def spmm(self, indptr, indices, data, m, n, X, mu=None, transposed=False):
        suf, ct, keep, args = self._csr_args(indptr, indices, data, m, n)
        X = np.ascontiguousarray(X, dtype=data.dtype)
        l = X.shape[1]
        out = np.zeros((n if transposed else m, l), dtype=data.dtype)
        mu_p = _p(np.ascontiguousarray(mu, dtype=data.dtype), ct) if mu is not None else None
        fn = getattr(L.load(), f"sapca_spmm{'t' if transposed else ''}_csr_{suf}")
        L.check(self._h, fn(*args, mu_p, C.c_uint64(l), _p(X, ct), _p(out, ct)))
        return out

    def normalize_panel(self, P, normalizer):
        P = np.array(P, order="C", copy=True)
        suf, ct = _SUF[P.dtype]
        L.check(self._h, getattr(L.load(), f"sapca_normalize_panel_{suf}")(
            self._h, C.c_int32(int(normalizer)), C.c_uint64(P.shape[0]), C.c_uint64(P.shape[1]), _p(P, ct)))
        return P

    def project_out_panel(self, P, Q):
        """sapca_project_out_panel_*: P - Q (Q^T P) for a rows x l panel and a rows x r basis (r <= 16), by the two kernels of
        the covariate route (csrc/covar.hip)"""
        P = np.array(P, order="C", copy=True)
        Q = np.ascontiguousarray(Q, dtype=P.dtype)
        if Q.ndim != 2 or P.ndim != 2 or Q.shape[0] != P.shape[0]:
            raise ValueError(f"panel {P.shape} and basis {Q.shape} must be two-dimensional with the same number of rows")
        suf, ct = _SUF[P.dtype]
        L.check(self._h, getattr(L.load(), f"sapca_project_out_panel_{suf}")(
            self._h, C.c_uint64(P.shape[0]), C.c_uint64(P.shape[1]), _p(P, ct), C.c_uint32(Q.shape[1]), _p(Q, ct)))
        return P

    def scale_panel_rows(self, P, scale):
        """sapca_scale_panel_rows_*: P[r, :] * dtype(scale[r]) for a rows x l panel, by the row-scaling kernel of the
        column-scaling route (csrc/colscale.hip)"""
        P = np.array(P, order="C", copy=True)
        d = np.ascontiguousarray(scale, dtype=np.float64)
        if P.ndim != 2 or d.ndim != 1 or d.shape[0] != P.shape[0]:
            raise ValueError(f"panel {P.shape} must be two-dimensional and scale {d.shape} hold one factor per row")
        suf, ct = _SUF[P.dtype]
        L.check(self._h, getattr(L.load(), f"sapca_scale_panel_rows_{suf}")(
            self._h, C.c_uint64(P.shape[0]), C.c_uint64(P.shape[1]), _p(P, ct), _p(d, C.c_double)))
        return P

    def normalize_panel_ex(self, slabs, normalizer, passes=0, mu=None, sv=None, w=None, want_vec=True, want_r=True):
        """sapca_normalize_panel_ex_*: Engine::normalize with its extras on a panel still lying in the nsplit x rows x l slabs
        of a sweep (a rows x l array is one slab), minus mu sv^T.  Returns a dict: panel (rows x l), vec (l: sum_r w[r]
        panel[r, :], w None = ones; None without want_vec), r1 / r2 (l x l f64 upper factors of the CholeskyQR passes, zeros
        for a pass that did not run; None without want_r), regularised (pivots floored)."""
        S = np.array(slabs, order="C", copy=True)
        if S.ndim == 2:
            S = S[None]
        if S.ndim != 3:
            raise ValueError(f"slabs {S.shape} must be nsplit x rows x l (or rows x l)")
        nsplit, rows, l = S.shape
        suf, ct = _SUF[S.dtype]
        if (mu is None) != (sv is None):
            raise ValueError("mu and sv go together")
        vecs = {}
        for name, v, n in (("mu", mu, rows), ("sv", sv, l), ("w", w, rows)):
            if v is not None:
                v = np.ascontiguousarray(v, dtype=S.dtype)
                if v.shape != (n,):
                    raise ValueError(f"{name} {v.shape} must hold {n} values")
            vecs[name] = v
        ptr = lambda a, t=ct: None if a is None else _p(a, t)   # noqa: E731
        panel = np.zeros((rows, l), dtype=S.dtype)
        vec = np.zeros(l, dtype=S.dtype) if want_vec else None
        r1 = np.zeros((l, l)) if want_r else None
        r2 = np.zeros((l, l)) if want_r else None
        reg = C.c_int32(-1)
        L.check(self._h, getattr(L.load(), f"sapca_normalize_panel_ex_{suf}")(
            self._h, C.c_int32(int(normalizer)), C.c_int32(int(passes)), C.c_uint64(rows), C.c_uint64(l), C.c_uint32(nsplit),
            _p(S, ct), ptr(vecs["mu"]), ptr(vecs["sv"]), ptr(vecs["w"]), _p(panel, ct), ptr(vec), ptr(r1, C.c_double),
            ptr(r2, C.c_double), C.byref(reg)))
        return {"panel": panel, "vec": vec, "r1": r1, "r2": r2, "regularised": int(reg.value)}

    def rotate_panel(self, P, M):
        """sapca_rotate_panel_*: (components, signs) = svd_flip((P M)^T) for an n x l panel P and an l x k factor M (taken as
        f64) -- components k x n in P's dtype, signs k doubles -- by the panel product and the sign kernels a fit ends in."""
        P = np.ascontiguousarray(P)
        M = np.ascontiguousarray(M, dtype=np.float64)
        if P.ndim != 2 or M.ndim != 2 or M.shape[0] != P.shape[1]:
            raise ValueError(f"panel {P.shape} and factor {M.shape} must be n x l and l x k")
        suf, ct = _SUF[P.dtype]
        n, l = P.shape
        k = M.shape[1]
        comps = np.zeros((k, n), dtype=P.dtype)
        signs = np.zeros(k)
        L.check(self._h, getattr(L.load(), f"sapca_rotate_panel_{suf}")(
            self._h, C.c_uint64(n), C.c_uint64(l), C.c_uint64(k), _p(P, ct), _p(M, C.c_double), _p(comps, ct), _p(signs, C.c_double)))
        return comps, signs

    def generate_omega(self, rows, l, dtype=np.float64):
        out = np.zeros((rows, l), dtype=dtype)
        suf, ct = _SUF[np.dtype(dtype)]
        L.check(self._h, getattr(L.load(), f"sapca_generate_omega_{suf}")(self._h, C.c_uint64(rows), C.c_uint64(l), _p(out, ct)))
        return out

    def knn(self, queries, corpus=None, n_neighbors=15, metric="euclidean", exclude_self=None):
        """sapca_knn_device_*: (indices, values), two device tensors of shape (rows of queries, n_neighbors) -- for every query row
        the n_neighbors nearest rows of `corpus`, best first: int32 corpus row numbers, and the Euclidean distance or the
        cosine / Pearson similarity of the reference's src/similarity/mod.rs.  Ordered by value (ascending distance,
        descending similarity), then by ascending index; the same bytes from call to call.  corpus None: the queries
        themselves, with a row's own index left out unless exclude_self=False.  Both panels are CUDA tensors of one dtype with
        contiguous rows (a column slice of a wider score buffer is taken in place).  A row of norm <= sqrt(eps) -- after centring,
        for Pearson -- is the zero vector: similarity 0 to everything.
        Stream order: the Session works on its own stream (or the one it was given); torch's current stream is synchronised
        first, and the outputs are complete on return.  Bad arguments raise ValueError here, before any device work."""
        import torch
        if isinstance(metric, str):
            if metric.lower() not in L.KNN_METRICS:
                raise ValueError(f"unknown metric {metric!r}: one of {sorted(L.KNN_METRICS)}")
            code = L.KNN_METRICS[metric.lower()]
        else:
            code = int(metric)
            if code not in L.KNN_METRICS.values():
                raise ValueError(f"unknown metric {metric!r}: one of {sorted(L.KNN_METRICS)}")
        mq, d, ldq, dt = _knn_panel("queries", queries)
        if corpus is None:
            corpus = queries
            if exclude_self is None:
                exclude_self = True
        mc, dc, ldc, dtc = _knn_panel("corpus", corpus)
        if dc != d:
            raise ValueError(f"queries have {d} columns, the corpus {dc}")
        if dtc != dt or corpus.device != queries.device:
            raise ValueError(f"queries ({dt}, {queries.device}) and corpus ({dtc}, {corpus.device}) must share dtype and device")
        exclude_self = bool(exclude_self)
        k = int(n_neighbors)
        if k < 1:
            raise ValueError(f"n_neighbors must be at least 1, got {n_neighbors}")
        if k > L.KNN_MAX_NEIGHBORS:
            raise ValueError(f"n_neighbors = {k} exceeds the {L.KNN_MAX_NEIGHBORS} the library keeps per query")
        if k > mc - int(exclude_self):
            raise ValueError(f"n_neighbors = {k} exceeds the {max(mc - int(exclude_self), 0)} corpus rows a query can have "
                             f"(corpus rows {mc}{', itself excluded' if exclude_self else ''})")
        if d < 1 or d > 1024:
            raise ValueError(f"the panels have {d} columns; 1 .. 1024 are supported")
        for name, t in (("queries", queries), ("corpus", corpus)):   # (last: everything above is checked without a device)
            if not t.is_cuda:
                raise ValueError(f"{name} must live on the device (a CUDA tensor), got a tensor on {t.device}")
        idx = torch.empty((mq, k), dtype=torch.int32, device=queries.device)
        val = torch.empty((mq, k), dtype=dt, device=queries.device)
        suf = "f32" if dt == torch.float32 else "f64"
        torch.cuda.current_stream().synchronize()   # what torch has queued for the panels is complete before the handle's stream reads them
        L.check(self._h, getattr(L.load(), f"sapca_knn_device_{suf}")(
            self._h, C.c_uint64(mq), C.c_void_p(queries.data_ptr() if mq else None), C.c_uint64(ldq), C.c_uint64(mc),
            C.c_void_p(corpus.data_ptr()), C.c_uint64(ldc), C.c_uint64(d), C.c_int32(code), C.c_uint32(k),
            C.c_uint32(L.KNN_EXCLUDE_SELF if exclude_self else 0), C.c_void_p(idx.data_ptr() if mq else None),
            C.c_void_p(val.data_ptr() if mq else None)))
        return idx, val

    # ---- t-SNE (sapca_tsne_*): the affinity graph, one gradient evaluation, the embedding ----
    def _tsne_options(self, perplexity, epochs, output_dim, init_given, seed, constants):
        o = L.default_tsne_options()
        o.random_seed = int(self._seed if seed is None else seed)
        o.perplexity, o.epochs, o.output_dim, o.init_given = float(perplexity), int(epochs), int(output_dim), int(bool(init_given))
        for name, value in constants.items():
            if name not in ("theta", "stop_lying_epoch", "momentum_switch_epoch", "exaggeration", "learning_rate", "momentum",
                            "final_momentum"):
                raise ValueError(f"unknown t-SNE constant {name!r}")
            setattr(o, name, type(getattr(o, name))(value))
        return o

    def tsne_affinities(self, indices, dist, perplexity):
        """sapca_tsne_affinities_device_*: (P, beta) from neighbour lists as knn() returns them (m x K device tensors, int32
        indices and f32 / f64 distances).  P is the symmetric affinity matrix (p_j|i + p_i|j) / (2 m) as a canonical
        ResidentCsr in the Session's t-SNE buffers (valid until the next affinity call on the Session), beta the m precisions
        of the perplexity search (f64 device tensor)."""
        import torch
        m, K, ld, dt = _knn_panel("dist", dist)
        if not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int32 and tuple(indices.shape) == (m, K)
                and indices.is_contiguous() and dist.is_contiguous()):
            raise ValueError("indices must be a contiguous int32 tensor of the shape of dist, dist contiguous")
        if not (indices.is_cuda and dist.is_cuda):
            raise ValueError("indices and dist must live on the device")
        beta = torch.empty((m,), dtype=torch.float64, device=dist.device)
        suf = "f32" if dt == torch.float32 else "f64"
        nnz = C.c_uint64()
        dp, di, dv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_tsne_affinities_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(indices.data_ptr() if m else None), C.c_void_p(dist.data_ptr() if m else None),
            C.c_uint32(K), C.c_double(float(perplexity)), C.byref(nnz), C.byref(dp), C.byref(di), C.byref(dv),
            C.c_void_p(beta.data_ptr() if m else None)))
        P = ResidentCsr(self, (m, m), nnz.value, np.float32 if suf == "f32" else np.float64, dp.value or 0, di.value or 0, dv.value or 0)
        return P, beta

    def tsne_gradient(self, P, Y, exaggeration=1.0):
        """sapca_tsne_gradient_device_*: (grad, Z, kl) at the embedding Y (m x output_dim device tensor of P's dtype) for the
        affinity matrix P (a ResidentCsr): grad a device tensor of Y's shape, Z and kl Python floats."""
        import torch
        m, D, ld, dt = _knn_panel("Y", Y)
        if not Y.is_cuda:
            raise ValueError("Y must live on the device")
        if np.dtype(np.float32 if dt == torch.float32 else np.float64) != P.dtype or P.shape != (m, m):
            raise ValueError(f"P {P.shape} {P.dtype} and Y {tuple(Y.shape)} {dt} do not belong together")
        grad = torch.empty((m, D), dtype=dt, device=Y.device)
        Z, kl = C.c_double(), C.c_double()
        suf = "f32" if dt == torch.float32 else "f64"
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_tsne_gradient_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint64(P.nnz), C.c_void_p(P.d_ptr), C.c_void_p(P.d_idx), C.c_void_p(P.d_val),
            C.c_void_p(Y.data_ptr() if m else None), C.c_uint64(ld), C.c_uint32(D), C.c_double(float(exaggeration)),
            C.c_void_p(grad.data_ptr() if m else None), C.byref(Z), C.byref(kl)))
        return grad, Z.value, kl.value

    def tsne_embed(self, P, epochs=1000, output_dim=2, init=None, seed=None, **constants):
        """sapca_tsne_embed_device_*: (Y, kl) for the affinity matrix P (a ResidentCsr): the optimiser alone.  init: an
        m x output_dim device tensor to start from (copied), or None for 1e-4 N(0, 1) under the seed."""
        import torch
        m = P.shape[0]
        o = self._tsne_options(20.0, epochs, output_dim, init is not None, seed, constants)
        dt = torch.float32 if P.dtype == np.float32 else torch.float64
        if init is not None:
            if not (isinstance(init, torch.Tensor) and init.is_cuda and init.dtype == dt and tuple(init.shape) == (m, int(output_dim))):
                raise ValueError(f"init must be a device tensor of shape {(m, int(output_dim))} and dtype {dt}")
            Y = init.contiguous().clone()
        else:
            Y = torch.empty((m, int(output_dim)), dtype=dt, device=self._device())
        kl = C.c_double()
        suf = "f32" if dt == torch.float32 else "f64"
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_tsne_embed_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint64(P.nnz), C.c_void_p(P.d_ptr), C.c_void_p(P.d_idx), C.c_void_p(P.d_val), C.byref(o),
            C.c_void_p(Y.data_ptr() if m else None), C.byref(kl)))
        return Y, kl.value

    def tsne(self, X, perplexity=20.0, epochs=1000, output_dim=2, init=None, seed=None, **constants):
        """sapca_tsne_device_* / sapca_tsne_*: (Y, kl), the t-SNE embedding of the rows of X and its Kullback-Leibler
        divergence.  X: an m x d torch device tensor of float32 / float64 with contiguous rows (a column slice of the scores
        is searched in place; Y is a device tensor), or a numpy array (the host route, the drop-in for the reference's
        run_f32 / run_f64; Y is a numpy array).  init: the initial embedding in the same kind of array, else 1e-4 N(0, 1)
        under `seed` (the Session's by default).  constants: theta (stored, not read), stop_lying_epoch,
        momentum_switch_epoch, exaggeration, learning_rate, momentum, final_momentum.  The same bytes from call to call."""
        o = self._tsne_options(perplexity, epochs, output_dim, init is not None, seed, constants)
        D = int(output_dim)
        kl = C.c_double()
        if isinstance(X, np.ndarray):
            if X.ndim != 2 or X.dtype not in _SUF:
                raise ValueError(f"X must be a two-dimensional float32 / float64 array, got {X.dtype} {X.shape}")
            X = np.ascontiguousarray(X)
            m, d = X.shape
            Y = np.zeros((m, D), dtype=X.dtype)
            if init is not None:
                init = np.asarray(init)
                if init.shape != (m, D):
                    raise ValueError(f"init must have shape {(m, D)}, got {init.shape}")
                Y[...] = init
            suf, ct = _SUF[X.dtype]
            L.check(self._h, getattr(L.load(), f"sapca_tsne_{suf}")(
                self._h, C.c_uint64(m), C.c_uint64(d), X.ctypes.data_as(C.c_void_p), C.byref(o), Y.ctypes.data_as(C.c_void_p),
                C.byref(kl)))
            return Y, kl.value
        import torch
        m, d, ld, dt = _knn_panel("X", X)
        if not X.is_cuda:
            raise ValueError(f"X must live on the device (a CUDA tensor) or be a numpy array, got a tensor on {X.device}")
        if init is not None:
            if not (isinstance(init, torch.Tensor) and init.is_cuda and init.dtype == dt and tuple(init.shape) == (m, D)):
                raise ValueError(f"init must be a device tensor of shape {(m, D)} and dtype {dt}")
            Y = init.contiguous().clone()
        else:
            Y = torch.empty((m, D), dtype=dt, device=X.device)
        suf = "f32" if dt == torch.float32 else "f64"
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_tsne_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(X.data_ptr() if m else None), C.c_uint64(ld), C.c_uint64(d), C.byref(o),
            C.c_void_p(Y.data_ptr() if m else None), C.byref(kl)))
        return Y, kl.value

    # ---- UMAP (sapca_umap_*): the fuzzy union of neighbour lists, the layout, the whole chain ----
    def _umap_options(self, n_neighbors, min_dist, spread, n_epochs, output_dim, init, negative_sample_rate, learning_rate,
                      repulsion_strength, a, b, seed):
        """(options, the initial embedding or None): init is "panel", "random" or an array / tensor to start from"""
        o = L.default_umap_options()
        o.random_seed = int(self._seed if seed is None else seed)
        o.n_neighbors, o.output_dim, o.negative_sample_rate = int(n_neighbors), int(output_dim), int(negative_sample_rate)
        o.min_dist, o.spread, o.epochs = float(min_dist), float(spread), int(n_epochs or 0)
        o.learning_rate, o.repulsion_strength = float(learning_rate), float(repulsion_strength)
        if (a is None) != (b is None):
            raise ValueError(f"a = {a!r}, b = {b!r}: give both, or neither to have them fitted from (spread, min_dist)")
        o.a, o.b = (0.0, 0.0) if a is None else (float(a), float(b))
        given = None
        if isinstance(init, str):
            if init.lower() not in L.UMAP_INITS:
                raise ValueError(f"unknown init {init!r}: one of {sorted(L.UMAP_INITS)} or an initial embedding")
            o.init = L.UMAP_INITS[init.lower()]
        else:
            o.init, given = L.UMAP_INIT_GIVEN, init
        return o, given

    def umap_graph(self, indices, dist, n_neighbors):
        """sapca_umap_graph_device_*: (G, sigma, rho) from neighbour lists as knn() returns them (m x K device tensors, int32
        indices and f32 / f64 distances; n_neighbors counts the point itself, usually K + 1).  G is the fuzzy union as a
        canonical ResidentCsr in the Session's UMAP buffers (valid until the next graph call on the Session), sigma and rho
        the m smooth-distance scales and offsets (f64 device tensors)."""
        import torch
        m, K, ld, dt = _knn_panel("dist", dist)
        if not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int32 and tuple(indices.shape) == (m, K)
                and indices.is_contiguous() and dist.is_contiguous()):
            raise ValueError("indices must be a contiguous int32 tensor of the shape of dist, dist contiguous")
        if not (indices.is_cuda and dist.is_cuda):
            raise ValueError("indices and dist must live on the device")
        sigma = torch.empty((m,), dtype=torch.float64, device=dist.device)
        rho = torch.empty((m,), dtype=torch.float64, device=dist.device)
        suf = "f32" if dt == torch.float32 else "f64"
        nnz = C.c_uint64()
        dp, di, dv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_umap_graph_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(indices.data_ptr() if m else None), C.c_void_p(dist.data_ptr() if m else None),
            C.c_uint32(K), C.c_uint32(int(n_neighbors)), C.byref(nnz), C.byref(dp), C.byref(di), C.byref(dv),
            C.c_void_p(sigma.data_ptr() if m else None), C.c_void_p(rho.data_ptr() if m else None)))
        G = ResidentCsr(self, (m, m), nnz.value, np.float32 if suf == "f32" else np.float64, dp.value or 0, di.value or 0, dv.value or 0)
        return G, sigma, rho

    def umap_embed(self, G, n_epochs=None, output_dim=2, init="random", negative_sample_rate=5, learning_rate=1.0,
                   repulsion_strength=1.0, min_dist=0.1, spread=1.0, a=None, b=None, seed=None):
        """sapca_umap_embed_device_*: Y for the symmetric graph G (a ResidentCsr): the layout alone.  init: "random", or an
        m x output_dim device tensor to start from (copied); "panel" needs the panel and is refused here."""
        import torch
        m = G.shape[0]
        o, given = self._umap_options(2, min_dist, spread, n_epochs, output_dim, init, negative_sample_rate, learning_rate,
                                      repulsion_strength, a, b, seed)
        D = int(output_dim)
        dt = torch.float32 if G.dtype == np.float32 else torch.float64
        if given is not None:
            if not (isinstance(given, torch.Tensor) and given.is_cuda and given.dtype == dt and tuple(given.shape) == (m, D)):
                raise ValueError(f"init must be a device tensor of shape {(m, D)} and dtype {dt}")
            Y = given.contiguous().clone()
        else:
            Y = torch.empty((m, D), dtype=dt, device=self._device())
        suf = "f32" if dt == torch.float32 else "f64"
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_umap_embed_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx), C.c_void_p(G.d_val), C.byref(o),
            C.c_void_p(Y.data_ptr() if m else None)))
        return Y

    def umap(self, X, n_neighbors=15, min_dist=0.1, spread=1.0, n_epochs=None, output_dim=2, init="panel", negative_sample_rate=5,
             learning_rate=1.0, repulsion_strength=1.0, a=None, b=None, seed=None):
        """sapca_umap_device_* / sapca_umap_*: Y, the UMAP embedding of the rows of X.  X: an m x d torch device tensor of
        float32 / float64 with contiguous rows (a column slice of the scores is searched in place; Y is a device tensor), or a
        numpy array (the host route; Y is a numpy array).  init: "panel" (the first output_dim columns of X scaled to 0 .. 10),
        "random" (under `seed`, the Session's by default), or the initial embedding in the same kind of array.  n_epochs None:
        500 for at most 10000 rows, else 200.  a, b None: fitted from (spread, min_dist).  The same bytes from call to call."""
        o, given = self._umap_options(n_neighbors, min_dist, spread, n_epochs, output_dim, init, negative_sample_rate, learning_rate,
                                      repulsion_strength, a, b, seed)
        D = int(output_dim)
        if isinstance(X, np.ndarray):
            if X.ndim != 2 or X.dtype not in _SUF:
                raise ValueError(f"X must be a two-dimensional float32 / float64 array, got {X.dtype} {X.shape}")
            X = np.ascontiguousarray(X)
            m, d = X.shape
            Y = np.zeros((m, D), dtype=X.dtype)
            if given is not None:
                given = np.asarray(given)
                if given.shape != (m, D):
                    raise ValueError(f"init must have shape {(m, D)}, got {given.shape}")
                Y[...] = given
            suf, ct = _SUF[X.dtype]
            L.check(self._h, getattr(L.load(), f"sapca_umap_{suf}")(
                self._h, C.c_uint64(m), C.c_uint64(d), X.ctypes.data_as(C.c_void_p), C.byref(o), Y.ctypes.data_as(C.c_void_p)))
            return Y
        import torch
        m, d, ld, dt = _knn_panel("X", X)
        if not X.is_cuda:
            raise ValueError(f"X must live on the device (a CUDA tensor) or be a numpy array, got a tensor on {X.device}")
        if given is not None:
            if not (isinstance(given, torch.Tensor) and given.is_cuda and given.dtype == dt and tuple(given.shape) == (m, D)):
                raise ValueError(f"init must be a device tensor of shape {(m, D)} and dtype {dt}")
            Y = given.contiguous().clone()
        else:
            Y = torch.empty((m, D), dtype=dt, device=X.device)
        suf = "f32" if dt == torch.float32 else "f64"
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_umap_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(X.data_ptr() if m else None), C.c_uint64(ld), C.c_uint64(d), C.byref(o),
            C.c_void_p(Y.data_ptr() if m else None)))
        return Y

    # ---- k-means (sapca_kmeans_*): seeding, one assignment, one update, the whole run ----
    @staticmethod
    def _kmeans_shape(name, X, n_clusters, at_most_rows):
        """(m, d, ld, torch dtype, suffix) of a device panel and a number of clusters, checked on the host: ValueError."""
        import torch
        m, d, ld, dt = _knn_panel(name, X)
        k = int(n_clusters)
        if k < 1:
            raise ValueError(f"n_clusters must be at least 1, got {n_clusters}")
        if k > L.KMEANS_MAX_CLUSTERS:
            raise ValueError(f"n_clusters = {k} exceeds the {L.KMEANS_MAX_CLUSTERS} the library supports")
        if at_most_rows and m and k > m:
            raise ValueError(f"n_clusters = {k} exceeds the {m} rows of {name}")
        if d < 1 or d > 1024:
            raise ValueError(f"{name} has {d} columns; 1 .. 1024 are supported")
        if not X.is_cuda:   # (last: everything above is checked without a device)
            raise ValueError(f"{name} must live on the device (a CUDA tensor), got a tensor on {X.device}")
        return m, d, ld, dt, "f32" if dt == torch.float32 else "f64"

    @staticmethod
    def _kmeans_centroids(C_, k, d, dt, device):
        import torch
        if not (isinstance(C_, torch.Tensor) and C_.dtype == dt and tuple(C_.shape) == (k, d) and C_.device == device):
            raise ValueError(f"centroids must be a device tensor of shape {(k, d)} and dtype {dt} beside the rows")
        return C_.contiguous()

    def kmeans_seed(self, X, n_clusters, seed=None):
        """sapca_kmeans_seed_device_*: (centroids, rows) -- the k-means++ centres of the rows of the device panel X under the
        uniforms hash_u01(seed, 21, t) (the Session's seed by default): n_clusters x d copies of rows of X, and their int32
        row numbers."""
        import torch
        m, d, ld, dt, suf = self._kmeans_shape("X", X, n_clusters, True)
        k = int(n_clusters)
        cen = torch.empty((k, d), dtype=dt, device=X.device)
        rows = torch.empty((k,), dtype=torch.int32, device=X.device)
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_kmeans_seed_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(X.data_ptr() if m else None), C.c_uint64(ld), C.c_uint64(d), C.c_uint32(k),
            C.c_uint32(int(self._seed if seed is None else seed)), C.c_void_p(cen.data_ptr()), C.c_void_p(rows.data_ptr())))
        return cen, rows

    def kmeans_assign(self, X, centroids):
        """sapca_kmeans_assign_device_* (also the out-of-sample predict): (labels, dist2, inertia, n_ambiguous) -- for every row
        of the device panel X the nearest of the centroids (k x d device tensor), ties to the lower index, as an int32 device
        tensor; its squared distance (the direct formula in f64, rounded once); their f64 sum; and the number of rows the
        matrix-core ranking left to the f64 pass."""
        import torch
        if not isinstance(centroids, torch.Tensor) or centroids.dim() != 2:
            raise ValueError("centroids must be a two-dimensional device tensor")
        m, d, ld, dt, suf = self._kmeans_shape("X", X, centroids.shape[0], False)
        k = int(centroids.shape[0])
        cen = self._kmeans_centroids(centroids, k, d, dt, X.device)
        labels = torch.empty((m,), dtype=torch.int32, device=X.device)
        dist2 = torch.empty((m,), dtype=dt, device=X.device)
        inertia, namb = C.c_double(), C.c_uint64()
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_kmeans_assign_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(X.data_ptr() if m else None), C.c_uint64(ld), C.c_uint64(d), C.c_uint32(k),
            C.c_void_p(cen.data_ptr()), C.c_void_p(labels.data_ptr() if m else None), C.c_void_p(dist2.data_ptr() if m else None),
            C.byref(inertia), C.byref(namb)))
        return labels, dist2, inertia.value, namb.value

    def kmeans_update(self, X, labels, centroids):
        """sapca_kmeans_update_device_*: (centroids, counts) -- the means of the rows of X under `labels` (int32 device tensor;
        a label outside [0, k) belongs to no cluster), summed and divided in f64 and rounded once; a cluster without rows keeps
        its row of `centroids` (k x d device tensor, not modified: a copy is updated).  counts: int64 device tensor."""
        import torch
        if not isinstance(centroids, torch.Tensor) or centroids.dim() != 2:
            raise ValueError("centroids must be a two-dimensional device tensor")
        m, d, ld, dt, suf = self._kmeans_shape("X", X, centroids.shape[0], False)
        k = int(centroids.shape[0])
        if not (isinstance(labels, torch.Tensor) and labels.dtype == torch.int32 and tuple(labels.shape) == (m,)
                and labels.is_contiguous() and labels.device == X.device):
            raise ValueError(f"labels must be a contiguous int32 device tensor of {m} entries beside the rows")
        cen = self._kmeans_centroids(centroids, k, d, dt, X.device).clone()
        counts = torch.zeros((k,), dtype=torch.int64, device=X.device)
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_kmeans_update_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(X.data_ptr() if m else None), C.c_uint64(ld), C.c_uint64(d), C.c_uint32(k),
            C.c_void_p(labels.data_ptr() if m else None), C.c_void_p(cen.data_ptr()), C.c_void_p(counts.data_ptr())))
        return cen, counts

    def kmeans(self, X, n_clusters=8, init="k-means++", max_iter=300, tol=1e-4, seed=None):
        """sapca_kmeans_device_* / sapca_kmeans_*: (labels, centroids, inertia, n_iter) -- Lloyd's k-means of the rows of X
        (include/sapca.h states the algorithm; scikit-learn's rule, n_iter included, except that an empty cluster keeps its
        centroid).  X: an m x d torch device tensor of float32 / float64 with contiguous rows (a column slice of the scores is
        clustered in place; labels and centroids are device tensors), or a numpy array (the host route; numpy arrays back).
        init: "k-means++" (seeded by `seed`, the Session's by default) or an n_clusters x d array of centroids (a numpy
        array, or beside device rows a device tensor).  The same bytes from call to call."""
        o = L.default_kmeans_options()
        o.random_seed = int(self._seed if seed is None else seed)
        k = int(n_clusters)
        given = not isinstance(init, str)
        if not given and init != "k-means++":
            raise ValueError(f"unknown init {init!r}: 'k-means++' or an array of centroids")
        if int(max_iter) < 0:
            raise ValueError(f"max_iter must not be negative, got {max_iter}")
        if not (float(tol) >= 0.0 and np.isfinite(float(tol))):
            raise ValueError(f"tol must be finite and not negative, got {tol}")
        o.init, o.max_iter, o.tol = (L.KMEANS_GIVEN if given else L.KMEANS_PLUSPLUS), int(max_iter), float(tol)
        inertia, n_iter = C.c_double(), C.c_uint64()
        if isinstance(X, np.ndarray):
            if X.ndim != 2 or X.dtype not in _SUF:
                raise ValueError(f"X must be a two-dimensional float32 / float64 array, got {X.dtype} {X.shape}")
            X = np.ascontiguousarray(X)
            m, d = X.shape
            if k < 1 or k > L.KMEANS_MAX_CLUSTERS or (m and k > m):
                raise ValueError(f"n_clusters = {n_clusters} must lie in 1 .. min({L.KMEANS_MAX_CLUSTERS}, the {m} rows)")
            if d < 1 or d > 1024:
                raise ValueError(f"X has {d} columns; 1 .. 1024 are supported")
            o.n_clusters = k
            cen = np.zeros((k, d), dtype=X.dtype)
            if given:
                init = np.asarray(init)
                if init.shape != (k, d):
                    raise ValueError(f"init must have shape {(k, d)}, got {init.shape}")
                cen[...] = init
            labels = np.zeros((m,), dtype=np.int32)
            suf, ct = _SUF[X.dtype]
            L.check(self._h, getattr(L.load(), f"sapca_kmeans_{suf}")(
                self._h, C.c_uint64(m), C.c_uint64(d), X.ctypes.data_as(C.c_void_p), C.byref(o), cen.ctypes.data_as(C.c_void_p),
                labels.ctypes.data_as(C.c_void_p), C.byref(inertia), C.byref(n_iter)))
            return labels, cen, inertia.value, n_iter.value
        import torch
        m, d, ld, dt, suf = self._kmeans_shape("X", X, k, True)
        o.n_clusters = k
        if given and not isinstance(init, torch.Tensor):   # a host array of centroids beside device rows: uploaded
            init = np.asarray(init)
            if init.shape != (k, d):
                raise ValueError(f"init must have shape {(k, d)}, got {init.shape}")
            init = torch.as_tensor(init, device=X.device).to(dt)
        cen = self._kmeans_centroids(init, k, d, dt, X.device).clone() if given else torch.empty((k, d), dtype=dt, device=X.device)
        labels = torch.empty((m,), dtype=torch.int32, device=X.device)
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_kmeans_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(X.data_ptr() if m else None), C.c_uint64(ld), C.c_uint64(d), C.byref(o),
            C.c_void_p(cen.data_ptr()), C.c_void_p(labels.data_ptr() if m else None), C.byref(inertia), C.byref(n_iter)))
        return labels, cen, inertia.value, n_iter.value

    # ---- Harmony (sapca_harmony_*): one clustering pass, the centroids, the correction, the whole run ----
    @staticmethod
    def _harmony_batch(batch, m, device):
        """The batch labels as they are where they are a contiguous int32 device tensor beside the rows (what k-means or the
        user left on the device); anything else is converted and uploaded."""
        import torch
        if not isinstance(batch, torch.Tensor):
            batch = torch.as_tensor(np.ascontiguousarray(np.asarray(batch), dtype=np.int32))
        if batch.dim() != 1 or int(batch.shape[0]) != m:
            raise ValueError(f"batch must hold one label per row ({m}), got shape {tuple(batch.shape)}")
        if batch.dtype != torch.int32 or batch.device != device or not batch.is_contiguous():
            batch = batch.to(device=device, dtype=torch.int32).contiguous()
        return batch

    @staticmethod
    def _harmony_panel(name, t, rows, cols, dt, device):
        import torch
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == (rows, cols) and t.device == device):
            raise ValueError(f"{name} must be a device tensor of shape {(rows, cols)} and dtype {dt} beside the rows")
        return t.contiguous()

    @staticmethod
    def _harmony_rows(name, X):
        import torch
        m, d, ld, dt = _knn_panel(name, X)
        if not X.is_cuda:
            raise ValueError(f"{name} must live on the device (a CUDA tensor), got a tensor on {X.device}")
        return m, d, ld, dt, "f32" if dt == torch.float32 else "f64"

    def harmony_centroids(self, Zc, R):
        """sapca_harmony_centroids_device_*: normalise_rows(R^T Zc) as a K x d device tensor; Zc: m x d device rows (unit
        norm), R: m x K device tensor of the same dtype.  The sums are f64 in a fixed order."""
        import torch
        m, d, ld, dt, suf = self._harmony_rows("Zc", Zc)
        if not isinstance(R, torch.Tensor) or R.dim() != 2:
            raise ValueError("R must be a two-dimensional device tensor")
        K = int(R.shape[1])
        R = self._harmony_panel("R", R, m, K, dt, Zc.device)
        Y = torch.zeros((K, d), dtype=dt, device=Zc.device)
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_harmony_centroids_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(Zc.data_ptr() if m else None), C.c_uint64(ld), C.c_uint64(d), C.c_uint32(K),
            C.c_void_p(R.data_ptr() if m else None), C.c_void_p(Y.data_ptr())))
        return Y

    def harmony_assign(self, Zc, batch, n_batches, R, Y=None, theta=2.0, sigma=0.1, n_blocks=20, seed=None, pass_index=0):
        """sapca_harmony_assign_device_*: one clustering pass (item 2 of include/sapca.h) -> (R, Y, O, rs, objective).  Zc: m x d
        device rows of unit norm; batch: m labels in [0, n_batches); R: the m x K assignment going in (not modified: a copy is
        updated); Y: K x d unit centroids used as given, or None to recompute them from R.  O (n_batches x K), rs (K) and the
        three terms of the objective come back as numpy f64 arrays."""
        import torch
        m, d, ld, dt, suf = self._harmony_rows("Zc", Zc)
        if not isinstance(R, torch.Tensor) or R.dim() != 2:
            raise ValueError("R must be a two-dimensional device tensor")
        K, B = int(R.shape[1]), int(n_batches)
        R = self._harmony_panel("R", R, m, K, dt, Zc.device).clone()
        recompute = Y is None
        Y = torch.zeros((K, d), dtype=dt, device=Zc.device) if recompute else self._harmony_panel("Y", Y, K, d, dt, Zc.device).clone()
        batch = self._harmony_batch(batch, m, Zc.device)
        O = np.zeros((max(B, 0), K), dtype=np.float64)
        rs = np.zeros((K,), dtype=np.float64)
        obj = np.zeros((3,), dtype=np.float64)
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_harmony_assign_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(Zc.data_ptr() if m else None), C.c_uint64(ld), C.c_uint64(d),
            C.c_void_p(batch.data_ptr() if m else None), C.c_uint32(B), C.c_uint32(K), C.c_void_p(Y.data_ptr()),
            C.c_int32(1 if recompute else 0), C.c_void_p(R.data_ptr() if m else None), C.c_double(float(theta)), C.c_double(float(sigma)),
            C.c_uint32(int(n_blocks)), C.c_uint32(int(self._seed if seed is None else seed)), C.c_uint64(int(pass_index)),
            O.ctypes.data_as(C.c_void_p), rs.ctypes.data_as(C.c_void_p), obj.ctypes.data_as(C.c_void_p)))
        return R, Y, O, rs, obj

    def harmony_correct(self, Z, batch, n_batches, R, lam=1.0):
        """sapca_harmony_correct_device_*: the mixture-of-experts ridge correction (item 5) -> (Zcorr, beta).  Z: m x d device
        rows (a column slice of the scores is read in place), R: m x K; Zcorr is a new m x d device tensor, beta the K x
        n_batches x d coefficients as a numpy f64 array."""
        import torch
        m, d, ld, dt, suf = self._harmony_rows("Z", Z)
        if not isinstance(R, torch.Tensor) or R.dim() != 2:
            raise ValueError("R must be a two-dimensional device tensor")
        K, B = int(R.shape[1]), int(n_batches)
        R = self._harmony_panel("R", R, m, K, dt, Z.device)
        batch = self._harmony_batch(batch, m, Z.device)
        out = torch.empty((m, d), dtype=dt, device=Z.device)
        beta = np.zeros((K, max(B, 0), d), dtype=np.float64)
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_harmony_correct_device_{suf}")(
            self._h, C.c_uint64(m), C.c_void_p(Z.data_ptr() if m else None), C.c_uint64(ld), C.c_uint64(d),
            C.c_void_p(batch.data_ptr() if m else None), C.c_uint32(B), C.c_uint32(K), C.c_void_p(R.data_ptr() if m else None),
            C.c_double(float(lam)), C.c_void_p(out.data_ptr() if m else None), C.c_uint64(d), beta.ctypes.data_as(C.c_void_p)))
        return out, beta

    def harmony(self, X, batch, n_clusters=None, n_batches=None, init="kmeans", theta=2.0, sigma=0.1, lam=1.0, n_blocks=20,
                max_iter_harmony=10, max_iter_cluster=20, epsilon_cluster=1e-5, epsilon_harmony=1e-4, seed=None):
        """sapca_harmony_device_* / sapca_harmony_*: (Zcorr, result) -- Harmony batch integration of the score rows X
        (include/sapca.h states the algorithm and its deviations from harmonypy; what scanpy.external.pp.harmony_integrate
        does between the PCA and `neighbors`).  X: an m x d torch device tensor of float32 / float64 with contiguous rows (a
        column slice of the scores is read in place; the corrected panel is a new device tensor), or a numpy array (the host
        route; a numpy array back).  batch: one integer label per row in [0, n_batches) -- an int32 device tensor is taken as
        it is; n_batches defaults to the largest label + 1.  n_clusters defaults to min(round(m / 30), 100), at least 1.  init:
        "kmeans" (this library's k-means++ / Lloyd under `seed`) or an n_clusters x d array of centroids.  result: a
        HarmonyResult with R (m x K), centroids (K x d), objectives, passes, n_iter, converged.  The same bytes from call to call."""
        given = not isinstance(init, str)
        if not given and init != "kmeans":
            raise ValueError(f"unknown init {init!r}: 'kmeans' or an array of centroids")
        host = isinstance(X, np.ndarray)
        if host:
            if X.ndim != 2 or X.dtype not in _SUF:
                raise ValueError(f"X must be a two-dimensional float32 / float64 array, got {X.dtype} {X.shape}")
            X = np.ascontiguousarray(X)
            m, d = X.shape
        else:
            import torch
            m, d, ld, dt, suf = self._harmony_rows("X", X)
        K = max(1, min(int(round(m / 30.0)), 100)) if n_clusters is None else int(n_clusters)
        if K < 0 or int(max_iter_harmony) < 0 or int(max_iter_cluster) < 0 or int(n_blocks) < 0:
            raise ValueError("n_clusters, n_blocks and the iteration limits must not be negative")
        if host:
            batch = np.ascontiguousarray(np.asarray(batch), dtype=np.int32)
            if batch.shape != (m,):
                raise ValueError(f"batch must hold one label per row ({m}), got shape {batch.shape}")
            B = (int(batch.max()) + 1 if m else 1) if n_batches is None else int(n_batches)
        else:
            batch = self._harmony_batch(batch, m, X.device)
            B = (int(batch.max().item()) + 1 if m else 1) if n_batches is None else int(n_batches)
        B = max(B, 0)
        objectives = np.zeros((max(int(max_iter_harmony), 1),), dtype=np.float64)
        passes = np.zeros((max(int(max_iter_harmony), 1),), dtype=np.uint32)
        n_iter, converged = C.c_uint32(), C.c_int32()
        scalars = (C.c_uint32(B), C.c_uint32(K), C.c_uint32(L.HARMONY_GIVEN if given else L.HARMONY_KMEANS), C.c_double(float(theta)),
                   C.c_double(float(sigma)), C.c_double(float(lam)), C.c_uint32(int(n_blocks)), C.c_uint32(int(max_iter_harmony)),
                   C.c_uint32(int(max_iter_cluster)), C.c_double(float(epsilon_cluster)), C.c_double(float(epsilon_harmony)),
                   C.c_uint32(int(self._seed if seed is None else seed)))
        tail = (objectives.ctypes.data_as(C.c_void_p), passes.ctypes.data_as(C.c_void_p), C.byref(n_iter), C.byref(converged))
        if host:
            suf = _SUF[X.dtype][0]
            Y = np.zeros((K, d), dtype=X.dtype)
            if given:
                init = np.asarray(init)
                if init.shape != (K, d):
                    raise ValueError(f"init must have shape {(K, d)}, got {init.shape}")
                Y[...] = init
            out = np.zeros((m, d), dtype=X.dtype)
            R = np.zeros((m, K), dtype=X.dtype)
            L.check(self._h, getattr(L.load(), f"sapca_harmony_{suf}")(
                self._h, C.c_uint64(m), C.c_uint64(d), X.ctypes.data_as(C.c_void_p), batch.ctypes.data_as(C.c_void_p), *scalars,
                out.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), Y.ctypes.data_as(C.c_void_p), *tail))
        else:
            if given and not isinstance(init, torch.Tensor):   # a host array of centroids beside device rows: uploaded
                init = np.asarray(init)
                if init.shape != (K, d):
                    raise ValueError(f"init must have shape {(K, d)}, got {init.shape}")
                init = torch.as_tensor(init, device=X.device).to(dt)
            Y = self._harmony_panel("init", init, K, d, dt, X.device).clone() if given else torch.zeros((K, d), dtype=dt, device=X.device)
            out = torch.empty((m, d), dtype=dt, device=X.device)
            R = torch.zeros((m, K), dtype=dt, device=X.device)
            torch.cuda.current_stream().synchronize()
            L.check(self._h, getattr(L.load(), f"sapca_harmony_device_{suf}")(
                self._h, C.c_uint64(m), C.c_void_p(X.data_ptr() if m else None), C.c_uint64(ld), C.c_uint64(d),
                C.c_void_p(batch.data_ptr() if m else None), *scalars, C.c_void_p(out.data_ptr() if m else None), C.c_uint64(d),
                C.c_void_p(R.data_ptr() if m else None), C.c_void_p(Y.data_ptr()), *tail))
        n = int(n_iter.value)
        return out, HarmonyResult(R, Y, objectives[:n].copy(), passes[:n].astype(np.int64), n, bool(converged.value))

    # ---- Louvain (sapca_louvain_*): the modularity of labels, one sweep, one aggregation, the whole run ----
    @staticmethod
    def _louvain_graph(G):
        if not isinstance(G, ResidentCsr) or G.shape[0] != G.shape[1]:
            raise ValueError("the graph must be a square ResidentCsr (what umap_graph returns)")
        return G.shape[0], _SUF[G.dtype][0]

    @staticmethod
    def _louvain_labels(labels, m):
        import torch
        if isinstance(labels, np.ndarray):
            labels = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.int32), device="cuda")
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == (m,)
                and labels.is_contiguous()):
            raise ValueError(f"labels must be {m} contiguous int32 values (a device tensor or a numpy array)")
        return labels

    @staticmethod
    def _louvain_gamma(resolution):
        if not (float(resolution) >= 0.0 and np.isfinite(float(resolution))):
            raise ValueError(f"resolution must be finite and not negative, got {resolution}")
        return float(resolution)

    def modularity(self, G, labels, resolution=1.0):
        """sapca_louvain_modularity_device_*: Q of `labels` (m int32: a device tensor, or a numpy array that is uploaded) on the
        symmetric graph G (a ResidentCsr), at the given resolution: scores any labels, k-means' for instance."""
        import torch
        m, suf = self._louvain_graph(G)
        gamma = self._louvain_gamma(resolution)
        labels = self._louvain_labels(labels, m)
        q = C.c_double()
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_louvain_modularity_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx), C.c_void_p(G.d_val),
            C.c_void_p(labels.data_ptr() if m else None), C.c_double(gamma), C.byref(q)))
        return q.value

    def louvain_sweep(self, G, labels, seed=None, level=0, sweep=0, resolution=1.0):
        """sapca_louvain_sweep_device_*: (labels', n_moved) -- one hashed half-active sweep from `labels`, no keep / undo."""
        import torch
        m, suf = self._louvain_graph(G)
        gamma = self._louvain_gamma(resolution)
        labels = self._louvain_labels(labels, m)
        out = torch.empty_like(labels)
        moved = C.c_uint64()
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_louvain_sweep_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx), C.c_void_p(G.d_val),
            C.c_void_p(labels.data_ptr() if m else None), C.c_uint32(int(self._seed if seed is None else seed)), C.c_uint32(int(level)),
            C.c_uint32(int(sweep)), C.c_double(gamma), C.c_void_p(out.data_ptr() if m else None), C.byref(moved)))
        return out, moved.value

    def louvain_aggregate(self, G, labels):
        """sapca_louvain_aggregate_device_*: (coarse graph, renumbered labels) -- the communities of `labels` as vertices, f64
        values whatever G's; a ResidentCsr in the Session's Louvain buffers, valid until the next Louvain call."""
        import torch
        m, suf = self._louvain_graph(G)
        labels = self._louvain_labels(labels, m)
        ren = torch.empty_like(labels)
        n_out, nnz = C.c_uint64(), C.c_uint64()
        dp, di, dv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_louvain_aggregate_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx), C.c_void_p(G.d_val),
            C.c_void_p(labels.data_ptr() if m else None), C.byref(n_out), C.byref(nnz), C.byref(dp), C.byref(di), C.byref(dv),
            C.c_void_p(ren.data_ptr() if m else None)))
        return ResidentCsr(self, (n_out.value, n_out.value), nnz.value, np.float64, dp.value or 0, di.value or 0, dv.value or 0), ren

    def _louvain_options(self, resolution, tol, max_sweeps, max_levels, seed):
        o = L.default_louvain_options()
        o.random_seed = int(self._seed if seed is None else seed)
        o.resolution = self._louvain_gamma(resolution)
        if not (float(tol) >= 0.0 and np.isfinite(float(tol))):
            raise ValueError(f"tol must be finite and not negative, got {tol}")
        if not 1 <= int(max_sweeps) <= 4096:
            raise ValueError(f"max_sweeps = {max_sweeps} is outside 1 .. 4096")
        if max_levels is not None and not 1 <= int(max_levels) <= 64:
            raise ValueError(f"max_levels = {max_levels} is outside 1 .. 64")
        o.tol, o.max_sweeps, o.max_levels = float(tol), int(max_sweeps), 0 if max_levels is None else int(max_levels)
        return o

    def louvain(self, G_or_X, resolution=1.0, tol=1e-7, max_sweeps=256, max_levels=None, seed=None, n_neighbors=15):
        """sapca_louvain_device_*: (labels, n_communities, modularity, n_levels) -- Louvain communities (include/sapca.h states
        the algorithm) of a symmetric graph.  A ResidentCsr is clustered as it is; an m x d device panel goes through knn
        (Euclidean, self excluded, n_neighbors - 1), umap_graph and then the run.  labels: m int32 on the device.  The same bytes
        from call to call."""
        import torch
        o = self._louvain_options(resolution, tol, max_sweeps, max_levels, seed)
        G = G_or_X
        if not isinstance(G, ResidentCsr):
            idx, dist = self.knn(G_or_X, n_neighbors=int(n_neighbors) - 1, metric="euclidean", exclude_self=True)
            G = self.umap_graph(idx, dist, int(n_neighbors))[0]
        m, suf = self._louvain_graph(G)
        labels = torch.empty((m,), dtype=torch.int32, device=self._device())
        ncomm, q, levels = C.c_uint64(), C.c_double(), C.c_uint32()
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_louvain_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx), C.c_void_p(G.d_val), C.byref(o),
            C.c_void_p(labels.data_ptr() if m else None), C.byref(ncomm), C.byref(q), C.byref(levels)))
        return labels, ncomm.value, q.value, levels.value

    def louvain_host(self, indptr, indices, data, resolution=1.0, tol=1e-7, max_sweeps=256, max_levels=None, seed=None):
        """sapca_louvain_*: the same with a host CSR in (scipy's three arrays) and host labels out."""
        o = self._louvain_options(resolution, tol, max_sweeps, max_levels, seed)
        data = np.ascontiguousarray(data)
        if data.dtype not in _SUF:
            raise ValueError(f"data must be float32 / float64, got {data.dtype}")
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        m = len(indptr) - 1
        labels = np.zeros((m,), dtype=np.int32)
        ncomm, q, levels = C.c_uint64(), C.c_double(), C.c_uint32()
        L.check(self._h, getattr(L.load(), f"sapca_louvain_{_SUF[data.dtype][0]}")(
            self._h, C.c_uint64(m), C.c_uint64(len(data)), indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p),
            data.ctypes.data_as(C.c_void_p), C.byref(o), labels.ctypes.data_as(C.c_void_p), C.byref(ncomm), C.byref(q), C.byref(levels)))
        return labels, ncomm.value, q.value, levels.value

    # ---- spectral embedding / diffusion maps (sapca_graph_components_device, sapca_spectral_*): components, scale, operator,
    # the eigen-solve, the diffusion map and UMAP's spectral start ----
    @staticmethod
    def _spectral_kind(kind):
        if not isinstance(kind, str) or kind.lower() not in L.SPECTRAL_KINDS:
            raise ValueError(f"unknown kind {kind!r}: one of {sorted(L.SPECTRAL_KINDS)}")
        return L.SPECTRAL_KINDS[kind.lower()]

    def _spectral_options(self, n_eigen, kind, tol, max_steps, seed, single_round=False):
        o = L.default_spectral_options()
        o.single_round = 1 if single_round else 0
        o.kind = self._spectral_kind(kind)
        if not 1 <= int(n_eigen) <= 64:
            raise ValueError(f"n_eigen = {n_eigen} is outside 1 .. 64")
        if not (float(tol) >= 0.0 and np.isfinite(float(tol))):
            raise ValueError(f"tol must be finite and not negative, got {tol}")
        if max_steps is not None and not 1 <= int(max_steps) <= 4096:
            raise ValueError(f"max_steps = {max_steps} is outside 1 .. 4096")
        o.random_seed = int(self._seed if seed is None else seed)
        o.n_eigen, o.tol, o.max_steps = int(n_eigen), float(tol), 0 if max_steps is None else int(max_steps)
        return o

    def graph_components(self, G):
        """sapca_graph_components_device: (labels, n_components) of the structure of the square graph G (a ResidentCsr; every
        stored entry is an edge).  labels: m int32 on the device, components numbered in ascending order of their smallest
        vertex, as scipy.sparse.csgraph.connected_components(directed=False) numbers them."""
        import torch
        m, _ = self._louvain_graph(G)
        labels = torch.empty((m,), dtype=torch.int32, device=self._device())
        n = C.c_uint64()
        torch.cuda.current_stream().synchronize()
        L.check(self._h, L.load().sapca_graph_components_device(
            self._h, C.c_uint64(m), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx),
            C.c_void_p(labels.data_ptr() if m else None), C.byref(n)))
        return labels, n.value

    def spectral_scale(self, G, kind="normalized"):
        """sapca_spectral_scale_device_*: s (m f64 on the device) of S = diag(s) G diag(s): "normalized" 1 / sqrt(d), "diffmap"
        1 / (q sqrt(z)) (include/sapca.h, "Spectral"); 0 for a vertex whose sums are not finite and positive."""
        import torch
        code = self._spectral_kind(kind)
        m, suf = self._louvain_graph(G)
        sc = torch.empty((m,), dtype=torch.float64, device=self._device())
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_spectral_scale_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx), C.c_void_p(G.d_val),
            C.c_uint32(code), C.c_void_p(sc.data_ptr() if m else None)))
        return sc

    def spectral_apply(self, G, x, kind="normalized"):
        """sapca_spectral_apply_device_*: y = S x for m f64 values x on the device (the short-row product of a Lanczos step)."""
        import torch
        code = self._spectral_kind(kind)
        m, suf = self._louvain_graph(G)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and tuple(x.shape) == (m,) and x.is_contiguous()):
            raise ValueError(f"x must be {m} contiguous float64 values on the device")
        y = torch.empty_like(x)
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_spectral_apply_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx), C.c_void_p(G.d_val),
            C.c_uint32(code), C.c_void_p(x.data_ptr() if m else None), C.c_void_p(y.data_ptr() if m else None)))
        return y

    def spectral(self, G, n_eigen=16, kind="normalized", tol=1e-8, max_steps=None, seed=None, single_round=False):
        """sapca_spectral_device_*: (evals, evecs, n_components, n_steps) -- the n_eigen leading eigenpairs of S = diag(s) G diag(s)
        for the symmetric graph G (a ResidentCsr).  evals: n_eigen f64 (numpy, descending); evecs: m x n_eigen on the device in
        G's dtype, one exact pair (eigenvalue 1.0) per connected component first, the sign of every other vector fixed by its
        entry of largest magnitude.  max_steps None: min(m, 1000).  The same bytes from call to call.  The solve runs Lanczos
        rounds until no copy of a repeated eigenvalue is missed (n_steps: their sum); single_round=True stops after the first,
        which is right only where the leading eigenvalues are simple."""
        import torch
        o = self._spectral_options(n_eigen, kind, tol, max_steps, seed, single_round)
        m, suf = self._louvain_graph(G)
        if m and o.n_eigen > m:
            raise ValueError(f"n_eigen = {n_eigen} exceeds m = {m}")
        dt = torch.float32 if suf == "f32" else torch.float64
        evecs = torch.empty((m, o.n_eigen), dtype=dt, device=self._device())
        evals = np.zeros((o.n_eigen,), dtype=np.float64)
        ncomp, steps = C.c_uint64(), C.c_uint32()
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_spectral_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint64(G.nnz), C.c_void_p(G.d_ptr), C.c_void_p(G.d_idx), C.c_void_p(G.d_val), C.byref(o),
            _p(evals, C.c_double), C.c_void_p(evecs.data_ptr() if m else None), C.byref(ncomp), C.byref(steps)))
        return evals, evecs, ncomp.value, steps.value

    def spectral_host(self, indptr, indices, data, n_eigen=16, kind="normalized", tol=1e-8, max_steps=None, seed=None,
                      single_round=False):
        """sapca_spectral_*: the same with a host CSR in (scipy's three arrays) and host eigenvectors out."""
        o = self._spectral_options(n_eigen, kind, tol, max_steps, seed, single_round)
        data = np.ascontiguousarray(data)
        if data.dtype not in _SUF:
            raise ValueError(f"data must be float32 / float64, got {data.dtype}")
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        m = len(indptr) - 1
        if m and o.n_eigen > m:
            raise ValueError(f"n_eigen = {n_eigen} exceeds m = {m}")
        evecs = np.zeros((m, o.n_eigen), dtype=data.dtype)
        evals = np.zeros((o.n_eigen,), dtype=np.float64)
        ncomp, steps = C.c_uint64(), C.c_uint32()
        L.check(self._h, getattr(L.load(), f"sapca_spectral_{_SUF[data.dtype][0]}")(
            self._h, C.c_uint64(m), C.c_uint64(len(data)), indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p),
            data.ctypes.data_as(C.c_void_p), C.byref(o), _p(evals, C.c_double), evecs.ctypes.data_as(C.c_void_p), C.byref(ncomp),
            C.byref(steps)))
        return evals, evecs, ncomp.value, steps.value

    def diffmap(self, G_or_X, n_comps=15, n_neighbors=15, tol=1e-8, max_steps=None, seed=None):
        """(X_diffmap, evals) -- scanpy's tl.diffmap: the n_comps leading eigenpairs of the density-normalised symmetric transition
        matrix (spectral(kind="diffmap")) of a symmetric graph.  A ResidentCsr is taken as it is; an m x d device panel goes
        through knn (Euclidean, self excluded, n_neighbors - 1) and umap_graph first, as louvain does.  The largest algebraic
        eigenvalues are taken (scanpy's which="LM" would also admit values near -1)."""
        if not 1 <= int(n_comps) <= 64:
            raise ValueError(f"n_comps = {n_comps} is outside 1 .. 64")
        G = G_or_X
        if not isinstance(G, ResidentCsr):
            idx, dist = self.knn(G_or_X, n_neighbors=int(n_neighbors) - 1, metric="euclidean", exclude_self=True)
            G = self.umap_graph(idx, dist, int(n_neighbors))[0]
        evals, evecs, _, _ = self.spectral(G, n_eigen=int(n_comps), kind="diffmap", tol=tol, max_steps=max_steps, seed=seed)
        return evecs, evals

    def umap_spectral_init(self, G, output_dim=2, seed=None, tol=1e-8, max_steps=None):
        """sapca_umap_spectral_init_device_*: umap-learn's spectral start for the symmetric graph G, an m x output_dim device
        tensor to pass to umap_embed / umap as init=: eigenvectors 1 .. output_dim of spectral(kind="normalized") expanded to
        +-10 plus 1e-4 uniform noise under `seed`.  On a disconnected graph the leading eigenvectors are component indicators
        and umap-learn's per-component meta-layout is not built: a warning says so."""
        import warnings

        import torch
        D = int(output_dim)
        if not 1 <= D <= 3:
            raise ValueError(f"output_dim = {output_dim} is outside 1 .. 3")
        m, suf = self._louvain_graph(G)
        if m <= D:
            raise ValueError(f"the spectral start needs more than output_dim = {D} vertices, got m = {m}")
        seed = int(self._seed if seed is None else seed)
        _, evecs, ncomp, _ = self.spectral(G, n_eigen=D + 1, kind="normalized", tol=tol, max_steps=max_steps, seed=seed)
        if ncomp > 1:
            warnings.warn(f"umap_spectral_init: the graph has {ncomp} connected components; the start separates components only "
                          "(umap-learn's per-component meta-layout is not built)", RuntimeWarning, stacklevel=2)
        Y = torch.empty((m, D), dtype=evecs.dtype, device=evecs.device)
        torch.cuda.current_stream().synchronize()
        L.check(self._h, getattr(L.load(), f"sapca_umap_spectral_init_device_{suf}")(
            self._h, C.c_uint64(m), C.c_uint32(D), C.c_void_p(evecs.data_ptr()), C.c_uint64(D + 1), C.c_uint32(D + 1),
            C.c_uint32(seed), C.c_void_p(Y.data_ptr())))
        return Y

    # ---- local regression (sapca_loess_f64) ----
    def loess(self, x, y, span=0.3):
        """sapca_loess_f64: the local quadratic regression of y on x (host f64 arrays) fitted at every x_i on the device: the
        "direct" surface of Cleveland's loess, degree 2, tricube weights (include/sapca.h, "Variable genes").  Returns the
        fitted values, one per point."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if x.ndim != 1 or x.shape != y.shape:
            raise ValueError(f"x and y must be one-dimensional and alike, got shapes {x.shape} and {y.shape}")
        out = np.zeros(x.size)
        L.check(self._h, L.load().sapca_loess_f64(self._h, C.c_uint64(x.size), _p(x, C.c_double), _p(y, C.c_double),
                                                  C.c_double(float(span)), _p(out, C.c_double)))
        return out


ROW, COLUMN = 0, 1   # Direction of the reference's Normalize / statistics traits (src/utils.rs)


def _dense_codes(batches):
    """(labels in order of first appearance, int32 code of every entry of `batches`); labels may be any hashable values"""
    arr = batches if isinstance(batches, np.ndarray) else None
    if arr is None and len(batches) and all(type(b) is int for b in batches):
        arr = np.asarray(batches)
    if arr is not None and arr.ndim == 1 and arr.dtype.kind in "iub":
        uniq, first, codes = np.unique(arr, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")
        rank = np.empty_like(order)
        rank[order] = np.arange(order.size)
        return [uniq[j].item() for j in order], rank[codes.reshape(-1)].astype(np.int32)
    lut = {}
    codes = np.fromiter((lut.setdefault(b, len(lut)) for b in batches), dtype=np.int32, count=len(batches))
    return list(lut), codes


def _row_list(rows, m):
    """The row list of ResidentCsr.select_rows as the uint64 array the C ABI takes: a boolean array of length exactly m
    becomes its ascending true positions; an integer sequence passes through in its own order, repeats included.  Pure
    host code (numpy only): a mask of another length, a negative index, a sequence that is neither or has more than one
    dimension raise ValueError.  An index >= m is left to the library, which names it (SAPCA_ERR_ARG)."""
    a = np.asarray(rows)
    if a.ndim != 1:
        raise ValueError(f"rows must be one-dimensional, got shape {a.shape}")
    if a.dtype == np.bool_:
        if a.size != int(m):
            raise ValueError(f"Row mask length ({a.size}) does not match number of rows ({int(m)})")
        return np.flatnonzero(a).astype(np.uint64)
    if a.size == 0:
        return np.zeros(0, dtype=np.uint64)
    if a.dtype.kind not in "iu":
        raise ValueError(f"rows must be a boolean mask or integer indices, got dtype {a.dtype}")
    if a.dtype.kind == "i" and (a < 0).any():
        j = int(np.flatnonzero(a < 0)[0])
        raise ValueError(f"negative row index {int(a[j])} at position {j}")
    return np.ascontiguousarray(a, dtype=np.uint64)


def _col_mask(cols, n):
    """The column selection of ResidentCsr.select as the uint8 mask of length n the C ABI takes: a boolean array of length
    exactly n passes through; strictly ascending integer indices below n become the mask that is true at them (an empty
    list: all false).  The ABI takes a mask, not a list, because the result must stay canonical: kept columns are
    renumbered by rank, which is their order only when they ascend without repeats.  Pure host code (numpy only): a mask
    of another length, a negative index, one >= n, repeated or descending indices, and input that is neither raise
    ValueError."""
    a = np.asarray(cols)
    n = int(n)
    if a.ndim != 1:
        raise ValueError(f"cols must be one-dimensional, got shape {a.shape}")
    if a.dtype == np.bool_:
        if a.size != n:
            raise ValueError(f"Column mask length ({a.size}) does not match number of columns ({n})")
        return np.ascontiguousarray(a, dtype=np.uint8)
    mask = np.zeros(n, dtype=np.uint8)
    if a.size == 0:
        return mask
    if a.dtype.kind not in "iu":
        raise ValueError(f"cols must be a boolean mask or integer indices, got dtype {a.dtype}")
    if a.dtype.kind == "i" and (a < 0).any():
        j = int(np.flatnonzero(a < 0)[0])
        raise ValueError(f"negative column index {int(a[j])} at position {j}")
    a = a.astype(np.uint64)
    if a.size > 1 and (a[1:] <= a[:-1]).any():
        j = int(np.flatnonzero(a[1:] <= a[:-1])[0]) + 1
        raise ValueError(f"column indices must be strictly ascending: {int(a[j])} at position {j} follows {int(a[j - 1])} "
                         "(a mask keeps the result canonical; sort and deduplicate, or canonicalize a reordered matrix)")
    if int(a[-1]) >= n:
        raise ValueError(f"column index {int(a[-1])} is out of range (n = {n})")
    mask[a.astype(np.int64)] = 1
    return mask


class CsrReport:
    """What sapca_check_csr_device_* / sapca_canonicalize_csr_device_* found in a device CSR (sapca_csr_report): the counts
    and first rows as attributes (a first_*_row is None where its count is zero), `flags` as the tuple of the names of the
    bits that are set (BAD_OFFSETS, COL_RANGE, UNSORTED, DUPLICATES, NONFINITE), `bits` as the number, and `canonical`:
    none of the first four is set."""

    _FIRSTS = ("first_bad_offset_row", "first_out_of_range_row", "first_unsorted_row", "first_duplicate_row", "first_nonfinite_row")
    _COUNTS = ("cols_out_of_range", "unsorted_rows", "duplicate_entries", "nonfinite_values", "stored_zeros")

    def __init__(self, raw):
        self.bits = int(raw.flags)
        self.flags = tuple(name for bit, name in sorted(L.CSR_FLAG_NAMES.items()) if self.bits & bit)
        self.canonical = (self.bits & 15) == 0
        for f in self._COUNTS:
            setattr(self, f, int(getattr(raw, f)))
        for f in self._FIRSTS:
            v = int(getattr(raw, f))
            setattr(self, f, None if v == 2 ** 64 - 1 else v)

    def __repr__(self):
        body = ", ".join(f"{f}={getattr(self, f)}" for f in self._COUNTS + self._FIRSTS if getattr(self, f) not in (0, None))
        return f"CsrReport(flags={'|'.join(self.flags) or '0'}{', ' + body if body else ''})"


def _new_report():
    r = L.CsrReport()
    r.struct_size = C.sizeof(L.CsrReport)
    return r


class RankGroupsResult:
    """What ResidentCsr.rank_groups returns, every array K x n (group x column): `scores` and `pvals` (arrays, or with method
    "both" dicts keyed "wilcoxon" / "t-test"), `means`, `vars`, `pct_nonzero` (stored non-zero entries / rows of the group, 0
    for an empty group), `group_rows` (K) and `names`: per group the column indices by descending score, ties to the lower
    index, cut to n_top (with "both": by the Wilcoxon score)."""

    def __init__(self, method, scores, pvals, means, vars_, nonzero, group_rows, n_top):
        self.method, self.scores, self.pvals, self.means, self.vars = method, scores, pvals, means, vars_
        self.nonzero, self.group_rows = nonzero, group_rows
        rows = group_rows.astype(np.float64)[:, None]
        self.pct_nonzero = np.divide(nonzero.astype(np.float64), rows, out=np.zeros(nonzero.shape), where=rows > 0)
        by = scores["wilcoxon"] if isinstance(scores, dict) else scores
        order = np.argsort(-by, axis=1, kind="stable")   # (stable: equal scores keep ascending column order)
        self.names = order if n_top is None else order[:, :int(n_top)]

    def logfoldchanges(self, base=2):
        """scanpy's convention on log1p data: log_base((expm1(mean_group) + 1e-9) / (expm1(mean_rest) + 1e-9)), the rest's
        mean from the groups' means and sizes (host arithmetic; nan where a side has no rows)."""
        rows = self.group_rows.astype(np.float64)[:, None]
        total = (self.means * rows).sum(axis=0, keepdims=True)
        rest = rows.sum() - rows
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_rest = (total - self.means * rows) / rest
            mean_group = np.where(rows > 0, self.means, np.nan)
            return np.log((np.expm1(mean_group) + 1e-9) / (np.expm1(mean_rest) + 1e-9)) / np.log(float(base))


class HvgResult:
    """What ResidentCsr.highly_variable returns, every array of length n (one per column): `means`, `variances`,
    `variances_norm` (seurat_v3), `dispersions`, `dispersions_norm` (seurat), `rank` (f64, NaN where the column is not
    ranked), `n_batches_hv` (u32) and `highly_variable` (bool, the library's u8 bytes viewed: the mask of a masked estimator
    and select(cols=...) take it as it is)."""

    def __init__(self, flavor, arrays):
        self.flavor = flavor
        for k, v in arrays.items():
            setattr(self, k, v)

    @property
    def n_selected(self):
        return int(self.highly_variable.sum())


class ResidentCsr:
    """A CSR matrix uploaded once into buffers owned by a Session (sapca_upload_csr_*): normalize -> log1p ->
    statistics -> PCA on it without crossing PCIe again.  `as_device_csr()` gives the
    sapca.DeviceCsr the estimators take (zero-copy torch views of the same memory)."""

    def __init__(self, session, shape, nnz, dtype, d_ptr, d_idx, d_val):
        self._s, self.shape, self.nnz, self.dtype = session, tuple(shape), int(nnz), np.dtype(dtype)
        self.d_ptr, self.d_idx, self.d_val = int(d_ptr), int(d_idx), int(d_val)

    def _args(self):
        m, n = self.shape
        return [self._s._h, C.c_uint64(m), C.c_uint64(n), C.c_uint64(self.nnz), C.c_void_p(self.d_ptr), C.c_void_p(self.d_idx),
                C.c_void_p(self.d_val)]

    def normalize(self, sums, target, direction):
        """Normalize<T>::normalize(&sums, target, &direction), csr.rs:1012-1066 (in place)"""
        suf, _ = _SUF[self.dtype]
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        L.check(self._s._h, getattr(L.load(), f"sapca_normalize_csr_device_{suf}")(
            *self._args(), _p(sums, C.c_double), C.c_uint64(sums.size), C.c_double(float(target)), C.c_int32(int(direction))))
        return self

    def log1p(self):
        """Log1P::log1p_normalize, csr.rs:1069-1078 (in place)"""
        suf, _ = _SUF[self.dtype]
        L.check(self._s._h, getattr(L.load(), f"sapca_log1p_csr_device_{suf}")(self._s._h, C.c_uint64(self.nnz), C.c_void_p(self.d_val)))
        return self

    def values_changed(self):
        """the caller edited the device values itself: drop the statistics gathered at upload (sapca_upload_values_changed)"""
        L.check(self._s._h, L.load().sapca_upload_values_changed(self._s._h))
        return self

    def stats(self, direction):
        """(sum, sum_squared, nonzero, min, max) per row (ROW) or column (COLUMN): sum_row/col, sum_row/col_squared,
        nonzero_row/col, min_max_row/col of the reference (csr.rs:23-134, 259-392, 558-630, 917-1008).  min / max compare
        as the reference does: a NaN never wins; ROW starts from the row's first stored value (a row that begins with a
        NaN is (NaN, NaN), a row of +inf alone has min +inf), COLUMN from (T::MAX, -T::MAX) (NaNs are ignored, a column
        of +inf alone keeps min T::MAX).  Lines without entries keep (T::MAX, -T::MAX)."""
        suf, ct = _SUF[self.dtype]
        m, n = self.shape
        ln = n if int(direction) == COLUMN else m
        sm, sq = np.zeros(ln), np.zeros(ln)
        nz = np.zeros(ln, dtype=np.uint64)
        lo, hi = np.zeros(ln, dtype=self.dtype), np.zeros(ln, dtype=self.dtype)
        L.check(self._s._h, getattr(L.load(), f"sapca_stats_csr_device_{suf}")(
            *self._args(), C.c_int32(int(direction)), _p(sm, C.c_double), _p(sq, C.c_double), _p(nz, C.c_uint64), _p(lo, ct), _p(hi, ct)))
        return sm, sq, nz, lo, hi

    def variance(self, direction):
        """var_row / var_col (csr.rs:632-726): host arithmetic on the sums"""
        sm, sq, _, _, _ = self.stats(direction)
        N = float(self.shape[0] if int(direction) == COLUMN else self.shape[1])
        if N <= 1:
            return np.zeros_like(sm)
        mean = sm / N
        return (sq / N - mean ** 2) * (N / (N - 1.0))

    def batch_stats(self, grouped_axis, codes, n_batches, want=("mean", "var", "count")):
        """sapca_batch_stats_csr_device_*: dense codes in [0, n_batches) label the rows (grouped_axis 0) or the columns
        (1); returns {name: array of n_batches x (n or m)} for the names in `want` (mean, var: f64; count: u64)"""
        suf, _ = _SUF[self.dtype]
        m, n = self.shape
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        ln = n if int(grouped_axis) == 0 else m
        out = {k: np.zeros((int(n_batches), ln), dtype=np.uint64 if k == "count" else np.float64) for k in want}
        ptrs = [_p(out[k], C.c_uint64 if k == "count" else C.c_double) if k in out else None for k in ("mean", "var", "count")]
        L.check(self._s._h, getattr(L.load(), f"sapca_batch_stats_csr_device_{suf}")(
            *self._args(), C.c_int32(int(grouped_axis)), _p(codes, C.c_int32), C.c_uint64(codes.size), C.c_uint32(int(n_batches)), *ptrs))
        return out

    def _grouped(self, batches, grouped_axis, what, message):
        want = self.shape[0] if grouped_axis == 0 else self.shape[1]
        if len(batches) != want:
            raise ValueError(message.format(len(batches), want))
        labels, codes = _dense_codes(batches)
        res = self.batch_stats(grouped_axis, codes, len(labels), want=(what,))[what]
        return {b: res[c] for c, b in enumerate(labels)}

    def var_batch_row(self, batches):
        """BatchMatrixVariance::var_batch_row (csr.rs:1088-1163): batches label the rows; {label: per-column variance of the
        stored entries in that label's rows} (count - 1 denominator, 0 for fewer than two entries)"""
        return self._grouped(batches, 0, "var", "Batch vector length ({}) doesn't match matrix row count ({})")

    def var_batch_col(self, batches):
        """BatchMatrixVariance::var_batch_col (csr.rs:1165-1244): batches label the columns; {label: per-row variance}"""
        return self._grouped(batches, 1, "var", "Batch vector length ({}) doesn't match matrix column count ({})")

    def mean_batch_row(self, batches):
        """BatchMatrixMean::mean_batch_row (csr.rs:1251-1296): batches label the columns; {label: per-row sum / number of
        columns with that label}"""
        return self._grouped(batches, 1, "mean", "Number of batch identifiers ({}) must match number of columns ({})")

    def mean_batch_col(self, batches):
        """BatchMatrixMean::mean_batch_col (csr.rs:1299-1343): batches label the rows; {label: per-column sum / number of
        rows with that label}"""
        return self._grouped(batches, 0, "mean", "Number of batch identifiers ({}) must match number of rows ({})")

    # ---- rank groups (sapca_rank_sums_csr_device_* / sapca_rank_groups_csr_device_*): marker columns of labelled rows ----
    def _rank_labels(self, labels, n_groups):
        """(device int32 labels, K): `labels` a numpy array (copied up), a torch device tensor or an estimator with device
        labels_ (KMeans, Louvain), used in place; n_groups None: 1 + the largest label."""
        import torch
        m = self.shape[0]

        def check_groups(k):
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
                raise ValueError(f"n_groups must be an integer, got {k!r}")
            if not 1 <= int(k) <= L.RANK_MAX_GROUPS:
                raise ValueError(f"n_groups = {int(k)} is outside 1 .. {L.RANK_MAX_GROUPS}")
            return int(k)

        if n_groups is not None:
            n_groups = check_groups(n_groups)
        labels = getattr(labels, "labels_", labels)
        if labels is None:
            raise ValueError("labels: the estimator has not been fitted")
        if isinstance(labels, np.ndarray) or not isinstance(labels, torch.Tensor):
            a = np.asarray(labels)
            if a.ndim != 1 or a.size != m or a.dtype.kind not in "iu":
                raise ValueError(f"labels must be {m} integers, got shape {a.shape} of dtype {a.dtype}")
            if a.size and (a.max() > 2 ** 31 - 1 or a.min() < -2 ** 31):
                raise ValueError("labels must fit int32")
            labels = torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=self._s._device())
        if not (labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == (m,) and labels.is_contiguous()):
            raise ValueError(f"labels must be {m} contiguous int32 values (a device tensor or a numpy array)")
        if n_groups is None:
            n_groups = check_groups(max(int(labels.max().item()) + 1, 1) if m else 1)
        return labels, n_groups

    def rank_sums(self, labels, n_groups=None):
        """sapca_rank_sums_csr_device_*: the exact quantities of the rank pass, every group of rows against the rest, per
        column: {"group_rows": K u64, "rank_sum2": K x n i64 (twice the rank sums), "nonzero": K x n u64, "tie_sum": n f64}.
        Rows whose label is outside [0, n_groups) are excluded."""
        import torch
        labels, K = self._rank_labels(labels, n_groups)
        suf, _ = _SUF[self.dtype]
        m, n = self.shape
        out = {"group_rows": np.zeros(K, dtype=np.uint64), "rank_sum2": np.zeros((K, n), dtype=np.int64),
               "nonzero": np.zeros((K, n), dtype=np.uint64), "tie_sum": np.zeros(n)}
        torch.cuda.current_stream().synchronize()
        L.check(self._s._h, getattr(L.load(), f"sapca_rank_sums_csr_device_{suf}")(
            *self._args(), C.c_void_p(labels.data_ptr() if m else None), C.c_uint32(K), _p(out["group_rows"], C.c_uint64),
            _p(out["rank_sum2"], C.c_int64), _p(out["nonzero"], C.c_uint64), _p(out["tie_sum"], C.c_double)))
        return out

    def rank_groups(self, labels, n_groups=None, method="wilcoxon", tie_correct=False, n_top=None):
        """sapca_rank_groups_csr_device_*: scanpy's rank_genes_groups of every group against the rest, method "wilcoxon"
        (scores: z, pvals: erfc(|z| / sqrt 2)), "t-test" (scores: Welch's t, pvals through scipy.stats.t.sf where scipy
        imports, else None) or "both" (scores / pvals become {"wilcoxon": .., "t-test": ..}).  Returns a RankGroupsResult."""
        import torch
        if method not in ("wilcoxon", "t-test", "both"):
            raise ValueError(f'method must be "wilcoxon", "t-test" or "both", got {method!r}')
        if n_top is not None and (isinstance(n_top, bool) or not isinstance(n_top, (int, np.integer)) or n_top < 0):
            raise ValueError(f"n_top must be a non-negative integer or None, got {n_top!r}")
        labels, K = self._rank_labels(labels, n_groups)
        suf, _ = _SUF[self.dtype]
        m, n = self.shape
        wil, tt = method != "t-test", method != "wilcoxon"
        a = {k: np.zeros((K, n)) for k in ("mean", "var") + (("t", "df") if tt else ()) + (("z", "pz") if wil else ())}
        rows, nz = np.zeros(K, dtype=np.uint64), np.zeros((K, n), dtype=np.uint64)
        f = lambda k: _p(a[k], C.c_double) if k in a else None   # noqa: E731
        torch.cuda.current_stream().synchronize()
        L.check(self._s._h, getattr(L.load(), f"sapca_rank_groups_csr_device_{suf}")(
            *self._args(), C.c_void_p(labels.data_ptr() if m else None), C.c_uint32(K), C.c_int32(1 if tie_correct else 0),
            _p(rows, C.c_uint64), f("mean"), f("var"), _p(nz, C.c_uint64), f("t"), f("df"), f("z"), f("pz")))
        scores, pvals = {}, {}
        if wil:
            scores["wilcoxon"], pvals["wilcoxon"] = a["z"], a["pz"]
        if tt:
            scores["t-test"] = a["t"]
            try:
                from scipy import stats
                with np.errstate(invalid="ignore"):
                    pt = 2.0 * stats.t.sf(np.abs(a["t"]), np.where(a["df"] > 0, a["df"], 1.0))
                pvals["t-test"] = np.where(a["df"] > 0, pt, 1.0)
            except ImportError:
                pvals["t-test"] = None
        if method != "both":
            scores, pvals = scores[method], pvals[method]
        return RankGroupsResult(method, scores, pvals, a["mean"], a["var"], nz, rows, n_top)

    # ---- variable genes (sapca_hvg_moments_csr_device_* / sapca_hvg_csr_device_*): feature selection between log1p and the fit ----
    def hvg_moments(self, transform, clip=None, batch=None, code=0):
        """sapca_hvg_moments_csr_device_*: per column, the sum and the sum of squares (f64) of the transformed stored entries
        of the included rows, and how many were clipped: {"sum", "sum_squared", "n_clipped"}.  transform "clip"
        (min(x, clip[j]); clip: n f64) or "expm1"; batch: labels per row (numpy or device int32) of which the rows with
        label == code are included, None: every row."""
        import torch
        if transform not in L.HVG_TRANSFORMS and not isinstance(transform, (int, np.integer)):
            raise ValueError(f'transform must be "clip" or "expm1", got {transform!r}')
        tr = L.HVG_TRANSFORMS.get(transform, transform)
        m, n = self.shape
        labels = None
        if batch is not None:
            labels, _ = self._rank_labels(batch, 1)
        if clip is not None:
            clip = np.ascontiguousarray(clip, dtype=np.float64)
            if clip.shape != (n,):
                raise ValueError(f"clip must hold {n} values, got shape {clip.shape}")
        suf, _ = _SUF[self.dtype]
        out = {"sum": np.zeros(n), "sum_squared": np.zeros(n), "n_clipped": np.zeros(n, dtype=np.uint64)}
        torch.cuda.current_stream().synchronize()
        L.check(self._s._h, getattr(L.load(), f"sapca_hvg_moments_csr_device_{suf}")(
            *self._args(), C.c_void_p(labels.data_ptr() if labels is not None and m else None), C.c_int32(int(code)),
            C.c_int32(int(tr)), _p(clip, C.c_double) if clip is not None else None, _p(out["sum"], C.c_double),
            _p(out["sum_squared"], C.c_double), _p(out["n_clipped"], C.c_uint64)))
        return out

    def highly_variable(self, n_top=2000, flavor="seurat_v3", batch=None, n_batches=None, span=0.3, n_bins=20, min_mean=0.0125,
                        max_mean=3.0, min_disp=0.5, max_disp=float("inf")):
        """sapca_hvg_csr_device_*: scanpy's pp.highly_variable_genes, flavor "seurat_v3" (on counts) or "seurat" (on log1p
        data; n_top None or 0: the four cutoffs).  batch: labels per row (numpy or device int32; a label outside
        [0, n_batches) excludes its row), None: one batch of all rows.  The loess of seurat_v3 is the direct surface, not
        skmisc's interpolated one (include/sapca.h).  Returns an HvgResult."""
        import torch
        if flavor not in L.HVG_FLAVORS and not isinstance(flavor, (int, np.integer)):
            raise ValueError(f'flavor must be "seurat_v3" or "seurat", got {flavor!r}')
        m, n = self.shape
        labels, K = None, 1
        if batch is not None:
            labels, K = self._rank_labels(batch, n_batches)
        elif n_batches is not None:
            K = int(n_batches)
        o = L.default_hvg_options()
        o.flavor = int(L.HVG_FLAVORS.get(flavor, flavor))
        o.n_top = int(n_top or 0)
        o.span, o.n_bins = float(span), int(n_bins)
        o.min_mean, o.max_mean, o.min_disp, o.max_disp = float(min_mean), float(max_mean), float(min_disp), float(max_disp)
        a = {k: np.zeros(n) for k in ("means", "variances", "variances_norm", "dispersions", "dispersions_norm", "rank")}
        a["n_batches_hv"] = np.zeros(n, dtype=np.uint32)
        a["highly_variable"] = np.zeros(n, dtype=np.uint8)
        suf, _ = _SUF[self.dtype]
        torch.cuda.current_stream().synchronize()
        L.check(self._s._h, getattr(L.load(), f"sapca_hvg_csr_device_{suf}")(
            *self._args(), C.c_void_p(labels.data_ptr() if labels is not None and m else None), C.c_uint32(K), C.byref(o),
            _p(a["means"], C.c_double), _p(a["variances"], C.c_double), _p(a["variances_norm"], C.c_double),
            _p(a["dispersions"], C.c_double), _p(a["dispersions_norm"], C.c_double), _p(a["rank"], C.c_double),
            _p(a["n_batches_hv"], C.c_uint32), _p(a["highly_variable"], C.c_uint8)))
        a["highly_variable"] = a["highly_variable"].view(np.bool_)   # (0 / 1 bytes)
        return HvgResult(flavor, a)

    def sum_row_n_top(self, n):
        """MatrixNTop::sum_row_n_top (csr.rs:1347-1376): per row, the sum of the n largest stored values (all of them when
        the row has fewer).  n an int -> m values; a sequence of ints -> len(n) x m, one pass over the rows for all."""
        single = np.ndim(n) == 0
        ns = np.atleast_1d(np.asarray(n))
        if ns.size == 0 or not np.issubdtype(ns.dtype, np.integer) or (ns < 0).any():
            raise ValueError("n must be a non-negative integer or a non-empty sequence of them")
        ns = np.ascontiguousarray(ns, dtype=np.uint64)
        suf, _ = _SUF[self.dtype]
        out = np.zeros((ns.size, self.shape[0]))
        L.check(self._s._h, getattr(L.load(), f"sapca_sum_row_n_top_csr_device_{suf}")(
            *self._args(), _p(ns, C.c_uint64), C.c_uint32(ns.size), _p(out, C.c_double)))
        return out[0] if single else out

    # ---- masked and chunk statistics (MatrixNonZero / MatrixSum / MatrixVariance *_masked, *_chunk; MatrixMinMax *_chunk) ----
    def masked_stats(self, direction, mask=None):
        """sapca_masked_stats_csr_device_*: (sum, sum_squared, count, var) per row (ROW; `mask` over the columns) or per
        column (COLUMN; `mask` over the rows), over the kept stored entries; mask None keeps everything.  var is the
        stored-entry variance (no correction, 0 where count is 0).  f64 sums; count u64."""
        suf, _ = _SUF[self.dtype]
        m, n = self.shape
        ln = n if int(direction) == COLUMN else m
        out = [np.zeros(ln), np.zeros(ln), np.zeros(ln, dtype=np.uint64), np.zeros(ln)]
        if mask is None:
            mp, ml = None, 0
        else:
            mk = np.ascontiguousarray(np.asarray(mask, dtype=bool).reshape(-1), dtype=np.uint8)
            mp, ml = _p(mk, C.c_uint8), mk.size
        L.check(self._s._h, getattr(L.load(), f"sapca_masked_stats_csr_device_{suf}")(
            *self._args(), C.c_int32(int(direction)), mp, C.c_uint64(ml), _p(out[0], C.c_double), _p(out[1], C.c_double),
            _p(out[2], C.c_uint64), _p(out[3], C.c_double)))
        return tuple(out)

    def _masked(self, direction, mask, what):
        want = self.shape[0] if int(direction) == COLUMN else self.shape[1]
        if len(mask) < want:   # the reference's message (its Err), before any library call
            raise ValueError(f"Mask length ({len(mask)}) is less than number of {'rows' if direction == COLUMN else 'columns'} ({want})")
        return self.masked_stats(direction, mask)[what]

    def nonzero_col_masked(self, mask):
        """MatrixNonZero::nonzero_col_masked (csr.rs:153-186): per column, the stored entries of the rows with mask[row]"""
        return self._masked(COLUMN, mask, 2)

    def nonzero_row_masked(self, mask):
        """MatrixNonZero::nonzero_row_masked (csr.rs:188-252): per row, the stored entries of the columns with mask[col]"""
        return self._masked(ROW, mask, 2)

    def sum_col_masked(self, mask):
        """MatrixSum::sum_col_masked (csr.rs:418-488): per column, the sum over the rows with mask[row] (exact, correctly
        rounded f64 sums)"""
        return self._masked(COLUMN, mask, 0)

    def sum_row_masked(self, mask):
        """MatrixSum::sum_row_masked (csr.rs:490-556): per row, the sum over the columns with mask[col] (f64)"""
        return self._masked(ROW, mask, 0)

    def var_col_masked(self, mask):
        """MatrixVariance::var_col_masked (csr.rs:815-862): per column, sumsq / count - mean^2 over the kept stored entries"""
        return self._masked(COLUMN, mask, 3)

    def var_row_masked(self, mask):
        """MatrixVariance::var_row_masked (csr.rs:864-914): per row, sum (x - mean)^2 / count over the kept stored entries"""
        return self._masked(ROW, mask, 3)

    # The chunk family updates the caller's numpy array in place and returns it.  Where the reference would index out of
    # bounds (a panic), these raise ValueError before touching it.
    def nonzero_col_chunk(self, reference):
        """MatrixNonZero::nonzero_col_chunk (csr.rs:124-134): reference[c] += stored entries of column c, c < len"""
        k = min(len(reference), self.shape[1])
        reference[:k] += self.stats(COLUMN)[2][:k].astype(reference.dtype)
        return reference

    def nonzero_row_chunk(self, reference):
        """MatrixNonZero::nonzero_row_chunk (csr.rs:136-150): reference[r] += stored entries of row r, r < len"""
        k = min(len(reference), self.shape[0])
        reference[:k] += self.stats(ROW)[2][:k].astype(reference.dtype)
        return reference

    def sum_col_chunk(self, reference):
        """MatrixSum::sum_col_chunk (csr.rs:394-405): reference[c] += sum of column c, c < len (the column's f64 sum is
        added once; the reference adds entry by entry in T)"""
        k = min(len(reference), self.shape[1])
        reference[:k] += self.stats(COLUMN)[0][:k].astype(reference.dtype)
        return reference

    def sum_row_chunk(self, reference):
        """MatrixSum::sum_row_chunk (csr.rs:407-416): reference[r] = sum of row r, overwritten; len must be >= m"""
        m = self.shape[0]
        if len(reference) < m:
            raise ValueError(f"sum_row_chunk: reference length {len(reference)} is less than number of rows {m}")
        reference[:m] = self.stats(ROW)[0]
        return reference

    def var_col_chunk(self, reference):
        """MatrixVariance::var_col_chunk (csr.rs:728-771): reference = per-column stored-entry variance (sumsq / count -
        mean^2); len must be n"""
        n = self.shape[1]
        if len(reference) != n:
            raise ValueError(f"Reference slice length {len(reference)} does not match number of columns {n}")
        reference[:] = self.masked_stats(COLUMN)[3]
        return reference

    def var_row_chunk(self, reference):
        """MatrixVariance::var_row_chunk (csr.rs:773-813): reference = per-row stored-entry variance (two passes); len
        must be m"""
        m = self.shape[0]
        if len(reference) != m:
            raise ValueError(f"Reference slice length {len(reference)} does not match number of rows {m}")
        reference[:] = self.masked_stats(ROW)[3]
        return reference

    def min_max_col_chunk(self, reference):
        """MatrixMinMax::min_max_col_chunk (csr.rs:939-973): reference = (mins, maxs); each column's stored values narrow
        mins[c] / maxs[c] (a nan in the arrays stays, nan values never win: a column of NaNs alone changes nothing).
        The column's own min / max come from stats(COLUMN), which start at (T::MAX, -T::MAX): a column holding only
        +inf lowers a mins[c] above T::MAX to T::MAX (the reference leaves it), and the mirror for -inf.  Every column
        with a stored entry must lie inside both arrays."""
        mins, maxs = reference
        _, _, nz, lo, hi = self.stats(COLUMN)
        has = np.flatnonzero(nz)
        if has.size and has[-1] >= min(len(mins), len(maxs)):
            raise ValueError(f"min_max_col_chunk: column {int(has[-1])} has stored entries but the reference arrays are "
                             f"{len(mins)} / {len(maxs)} long")
        lo, hi = lo[has], hi[has]
        mins[has] = np.where(lo < mins[has], lo, mins[has])
        maxs[has] = np.where(hi > maxs[has], hi, maxs[has])
        return reference

    def min_max_row_chunk(self, reference):
        """MatrixMinMax::min_max_row_chunk (csr.rs:975-1008): reference = (mins, maxs); rows with stored entries overwrite
        mins[r] / maxs[r] with their own min / max, the others are left alone.  The reference starts a row from its
        first stored value: a row that begins with a NaN writes (NaN, NaN), a NaN later in a row is ignored, a row of
        +inf alone writes min +inf (of -inf alone, max -inf).  Every row with a stored entry must lie inside both arrays."""
        mins, maxs = reference
        _, _, nz, lo, hi = self.stats(ROW)
        has = np.flatnonzero(nz)
        if has.size and has[-1] >= min(len(mins), len(maxs)):
            raise ValueError(f"min_max_row_chunk: row {int(has[-1])} has stored entries but the reference arrays are "
                             f"{len(mins)} / {len(maxs)} long")
        mins[has] = lo[has]
        maxs[has] = hi[has]
        return reference

    def select_rows(self, rows):
        """sapca_select_rows_csr_device_*: the rows `rows` of this matrix -- a boolean mask of length m, or integer indices
        in any order, repeats allowed -- as a ResidentCsr of shape (len(rows), n) in the same Session, without crossing
        PCIe.  This matrix stays resident and unchanged beside it; every method here works on the result (normalize and
        log1p included: its values are its own).  It lives in the Session's selection buffers: valid until the next
        select_rows on the Session, and not itself a source of one."""
        suf, _ = _SUF[self.dtype]
        r = _row_list(rows, self.shape[0])
        nnz_out = C.c_uint64()
        dp, di, dv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(self._s._h, getattr(L.load(), f"sapca_select_rows_csr_device_{suf}")(
            *self._args(), _p(r, C.c_uint64) if r.size else None, C.c_uint64(r.size), C.byref(nnz_out), C.byref(dp), C.byref(di),
            C.byref(dv)))
        return ResidentCsr(self._s, (r.size, self.shape[1]), nnz_out.value, self.dtype, dp.value or 0, di.value or 0, dv.value or 0)

    def select(self, rows=None, cols=None, drop_stored_zeros=False):
        """sapca_select_submatrix_csr_device_*: self[rows][:, cols] as a ResidentCsr in the same Session, in one call and
        without crossing PCIe.  rows: as in select_rows (None: every row in order).  cols: a boolean mask of length n or
        strictly ascending integer indices (None: every column); a kept column is renumbered by its rank among the kept
        ones, as MaskedCSRMatrix::new does, so the result is an ordinary (m', n') matrix for every method here and every
        fit -- the column compaction a masked fit repeats in each preparation is paid once.  drop_stored_zeros: entries
        whose value == 0 are dropped too (check().stored_zeros of the result is 0; a NaN stays).  Values move bit for
        bit.  The result shares the Session's selection buffers with select_rows: either call replaces it."""
        suf, _ = _SUF[self.dtype]
        m, n = self.shape
        if rows is None:
            rp, nr = None, m
        else:
            r = _row_list(rows, m)
            rp, nr = (_p(r, C.c_uint64) if r.size else None), r.size   # (no rows: NULL with n_rows = 0 says the same)
        if cols is None:
            mp, ml = None, 0
        else:
            mk = _col_mask(cols, n)
            mp, ml = (_p(mk, C.c_uint8) if mk.size else None), mk.size
        ncols, nnz_out = C.c_uint64(), C.c_uint64()
        dp, di, dv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(self._s._h, getattr(L.load(), f"sapca_select_submatrix_csr_device_{suf}")(
            *self._args(), rp, C.c_uint64(nr), mp, C.c_uint64(ml), C.c_uint32(L.SELECT_DROP_STORED_ZEROS if drop_stored_zeros else 0),
            C.byref(ncols), C.byref(nnz_out), C.byref(dp), C.byref(di), C.byref(dv)))
        return ResidentCsr(self._s, (nr, ncols.value), nnz_out.value, self.dtype, dp.value or 0, di.value or 0, dv.value or 0)

    def select_cols(self, cols):
        """select(cols=cols): every row, the columns `cols`"""
        return self.select(cols=cols)

    @classmethod
    def from_torch(cls, session, row_offsets, col_indices, values, shape):
        """Adopt a caller's own device arrays -- three contiguous CUDA tensors: int64 offsets (m + 1), int32 column indices
        and f32 / f64 values of equal length -- as a ResidentCsr of `session`, without copying.  The object keeps
        references to the tensors.  Nothing is validated here: check() / canonicalize() are the gate, before anything else.
        Stream order: the Session works on its own stream (or the one it was given), not on torch's.  Tensors that torch
        kernels have just written on another stream must be complete first -- torch.cuda.current_stream().synchronize(),
        or build the Session on torch's current stream -- or check() / canonicalize() race with their producer."""
        import torch
        m, n = (int(x) for x in shape)
        want = {"row_offsets": (row_offsets, torch.int64), "col_indices": (col_indices, torch.int32)}
        for name, (t, dt) in want.items():
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.dim() == 1 and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous one-dimensional CUDA tensor of {dt}")
        if not (isinstance(values, torch.Tensor) and values.is_cuda and values.dtype in (torch.float32, torch.float64)
                and values.dim() == 1 and values.is_contiguous()):
            raise ValueError("values must be a contiguous one-dimensional CUDA tensor of float32 or float64")
        if row_offsets.numel() != m + 1 or col_indices.numel() != values.numel():
            raise ValueError(f"shape {(m, n)} wants {m + 1} row offsets and as many column indices as values, got "
                             f"{row_offsets.numel()}, {col_indices.numel()} and {values.numel()}")
        dt = np.float32 if values.dtype == torch.float32 else np.float64
        out = cls(session, (m, n), values.numel(), dt, row_offsets.data_ptr(), col_indices.data_ptr(), values.data_ptr())
        out._keep = (row_offsets, col_indices, values)
        return out

    def check(self):
        """sapca_check_csr_device_*: a CsrReport of these arrays (read-only, one pass on the GPU).  `.canonical` says
        whether every entry point may take them as they are."""
        suf, _ = _SUF[self.dtype]
        rep = _new_report()
        L.check(self._s._h, getattr(L.load(), f"sapca_check_csr_device_{suf}")(*self._args(), C.byref(rep)))
        return CsrReport(rep)

    def canonicalize(self):
        """sapca_canonicalize_csr_device_*: (matrix, report) -- the same matrix with every row's columns ascending and equal
        columns summed (left to right in stored order), and the CsrReport of THIS matrix (duplicate_entries exact).  The
        matrix is `self` when nothing had to be done; otherwise it lives in the Session's canonical buffers, beside this
        one, until the next canonicalize on the Session.  Broken offsets or a column out of range raise SapcaError."""
        suf, _ = _SUF[self.dtype]
        rep = _new_report()
        nnz_out = C.c_uint64()
        dp, di, dv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(self._s._h, getattr(L.load(), f"sapca_canonicalize_csr_device_{suf}")(
            *self._args(), C.byref(nnz_out), C.byref(dp), C.byref(di), C.byref(dv), C.byref(rep)))
        got = (dp.value or 0, di.value or 0, dv.value or 0)
        if got == (self.d_ptr, self.d_idx, self.d_val):
            return self, CsrReport(rep)
        return ResidentCsr(self._s, self.shape, nnz_out.value, self.dtype, *got), CsrReport(rep)

    def values(self):
        """the current (device) values, copied to the host"""
        return self.as_device_csr().values.cpu().numpy()

    def as_device_csr(self):
        import torch
        from .dist import _DevView  # noqa: F401  (same zero-copy view helper)
        from .pca import DeviceCsr

        class _View:
            def __init__(self, ptr, count, typestr):
                self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2}
        m, n = self.shape
        ptr = torch.as_tensor(_View(self.d_ptr, m + 1, "<i8"), device="cuda")
        idx = torch.as_tensor(_View(self.d_idx, max(self.nnz, 1), "<i4"), device="cuda")[: self.nnz]
        val = torch.as_tensor(_View(self.d_val, max(self.nnz, 1), "<f4" if self.dtype == np.float32 else "<f8"), device="cuda")[: self.nnz]
        return DeviceCsr(ptr, idx, val, (m, n))


def _upload(self, indptr, indices, data, m, n):
    """sapca_upload_csr_*: host CSR -> ResidentCsr in this session's buffers"""
    suf, ct, keep, args = self._csr_args(indptr, indices, data, m, n)
    dp, di, dv = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.check(self._h, getattr(L.load(), f"sapca_upload_csr_{suf}")(*args, C.byref(dp), C.byref(di), C.byref(dv)))
    return ResidentCsr(self, (m, n), keep[2].size, keep[2].dtype, dp.value or 0, di.value or 0, dv.value or 0)


Session.upload = _upload


def covariate_basis(Z, center=True):
    """sapca_covariate_basis (host-only code path of the library): (Q, W, rank) for the design D = [1 | Z] (center) or Z.
    Q: rows x rank, orthonormal columns spanning D's; W: (cols + center) x rank with Q = D W (zero rows for the design
    columns the pivoted QR found dependent).  Rank 0 gives empty Q and W."""
    z = np.ascontiguousarray(np.asarray(Z, dtype=np.float64))
    if z.ndim == 1:
        z = np.ascontiguousarray(z[:, None])
    rows, cols = z.shape
    design = cols + int(bool(center))
    q = np.zeros((rows, L.MAX_DESIGN_COLUMNS))
    w = np.zeros((design, L.MAX_DESIGN_COLUMNS))
    rank = C.c_uint64()
    st = L.load().sapca_covariate_basis(_p(z, C.c_double) if z.size else None, C.c_uint64(rows), C.c_uint64(cols), C.c_int32(int(bool(center))),
                                        _p(q, C.c_double), _p(w, C.c_double), C.byref(rank))
    if st != L.OK:
        raise L.SapcaError(st, "sapca_covariate_basis refused the design (more than 16 design columns, or a non-finite value)")
    r = int(rank.value)
    return q[:, :r].copy(), w[:, :r].copy(), r


def partition_rows(indptr, nparts):
    """nnz-balanced contiguous row ranges (host-only code path of the library)."""
    ro = as_u64(indptr)
    bounds = np.zeros(nparts + 1, dtype=np.uint64)
    st = L.load().sapca_partition_rows(C.c_uint64(ro.size - 1), _p(ro, C.c_uint64), C.c_uint32(nparts), _p(bounds, C.c_uint64))
    if st != L.OK:
        raise L.SapcaError(st, "sapca_partition_rows failed")
    return bounds

"""Writes tests/golden/g14_spectral.npz: the fixtures of the spectral tests (python tests/golden/make_golden_spectral.py, CPU
only; numpy, scipy and scikit-learn).

Two symmetric k-NN graphs of clustered points with Gaussian weights rounded to float32 (so that the f32 and the f64 entry
points see the same numbers):
  conn   m = 300, connected, about 14 entries per row
  disc   m = 402: three well separated groups (3 components) and 2 isolated vertices (empty rows) -- 5 components
Per fixture `name`: {name}_indptr (int64) / _indices (int32) / _data (float32), {name}_labels, {name}_n_components, and per
kind in (normalized, diffmap) what tests/spectral_ref.py returns for n_eigen = 16: {name}_{kind}_evals, _evecs, _gaps,
_n_locked.  The seeds are searched so that every gap among the compared eigenvalues is at least MIN_GAP."""
import os
import sys

import numpy as np
import scipy.sparse as sp
from sklearn.neighbors import NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import spectral_ref as SR     # noqa: E402

N_EIGEN = 16
MIN_GAP = 5e-4
KINDS = (SR.NORMALIZED, SR.DIFFMAP)


def knn_graph(X, k):
    """max(A, A^T) of the k nearest neighbours with weights exp(-d^2 / mean d_k^2), float32-exact, canonical CSR"""
    m = X.shape[0]
    dist, idx = NearestNeighbors(n_neighbors=k + 1).fit(X).kneighbors(X)
    dist, idx = dist[:, 1:], idx[:, 1:]
    sigma2 = float(np.mean(dist[:, -1] ** 2))
    w = np.exp(-dist ** 2 / sigma2)
    A = sp.csr_matrix((w.ravel(), (np.repeat(np.arange(m), k), idx.ravel())), shape=(m, m))
    A = A.maximum(A.T).tocsr()
    A.data = A.data.astype(np.float32).astype(np.float64)
    A = ((A + A.T) * 0.5).tocsr()   # (the rounding is symmetric already; this keeps the structure canonical)
    A.sort_indices()
    return A


def clustered_points(rng, sizes, spread, dim=5):
    centres = rng.normal(size=(len(sizes), dim)) * spread
    return np.concatenate([c + rng.normal(size=(n, dim)) for c, n in zip(centres, sizes)])


def connected_fixture(seed):
    rng = np.random.default_rng(seed)
    X = clustered_points(rng, (80, 70, 60, 50, 40), spread=1.6)
    return knn_graph(rng.permutation(X), 10)


def disconnected_fixture(seed):
    rng = np.random.default_rng(seed)
    X = clustered_points(rng, (150, 130, 120), spread=30.0)
    A = knn_graph(X, 10).tolil()
    m = A.shape[0] + 2
    B = sp.lil_matrix((m, m))
    # the isolated vertices take the numbers 7 and m - 1: every other vertex keeps its order around them
    keep = np.array([i for i in range(m) if i not in (7, m - 1)])
    B[np.ix_(keep, keep)] = A
    B = B.tocsr()
    B.sort_indices()
    return B


def describe(A, want_components):
    ptr, idx, dat = A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data
    labels, ncomp = SR.components(ptr, idx)
    if ncomp != want_components:
        return None
    out = {"labels": labels, "n_components": np.int64(ncomp)}
    for kind in KINDS:
        r = SR.eigenpairs(ptr, idx, dat, kind, N_EIGEN)
        if np.min(r["gaps"]) < MIN_GAP:
            return None
        for key in ("evals", "evecs", "gaps"):
            out[f"{kind}_{key}"] = r[key]
        out[f"{kind}_n_locked"] = np.int64(r["n_locked"])
    return out


def search(make, want_components):
    for seed in range(200):
        A = make(seed)
        d = describe(A, want_components)
        if d is not None:
            return seed, A, d
    raise RuntimeError("no seed gives the wanted components and gaps")


def build(verbose=False):
    out = {}
    for name, make, ncomp in (("conn", connected_fixture, 1), ("disc", disconnected_fixture, 5)):
        seed, A, d = search(make, ncomp)
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_indptr"] = A.indptr.astype(np.int64)
        out[f"{name}_indices"] = A.indices.astype(np.int32)
        out[f"{name}_data"] = A.data.astype(np.float32)
        assert np.array_equal(out[f"{name}_data"].astype(np.float64), A.data)
        for key, v in d.items():
            out[f"{name}_{key}"] = v
        if verbose:
            print(f"{name}: seed {seed}, m = {A.shape[0]}, {A.nnz / A.shape[0]:.1f} entries per row, {ncomp} components, smallest gaps "
                  + ", ".join(f"{k} {np.min(d[f'{k}_gaps']):.2e}" for k in KINDS))
    return out


def main():
    out = build(verbose=True)
    path = os.path.join(HERE, "g14_spectral.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/g9_kmeans.npz: the fixture of the k-means tests (python tests/golden/make_golden_kmeans.py, CPU only;
needs scikit-learn, which the tests themselves do not).

Two blob fixtures (tests/kmeans_ref.blobs, no cluster ever empty): a600 = 600 x 10, k = 5; b900 = 900 x 16, k = 9, each with
init = its first k rows.  For tol = 0 and tol = 1e-4 the outputs of scikit-learn's
KMeans(n_clusters=k, init=array, n_init=1, algorithm="lloyd", max_iter=300, tol=tol): labels_, cluster_centers_, inertia_,
n_iter_, and the version that produced them.  The generator insists that the restatement's smallest assignment margin along
each run is far above f64 rounding, so that the labels and n_iter_ are not a matter of summation order."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import kmeans_ref as KR      # noqa: E402

FIXTURES = {"a600": (600, 10, 5, 1.0, 3), "b900": (900, 16, 9, 1.0, 4)}   # m, d, k, spread, seed
TOLS = {"tol0": 0.0, "tol1e4": 1e-4}


def main():
    import sklearn
    from sklearn.cluster import KMeans
    out = dict(sklearn_version=np.array(sklearn.__version__))
    for name, (m, d, k, spread, seed) in FIXTURES.items():
        X, _ = KR.blobs(m, d, k, spread, seed)
        init = X[:k].copy()
        out[f"{name}_X"], out[f"{name}_init"] = X, init
        for tname, tol in TOLS.items():
            km = KMeans(n_clusters=k, init=init, n_init=1, algorithm="lloyd", max_iter=300, tol=tol).fit(X)
            ref = KR.lloyd(X, init, 300, tol)
            assert ref["min_margin"] > 1e-10, (name, tname, ref["min_margin"])
            assert np.bincount(km.labels_, minlength=k).min() > 0
            print(f"{name} {tname}: n_iter {km.n_iter_} (restatement {ref['n_iter']}), inertia {km.inertia_:.6f}, "
                  f"min margin {ref['min_margin']:.2e}, tol gap {ref['tol_gap']:.2e}")
            out[f"{name}_{tname}_labels"] = km.labels_.astype(np.int32)
            out[f"{name}_{tname}_centers"] = km.cluster_centers_
            out[f"{name}_{tname}_inertia"] = np.float64(km.inertia_)
            out[f"{name}_{tname}_n_iter"] = np.int64(km.n_iter_)
    np.savez_compressed(os.path.join(HERE, "g9_kmeans.npz"), **out)


if __name__ == "__main__":
    main()

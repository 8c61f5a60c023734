"""Writes tests/golden/g8_tsne.npz: the fixture of the t-SNE tests (python tests/golden/make_golden_tsne.py, CPU only; needs
scikit-learn, which the tests themselves do not).

  X (300 x 10, three Gaussian clusters), perplexity 10, the K = 30 exact neighbour lists (tests/knn_ref.py), beta and the
  symmetric P of tests/tsne_ref.py;
  Y0 (1e-4 N(0, 1)) and Y1 (scale ~ 10, where the repulsion matters); at each, scikit-learn's Kullback-Leibler divergence and
  its gradient / 4 (sklearn.manifold._t_sne._kl_divergence, whose `c = 4` the Barnes-Hut form drops), with P and with 12 P;
  Y20: the restatement's embedding after 20 epochs from Y0, and its KL.

The gain rule is discontinuous, so a trajectory can only be compared where no gain decision hangs on rounding: the generator
runs the 20 epochs a second time with every sum over j in the opposite order and insists that all gains agree, trying seeds
from SEED upwards until they do (the seed used is stored)."""
import os
import sys

import numpy as np
import scipy.sparse as sp
from scipy.spatial.distance import squareform

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "single-algebra_amd", "python"))

import knn_ref as KR      # noqa: E402
import tsne_ref as TR     # noqa: E402

SEED, M, DIM, PERPLEXITY, EPOCHS = 8, 300, 10, 10.0, 20


def sklearn_kl_grad(P, Y, exaggeration):
    from sklearn.manifold._t_sne import _kl_divergence
    m, D = Y.shape
    dense = np.asarray(sp.csr_matrix(P).todense()) * exaggeration
    kl, grad = _kl_divergence(Y.ravel().copy(), squareform(dense, checks=False), 1.0, m, D)
    return kl, grad.reshape(m, D) / 4.0


def main():
    X, labels = TR.clusters(M, DIM, SEED)
    K = TR.neighbours_of(PERPLEXITY)
    idx, dist = KR.knn(X, X, K, "euclidean", exclude_self=True)
    p, beta = TR.conditional(idx, dist, PERPLEXITY)
    P = TR.symmetrise(idx, p)
    seed = SEED
    while True:
        rng = np.random.default_rng(seed)
        Y0 = 1e-4 * rng.normal(size=(M, 2))
        Y20, kl20, gains = TR.embed(P, Y0, EPOCHS, return_gains=True)
        Yr, _, gains_r = TR.embed(P, Y0, EPOCHS, reverse=True, return_gains=True)
        if np.array_equal(gains, gains_r):
            break
        seed += 1
    print(f"initial embedding from seed {seed}; reordered trajectory differs by {np.abs(Y20 - Yr).max():.3e} (max |Y20| {np.abs(Y20).max():.3e})")
    Y1 = 10.0 * np.random.default_rng(SEED + 100).normal(size=(M, 2))
    out = dict(X=X, labels=labels.astype(np.int32), perplexity=np.float64(PERPLEXITY), indices=idx.astype(np.int32), dist=dist,
               beta=beta, P_indptr=P.indptr.astype(np.int64), P_indices=P.indices.astype(np.int32), P_data=P.data,
               Y0=Y0, Y1=Y1, Y20=Y20, kl20=np.float64(kl20), epochs=np.int64(EPOCHS), init_seed=np.int64(seed))
    for name, Y in (("Y0", Y0), ("Y1", Y1)):
        for e in (1.0, 12.0):
            kl, g = sklearn_kl_grad(P, Y, e)
            out[f"sk_grad_{name}_e{int(e)}"] = g
            if e == 1.0:
                out[f"sk_kl_{name}"] = np.float64(kl)
    path = os.path.join(HERE, "g8_tsne.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

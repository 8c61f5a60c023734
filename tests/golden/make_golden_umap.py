"""Writes tests/golden/g10_umap.npz: the fixture of the UMAP tests (python tests/golden/make_golden_umap.py, CPU only).

  X (200 x 8, three Gaussian clusters), n_neighbors 15, the K = 14 exact neighbour lists (tests/knn_ref.py), sigma, rho and
  the fuzzy union G of tests/umap_ref.py (f64 values);
  a, b of (spread 1, min_dist 0.1); Y0 = 10 hash_u01(42, 31, .) and the restatement's embedding after 20 epochs from it with
  the values of G and Y stored in f32 (Y20_f32) and in f64 (Y20_f64).

The search of stage 2 is a chain of threshold decisions, so sigma can only be compared bit for bit where none of them hangs
on rounding: the generator tries seeds from SEED upwards until every decision of the 200 searches clears its threshold by
1e-9 (the seed used is stored)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "single-algebra_amd", "python"))

import knn_ref as KR      # noqa: E402
import umap_ref as UR     # noqa: E402

SEED, M, DIM, N_NEIGHBORS, EPOCHS, LAYOUT_SEED = 10, 200, 8, 15, 20, 42


def main():
    seed = SEED
    while True:
        X, labels = UR.clusters(M, DIM, seed)
        idx, dist = KR.knn(X, X, N_NEIGHBORS - 1, "euclidean", exclude_self=True)
        sigma, rho, floored, margin = UR.smooth(idx, dist, N_NEIGHBORS)
        if margin >= 1e-9:
            break
        seed += 1
    print(f"clusters from seed {seed}: smallest decision margin {margin:.3e}, {int(floored.sum())} floored rows")
    G = UR.union(idx, UR.memberships(idx, dist, sigma, rho))
    a, b = UR.find_ab(1.0, 0.1)
    Y0 = UR.init_random(M, 2, LAYOUT_SEED)
    out = dict(X=X, labels=labels.astype(np.int32), n_neighbors=np.int64(N_NEIGHBORS), indices=idx.astype(np.int32), dist=dist,
               sigma=sigma, rho=rho, G_indptr=G.indptr.astype(np.int64), G_indices=G.indices.astype(np.int32), G_data=G.data,
               a=np.float64(a), b=np.float64(b), Y0=Y0, epochs=np.int64(EPOCHS), layout_seed=np.int64(LAYOUT_SEED),
               cluster_seed=np.int64(seed))
    for name, st in (("f32", np.float32), ("f64", np.float64)):
        Gs = G.astype(st)
        Y = UR.layout(Gs, Y0, EPOCHS, a, b, seed=LAYOUT_SEED, storage=st)
        Yr = UR.layout(Gs, Y0, EPOCHS, a, b, seed=LAYOUT_SEED, storage=st, reverse=True)
        print(f"{name}: reordered trajectory differs by {np.abs(Y.astype(np.float64) - Yr).max():.3e} (max |Y| {np.abs(Y).max():.3e})")
        out[f"Y20_{name}"] = Y
    path = os.path.join(HERE, "g10_umap.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/g13_hvg.npz: a small count matrix (f32) with batch labels, a loess input, and what the host restatement
tests/hvg_ref.py makes of them; and, for the two matrices of tests/test_gpu_hvg.py (too large to commit: they are
regenerated from their seeds by hvg_ref.fixture), a checksum of the generated arrays and the restatement's unbatched
seurat_v3 norm_var, so that a drift of the generator or of the restatement shows on the CPU.
Run from the repository root: python tests/golden/make_golden_hvg.py"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hvg_ref as R  # noqa: E402

M, N, K, SEED = 240, 90, 3, 141
BIG = ((1500, 700, 131), (1500, 1300, 132))   # the GPU test's matrices: (m, n, seed)


def checksum(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def main():
    ptr, idx, val = R.fixture(M, N, SEED, np.float32)
    labels = R.batch_labels(M, K, SEED + 1)
    out = {"shape": np.array([M, N, K], dtype=np.int64), "ptr": ptr, "idx": idx, "val": val, "labels": labels}
    for tag, lab in (("one", None), ("k3", labels)):
        r = R.hvg(ptr, idx, val, M, N, labels=lab, K=K, flavor=R.SEURAT_V3, n_top=20, span=0.3)
        for k in ("means", "variances", "variances_norm", "rank", "n_batches_hv", "highly_variable"):
            out[f"v3_{tag}_{k}"] = r[k]
        out[f"v3_{tag}_clip"] = np.stack([b["clip"] for b in r["batches"]])
        out[f"v3_{tag}_n_clipped"] = np.stack([b["n_clipped"] for b in r["batches"]])
    x = R.log1p_normalized(ptr, val)
    for tag, n_top in (("top", 15), ("cut", 0)):
        r = R.hvg(ptr, idx, x, M, N, flavor=R.SEURAT, n_top=n_top, n_bins=20)
        for k in ("means", "dispersions", "dispersions_norm", "highly_variable"):
            out[f"seurat_{tag}_{k}"] = r[k]
    rng = np.random.default_rng(SEED + 2)
    lx = np.sort(rng.normal(0.0, 1.0, 120))
    ly = 0.5 * lx * lx - lx + rng.normal(0.0, 0.1, lx.size)
    out.update({"loess_x": lx, "loess_y": ly, "loess_fit": R.loess(lx, ly, 0.3)})
    for m, n, seed in BIG:
        p, i, v = R.fixture(m, n, seed, np.float32)
        out[f"big_{n}_crc"] = np.array([checksum(p, i, v)], dtype=np.uint64)
        out[f"big_{n}_norm_var"] = R.hvg(p, i, v, m, n, n_top=100)["batches"][0]["norm_var"]
    np.savez_compressed(os.path.join(HERE, "g13_hvg.npz"), **out)


if __name__ == "__main__":
    main()

"""Writes tests/golden/g15_harmony.npz: the 600 x 10 two-batch fixture of the Harmony tests (two batches of 300 rows, three cell
types, a batch shift), 20 given centroids (rows of the fixture) and the outputs of the numpy restatement tests/harmony_ref.py on
it under the default parameters, for the panel stored in f64 and in f32.

    PYTHONPATH=single-algebra_amd/python:tests python tests/golden/make_golden_harmony.py
"""
import os

import numpy as np

import harmony_ref as HR

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N_CLUSTERS = 7, 20


def main():
    Z, batch, kind = HR.two_batch_fixture(300, 10, 3, SEED)
    Y0 = Z[np.random.default_rng(SEED + 100).choice(Z.shape[0], N_CLUSTERS, replace=False)]
    out = dict(Z=Z, batch=batch, kind=kind, Y0=Y0)
    for name, dt in (("f64", np.float64), ("f32", np.float32)):
        r = HR.run(Z, batch, 2, Y0, dtype=dt)
        out[f"{name}_Zcorr"] = r["Zcorr"].astype(dt)
        out[f"{name}_objectives"] = r["objectives"]
        out[f"{name}_passes"] = r["passes"].astype(np.int64)
        out[f"{name}_n_iter"] = np.int64(r["n_iter"])
        out[f"{name}_converged"] = np.int64(r["converged"])
        out[f"{name}_margin"] = np.float64(r["margin"])
        print(name, r["passes"], r["n_iter"], r["converged"], r["margin"])
    np.savez_compressed(os.path.join(HERE, "g15_harmony.npz"), **out)


if __name__ == "__main__":
    main()

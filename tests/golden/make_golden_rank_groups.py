"""Writes tests/golden/g12_rank_groups.npz: two small labelled matrices (integer counts in f32, real values in f64) with the
results of the host restatement tests/rank_groups_ref.py.  Run from the repository root: python tests/golden/make_golden_rank_groups.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rank_groups_ref as R  # noqa: E402

M, N, K = 300, 24, 4


def main():
    out = {"shape": np.array([M, N, K], dtype=np.int64)}
    for tag, kind, dt, seed in (("counts", "counts", np.float32, 121), ("real", "real", np.float64, 122)):
        ptr, idx, val, labels = R.fixture(M, N, K, seed, dt, kind)
        out.update({f"{tag}_ptr": ptr, f"{tag}_idx": idx, f"{tag}_val": val, f"{tag}_labels": labels})
        exact = R.rank_sums(ptr, idx, val, M, N, labels, K)
        for k in ("rank_sum2", "nonzero", "tie_sum"):
            out[f"{tag}_{k}"] = exact[k]
        for tc in (0, 1):
            res = R.rank_groups(ptr, idx, val, M, N, labels, K, tie_correct=bool(tc))
            out[f"{tag}_z_score_tc{tc}"], out[f"{tag}_z_pvalue_tc{tc}"] = res["z_score"], res["z_pvalue"]
        for k in ("group_rows", "mean", "var", "t_score", "t_df"):
            out[f"{tag}_{k}"] = res[k]
    np.savez_compressed(os.path.join(HERE, "g12_rank_groups.npz"), **out)


if __name__ == "__main__":
    main()

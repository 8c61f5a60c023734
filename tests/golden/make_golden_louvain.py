"""Writes tests/golden/g11_louvain.npz: the fixture of the Louvain tests (python tests/golden/make_golden_louvain.py, CPU only;
needs networkx, which no GPU test then does).

Per fixture `name` (tests/louvain_ref.py builds the graphs; G is the fuzzy union of g10_umap.npz, blob the fuzzy union of one
structureless Gaussian blob of 2000 points, whose graph is not stored):
  {name}_indptr / _indices / _data   the graph (f64 values), {name}_gamma the resolution
  {name}_labels, _n_communities, _Q, _n_levels   what the restatement returns at seed 42
  {name}_level_labels (levels x m), _level_Q, _kept, _sweeps   per level that kept a sweep: the composed labels, Q, kept sweeps, sweeps run
  {name}_margin_gain, _margin_q      the smallest decision margins of the run
  {name}_nx_lo, _nx_hi               the lowest and highest modularity of networkx's louvain_communities over seeds 0 .. 4"""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "single-algebra_amd", "python"))

import louvain_ref as LR     # noqa: E402

SEED = 42
NO_GRAPH = ("blob",)   # too large to commit; tests that need it rebuild it


def g10_graph():
    z = np.load(os.path.join(HERE, "g10_umap.npz"))
    m = len(z["G_indptr"]) - 1
    return LR.as_csr(sp.csr_matrix((z["G_data"], z["G_indices"], z["G_indptr"]), shape=(m, m)))


def fixtures():
    """name -> (graph, gamma, dyadic: every sum of its weights is exact in any order)"""
    P = LR.planted(6, 100)
    return {
        "ring64": (LR.ring(64), 1.0, True), "ring1024": (LR.ring(1024), 1.0, True), "grid30": (LR.grid(30, 30), 1.0, True),
        "planted_g05": (P, 0.5, True), "planted_g1": (P, 1.0, True), "planted_g2": (P, 2.0, True),
        "matching64": (LR.matching(64), 1.0, True), "k16": (LR.clique(16), 1.0, True), "star5000": (LR.star(5000), 1.0, True),
        "two_cliques": (LR.two_cliques(8), 1.0, True),
        "G": (g10_graph(), 1.0, False), "blob": (LR.knn_fuzzy_blob(), 1.0, False),
    }


def networkx_range(A, gamma):
    import networkx as nx
    G = nx.from_scipy_sparse_array(A)
    qs = []
    for seed in range(5):
        comm = nx.community.louvain_communities(G, weight="weight", resolution=gamma, seed=seed)
        qs.append(nx.community.modularity(G, comm, weight="weight", resolution=gamma))
    return min(qs), max(qs)


def build(verbose=False):
    out = {}
    for name, (A, gamma, _) in fixtures().items():
        r = LR.run(A, seed=SEED, gamma=gamma)
        lo, hi = networkx_range(A, gamma)
        kept_levels = [lv for lv in r["levels"] if lv["kept"]]
        if name not in NO_GRAPH:
            out[f"{name}_indptr"] = A.indptr.astype(np.int64)
            out[f"{name}_indices"] = A.indices.astype(np.int32)
            out[f"{name}_data"] = A.data.astype(np.float64)
        out[f"{name}_gamma"] = np.float64(gamma)
        out[f"{name}_labels"] = r["labels"]
        out[f"{name}_n_communities"] = np.int64(r["n_communities"])
        out[f"{name}_Q"] = np.float64(r["Q"])
        out[f"{name}_n_levels"] = np.int64(r["n_levels"])
        out[f"{name}_level_labels"] = np.array([lv["labels"] for lv in kept_levels], dtype=np.int32).reshape(len(kept_levels), A.shape[0])
        out[f"{name}_level_Q"] = np.array([lv["Q"] for lv in kept_levels], dtype=np.float64)
        out[f"{name}_kept"] = np.array([lv["kept"] for lv in r["levels"]], dtype=np.int64)
        out[f"{name}_sweeps"] = np.array([lv["sweeps"] for lv in r["levels"]], dtype=np.int64)
        out[f"{name}_margin_gain"] = np.float64(r["margin_gain"])
        out[f"{name}_margin_q"] = np.float64(r["margin_q"])
        out[f"{name}_nx_lo"] = np.float64(lo)
        out[f"{name}_nx_hi"] = np.float64(hi)
        if verbose:
            print(f"{name}: Q {r['Q']:.5f} (networkx {lo:.5f} .. {hi:.5f}), {r['n_communities']} communities, {r['n_levels']} levels, "
                  f"sweeps {out[f'{name}_sweeps'].tolist()}, margins {r['margin_gain']:.2e} / {r['margin_q']:.2e}")
    return out


def main():
    out = build(verbose=True)
    path = os.path.join(HERE, "g11_louvain.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

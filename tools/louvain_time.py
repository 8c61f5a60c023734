#!/usr/bin/env python3
"""What Louvain costs on the neighbour graph (GPU): python tools/louvain_time.py [--rows 10000,50000,200000] [--reps 3] [--out F]

Device time from events on the stream the Session runs on, around whole calls (launches, gaps and the call's read-backs
included), best and median of `reps` after a warm-up.  Per m (f32 and f64), on the fuzzy union (n_neighbors 15) of 50-column
score-like rows:
  whole    Session.louvain on the resident graph at the defaults: every level, every aggregation;
  sweep    (louvain with max_levels 1, max_sweeps 24 - the same with max_sweeps 8) / 16: both runs carry the same set-up (row
           lists, degrees, the start's modularity) and the same aggregation at the end of a level that is cut short, so the
           difference holds level-0 sweeps 8 .. 23 and nothing else -- each with its keep / undo: the vertex sort, the
           totals, the modularity.  The host looks at the device flag every 8 sweeps in both.
Beside the sweep, the time two passes over the graph (offsets, columns, values: the sweep's walk and the walk for s_i) take at
the copy rate the box attains (sapca_measure_copy_gbs): a floor, not an estimate.  networkx's louvain_communities on the same
graph, at 10 000 rows only (host time).
profiles/louvain_time.txt is this script's output."""
import argparse
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sapca import _lib as L  # noqa: E402
from sapca import ops  # noqa: E402
from umap_time import scores, timed  # noqa: E402


def networkx_ms(G):
    import networkx as nx
    import scipy.sparse as sp
    d = G.as_device_csr()
    A = sp.csr_matrix((d.values.cpu().numpy().astype("float64"), d.col_indices.cpu().numpy(), d.row_offsets.cpu().numpy()), shape=G.shape)
    g = nx.from_scipy_sparse_array(A)
    t0 = time.perf_counter()
    comm = nx.community.louvain_communities(g, weight="weight", seed=0)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, nx.community.modularity(g, comm, weight="weight"), len(comm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="10000,50000,200000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sess = ops.Session()
    gbs = C.c_double()
    L.check(sess._h, L.load().sapca_measure_copy_gbs(sess._h, C.c_uint64(1 << 30), C.c_uint32(5), C.byref(gbs)))
    lines = [f"Louvain on the fuzzy union of score-like rows (d = 50, n_neighbors 15), {torch.cuda.get_device_name(0)}; 1 warm-up + "
             f"{args.reps} timed calls, ms (best / median); streaming copy {gbs.value:.0f} GB/s"]
    for m in [int(r) for r in args.rows.split(",")]:
        for dt, name in ((torch.float32, "f32"), (torch.float64, "f64")):
            x = scores(m, 50, dt)
            idx, dist = sess.knn(x, n_neighbors=14)
            G = sess.umap_graph(idx, dist, 15)[0]
            whole = timed(lambda: sess.louvain(G), args.reps)
            labels, n, q, levels = sess.louvain(G)
            short = timed(lambda: sess.louvain(G, max_levels=1, max_sweeps=8), args.reps)
            long_ = timed(lambda: sess.louvain(G, max_levels=1, max_sweeps=24), args.reps)
            sweep = [(b - a) / 16.0 for a, b in zip(short, long_)]
            size = 4 if dt == torch.float32 else 8
            floor_ms = 2 * (G.nnz * (4 + size) + (m + 1) * 8) / (gbs.value * 1e9) * 1e3
            lines.append(f"m = {m} {name}: graph {G.nnz} entries   whole {whole[0]:9.2f} / {whole[1]:9.2f}  ({n} communities, Q {q:.5f}, "
                         f"{levels} levels)   level-0 sweep {sweep[0]:7.4f} / {sweep[1]:7.4f}  (two passes over the graph at the copy rate: "
                         f"{floor_ms:.4f})")
            print(lines[-1], flush=True)
            if m == 10000 and dt == torch.float64:
                try:
                    ms, qn, nn = networkx_ms(G)
                    lines.append(f"m = {m}: networkx louvain_communities (seed 0, host) {ms:9.1f} ms, {nn} communities, Q {qn:.5f}")
                except ImportError:
                    lines.append(f"m = {m}: networkx is not installed, no host figure")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()

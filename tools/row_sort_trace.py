#!/usr/bin/env python3
"""The kernels the row-sort stage enqueues, for comparing two builds of the library (profiles/row_sort_refactor_ab.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o rs -- python tools/row_sort_trace.py
    python tools/row_sort_trace.py --list DIR            # the dispatches of that run in order, then the calls per kernel

The run makes one call each of canonicalize (the raw rows below as a matrix: unsorted, with duplicates), tsne_affinities and
umap_graph, f32, on hand-made neighbour lists that take the sort through every length class: K = 3, m = 4200, every row lists
row 0 (a raw row beyond canon_lds_cap() that merges mutual pairs), 300 rows list row 1 (a row between 65 entries and the cap),
the other slots are a ring.  Every input is built on the host, so the trace holds the library's kernels and nothing else.
SAPCA_LIB_PATH selects the library."""
import csv
import glob
import os
import re
import sys

import numpy as np


def hub_lists(m=4200, hub=300):
    i = np.arange(m)
    ring = lambda s: 2 + (i - 2 + s) % (m - 2)   # noqa: E731
    idx = np.stack([np.zeros(m, dtype=np.int64), np.where((i >= 2) & (i < 2 + hub), 1, ring(1)), ring(2)], axis=1)
    idx[0], idx[1] = (1, 2, 3), (0, 2, 3)
    return idx.astype(np.int32), np.random.default_rng(5).uniform(0.5, 1.5, size=(m, 3)).astype(np.float32)


def raw_rows(idx):
    """row i: its own slots, then the rows that list it -- what the graph builders emit, as (ptr, columns)"""
    m, K = idx.shape
    rows = np.concatenate([np.repeat(np.arange(m), K), idx.ravel()])
    cols = np.concatenate([idx.ravel(), np.repeat(np.arange(m), K)])
    order = np.argsort(rows, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int64), cols[order].astype(np.int32)


def run():
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "single-algebra_amd", "python"))
    from sapca import ops
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    idx, dist = hub_lists()
    ptr, cols = raw_rows(idx)
    sess = ops.Session()
    A = ops.ResidentCsr.from_torch(sess, dev(ptr), dev(cols), dev(np.ones(cols.size, dtype=np.float32)), (idx.shape[0],) * 2)
    C, rep = A.canonicalize()
    P = sess.tsne_affinities(dev(idx), dev(dist), 2.0)[0]
    G = sess.umap_graph(dev(idx), dev(dist), 4)[0]
    print(f"canonicalize: {rep.unsorted_rows} unsorted rows, {A.nnz - C.nnz} entries merged; t-SNE graph {P.nnz} entries, UMAP graph {G.nnz}")


def listing(directory):
    trace = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)[0]
    short = lambda n: re.sub(r"\(.*", "", re.sub(r"^void ", "", n.replace("(anonymous namespace)::", "")))   # noqa: E731
    names = [short(r["Kernel_Name"]) for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))]
    print(f"{len(names)} dispatches, in order:")
    for j, n in enumerate(names):
        print(f"  {j:3d} {n}")
    print("calls per kernel:")
    for n in sorted(set(names)):
        print(f"  {names.count(n):3d} {n}")


if __name__ == "__main__":
    listing(sys.argv[2]) if sys.argv[1:2] == ["--list"] else run()

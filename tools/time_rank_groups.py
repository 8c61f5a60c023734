#!/usr/bin/env python3
"""What rank_groups costs on the headline matrix (GPU): python tools/time_rank_groups.py [--rows 200000] [--cols 20000] [--reps 5] [--out F]

The sapca.synth gapped matrix of the headline shape (200 000 x 20 000, density 0.03, f32), row-normalised and log1p'd on the
device as a session would have it, labelled by a k-means with K = 16 on 16 principal-component scores.  Device time from
events on the current stream around whole calls (the calls block: launches, gaps, read-backs and the host finish are all
inside), 1 warm-up + `reps` timed calls, ms as median (min .. max):
  rank_groups       method "wilcoxon", "t-test" and "both" through the Python layer (its result object sorts `names` and
                    takes the t-test's p-values from scipy on the host);
  C call            sapca_rank_groups_csr_device_f32 itself into arrays that exist: the z outputs alone (group sizes,
                    transposition, rank pass, host finish of z and p), the moment outputs alone (group sizes, transposition,
                    labelled statistics, host finish of mean, var, t, df), and all of them;
  rank_sums         the exact quantities alone: the C call for z and p minus this is the host finish of z and p on K x n values;
  yardstick         batch_stats(grouped_axis 0) on the same matrix and codes: the same transposition plus one pass over A^T;
  transposition     stats(COLUMN): the transposition plus the plain column sums, the cheapest pass there is;
  by class          rank_sums on the sub-matrix of each length class's columns (ResidentCsr.select): each figure carries the
                    transposition of its own sub-matrix and the group sizes, and the long class its segmented radix sort AND
                    its walk -- the sort is not separated from the run-and-accumulate step here (the two LDS classes do both in
                    one kernel).
profiles/rank_groups_time.txt is this script's output."""
import argparse
import ctypes as C
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
import sapca  # noqa: E402
from sapca import _lib as L  # noqa: E402
from sapca import ops, synth  # noqa: E402
from sapca import PowerIterationNormalizer as PIN  # noqa: E402
from sapca import SVDMethod  # noqa: E402


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return f"{out[len(out) // 2]:9.1f} ({out[0]:.1f} .. {out[-1]:.1f})"


def c_call(X, labels, K, want):
    """the C entry point with the outputs named in `want`, the others NULL"""
    n = X.shape[1]
    out = {k: np.zeros((K, n), dtype=np.uint64 if k == "nz" else np.float64) for k in want}
    rows = np.zeros(K, dtype=np.uint64)
    p = lambda k: ops._p(out[k], C.c_uint64 if k == "nz" else C.c_double) if k in out else None   # noqa: E731
    fn = L.load().sapca_rank_groups_csr_device_f32

    def run():
        L.check(X._s._h, fn(*X._args(), C.c_void_p(labels.data_ptr()), C.c_uint32(K), C.c_int32(0), ops._p(rows, C.c_uint64),
                            p("mean"), p("var"), p("nz"), p("t"), p("df"), p("z"), p("pz")))
    return run


def class_limits():
    text = open(os.path.join(ROOT, "single-algebra_amd", "csrc", "rankgroups.h")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr int (kRank\w+) = (\d+);", text)}
    return got["kRankWaveMax"], got["kRankLdsMax"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--cols", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n, K = args.rows, args.cols, 16
    torch.cuda.set_device(0)
    dev = synth.gapped_csr(m, n, 0.03, 50, seed=42, dtype=torch.float32, device="cuda:0")
    sess = ops.Session()
    X = ops.ResidentCsr(sess, (m, n), dev[2].numel(), np.float32, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr())
    X.normalize(X.stats(ops.ROW)[0], 1e4, ops.ROW).log1p()
    est = sapca.SparsePCABuilder.new().n_components(16).svd_method(SVDMethod.Random(10, 2, PIN.QR)).build()
    scores = est.fit_transform(sapca.DeviceCsr(*dev, (m, n)))
    labels = sess.kmeans(scores, n_clusters=K)[0]
    codes = labels.cpu().numpy()
    lens = X.stats(ops.COLUMN)[2].astype(np.int64)
    wave_max, lds_max = class_limits()
    classes = (("wave", lens <= wave_max), ("workgroup", (lens > wave_max) & (lens <= lds_max)), ("long", lens > lds_max))
    lines = [f"rank_groups on the gapped matrix {m} x {n}, {X.nnz} entries (f32, normalised, log1p), K = {K} k-means labels "
             f"(group rows {np.bincount(codes, minlength=K).tolist()}), {torch.cuda.get_device_name(0)}",
             f"1 warm-up + {args.reps} timed calls, ms: median (min .. max)",
             "columns by stored length: " + ", ".join(f"{name} {int(mask.sum())} columns / {int(lens[mask].sum())} entries" for name, mask in classes)
             + f" (limits {wave_max}, {lds_max})"]
    for method in ("wilcoxon", "t-test", "both"):
        lines.append(f"  rank_groups {method:9s} {timed(lambda: X.rank_groups(labels, K, method=method), args.reps)}")
    for name, want in (("z, p", ("z", "pz")), ("mean, var, t, df", ("mean", "var", "t", "df")), ("all", ("mean", "var", "nz", "t", "df", "z", "pz"))):
        lines.append(f"  C call, {name:17s} {timed(c_call(X, labels, K, want), args.reps)}")
    lines.append(f"  rank_sums             {timed(lambda: X.rank_sums(labels, K), args.reps)}")
    lines.append(f"  yardstick batch_stats {timed(lambda: X.batch_stats(0, codes, K), args.reps)}")
    lines.append(f"  transposition + sums  {timed(lambda: X.stats(ops.COLUMN), args.reps)}")
    for name, mask in classes:
        if mask.any():
            S = X.select(cols=mask)
            lines.append(f"  rank_sums, {name:9s}  {timed(lambda: S.rank_sums(labels, K), args.reps)}   "
                         f"(sub-matrix of {S.shape[1]} columns, {S.nnz} entries; its yardstick {timed(lambda: S.batch_stats(0, codes, K), args.reps).strip()})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

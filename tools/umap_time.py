#!/usr/bin/env python3
"""What the UMAP stages cost (GPU): python tools/umap_time.py [--rows 10000,50000,200000] [--reps 3] [--out F]

Device time from events on the stream the Session runs on, around whole calls (launches, gaps and the call's final
synchronisation included), best and median of `reps` after a warm-up.  Per m (output_dim 2, f32 and f64), on 50-column
score-like rows at n_neighbors 15:
  knn      Session.knn with 14 neighbours (stage 1);
  graph    Session.umap_graph (stages 2-3: the smooth-distance search, the union);
  epoch    (umap_embed with 205 epochs - umap_embed with 5 epochs) / 200: no host synchronisation lies inside the loop and both
           calls carry the same set-up (w_max, the schedule, the start), so the difference holds epochs and nothing else.  The
           two runs differ in n_epochs, hence in alpha and in which entries the filter leaves out: the figure is the average
           epoch of a 205-epoch layout, not any single one;
  whole    Session.umap at the default number of epochs (500 up to 10000 rows, else 200), everything included.
Beside the epoch, the bytes it must stream at least once -- the two f64 schedule arrays read (written back where due), the
column index and the value of every stored entry -- at the copy rate the box attains (sapca_measure_copy_gbs): the kernel is
gather-latency bound on Y, so this is a floor, not an estimate.
profiles/umap_time.txt is this script's output."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
from sapca import _lib as L  # noqa: E402
from sapca import ops  # noqa: E402


def scores(rows, d, dtype, seed=0):
    """cluster structure with a decaying spectrum, like the leading principal components of count data"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = 10.0 / torch.arange(1, d + 1, device="cuda", dtype=torch.float64).sqrt()
    centres = torch.randn((40, d), generator=g, device="cuda", dtype=torch.float64) * scale
    which = torch.randint(0, 40, (rows,), generator=g, device="cuda")
    x = centres[which] + 0.35 * scale * torch.randn((rows, d), generator=g, device="cuda", dtype=torch.float64)
    return x.to(dtype).contiguous()


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
    return out[0], out[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="10000,50000,200000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sess = ops.Session()
    gbs = C.c_double()
    L.check(sess._h, L.load().sapca_measure_copy_gbs(sess._h, C.c_uint64(1 << 30), C.c_uint32(5), C.byref(gbs)))
    lines = [f"UMAP on score-like rows (d = 50, n_neighbors 15, output_dim 2), {torch.cuda.get_device_name(0)}; 1 warm-up + {args.reps} "
             f"timed calls, ms (best / median); streaming copy {gbs.value:.0f} GB/s"]
    for m in [int(r) for r in args.rows.split(",")]:
        for dt, name in ((torch.float32, "f32"), (torch.float64, "f64")):
            x = scores(m, 50, dt)
            knn = timed(lambda: sess.knn(x, n_neighbors=14), args.reps)
            idx, dist = sess.knn(x, n_neighbors=14)
            graph = timed(lambda: sess.umap_graph(idx, dist, 15), args.reps)
            G = sess.umap_graph(idx, dist, 15)[0]
            short = timed(lambda: sess.umap_embed(G, n_epochs=5), args.reps)
            long_ = timed(lambda: sess.umap_embed(G, n_epochs=205), args.reps)
            whole = timed(lambda: sess.umap(x), args.reps)
            epoch = [(b - a) / 200.0 for a, b in zip(short, long_)]
            size = 4 if dt == torch.float32 else 8
            floor_ms = G.nnz * (2 * 8 + 4 + size) / (gbs.value * 1e9) * 1e3
            lines.append(f"m = {m} {name}: knn {knn[0]:9.2f} / {knn[1]:9.2f}   graph ({G.nnz} entries) {graph[0]:8.2f} / {graph[1]:8.2f}   "
                         f"epoch {epoch[0]:7.4f} / {epoch[1]:7.4f}  (one pass over the schedule and the graph at the copy rate: {floor_ms:.4f})   "
                         f"whole, {500 if m <= 10000 else 200} epochs {whole[0]:9.2f} / {whole[1]:9.2f}")
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

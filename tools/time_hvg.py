#!/usr/bin/env python3
"""What the variable-genes operators cost on the headline matrix (GPU): python tools/time_hvg.py [--rows 200000] [--cols 20000] [--reps 5] [--out F]

The sapca.synth gapped matrix of the headline shape (200 000 x 20 000, density 0.03, f32) with its values turned into small
whole counts on the device (floor(4 |x|), stored zeros included).  Device time from events on the current stream around whole
calls (the calls block: launches, gaps, read-backs and the host finish are all inside), 1 warm-up + `reps` timed calls, ms as
median (min .. max):
  CLIP pass          hvg_moments("clip") with a clip that bites: the transposition plus one wave-per-column pass over A^T;
  yardstick          masked_stats(COLUMN) without a mask: the plain exact column pass over A in the long accumulators;
  transposition      stats(COLUMN): the transposition plus the plain f64 column sums, what the CLIP pass shares with it;
  loess              Session.loess at n = 20 000 points, span 0.3 (6 000-point windows), host arrays in and out;
  seurat_v3          the whole unbatched highly_variable call (n_top 2000): group sizes, transposition, two passes, loess, the
                     n-sized steps and the host's ranking;
  EXPM1 pass, seurat hvg_moments("expm1") and the whole unbatched call of the other flavour, on the log1p of the same values.
profiles/hvg_time.txt is this script's output."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
from sapca import ops, synth  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--cols", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n = args.rows, args.cols
    torch.cuda.set_device(0)
    dev = synth.gapped_csr(m, n, 0.03, 50, seed=42, dtype=torch.float32, device="cuda:0")
    dev[2].copy_(torch.floor(dev[2].abs() * 4.0))
    torch.cuda.synchronize()
    sess = ops.Session()
    X = ops.ResidentCsr(sess, (m, n), dev[2].numel(), np.float32, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr())
    s, q, cnt = X.masked_stats(ops.COLUMN)[:3]
    mean = s / m
    clip = mean + 2.0 * np.sqrt(np.maximum(q / m - mean * mean, 0.0))
    clipped = X.hvg_moments("clip", clip=clip)["n_clipped"]
    rng = np.random.default_rng(1)
    lx = rng.normal(0.0, 1.0, 20_000)
    ly = 0.5 * lx * lx + rng.normal(0.0, 0.3, lx.size)
    lines = [f"variable genes on the gapped matrix {m} x {n}, {X.nnz} entries (f32, whole counts, largest {float(dev[2].max()):.0f}), "
             f"{torch.cuda.get_device_name(0)}",
             f"1 warm-up + {args.reps} timed calls, ms: median (min .. max); the clip of the CLIP pass is mean + 2 sd: "
             f"{int(clipped.sum())} entries clipped in {int((clipped > 0).sum())} columns",
             f"  CLIP pass             {timed(lambda: X.hvg_moments('clip', clip=clip), args.reps)}",
             f"  yardstick masked_stats{timed(lambda: X.masked_stats(ops.COLUMN), args.reps)}",
             f"  transposition + sums  {timed(lambda: X.stats(ops.COLUMN), args.reps)}",
             f"  loess, n = 20 000     {timed(lambda: sess.loess(lx, ly, 0.3), args.reps)}",
             f"  seurat_v3, n_top 2000 {timed(lambda: X.highly_variable(2000), args.reps)}"]
    X.log1p()   # the other flavour's input
    lines += [f"  EXPM1 pass (log1p'd)  {timed(lambda: X.hvg_moments('expm1'), args.reps)}",
              f"  seurat, n_top 2000    {timed(lambda: X.highly_variable(2000, 'seurat'), args.reps)}"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

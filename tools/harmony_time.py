#!/usr/bin/env python3
"""What Harmony costs (GPU): python tools/harmony_time.py [--rows 200000] [--reps 3] [--kernel-stats DIR] [--out F]

200 000 x 50 score-like rows in four batches, K = 100, f32, the defaults of the Python layer otherwise.  Device time from events
on the stream the Session runs on, around whole calls (launches, gaps, read-backs and the final synchronisation included), best
and median of `reps` after a warm-up:
  pass         (one outer iteration with 10 clustering passes - one with 5) / 5 from given centroids: both calls carry the same
               set-up and one correction, so the difference holds passes and nothing else (the line names the passes that ran);
  block pair   the same difference at n_blocks = 80 against n_blocks = 20, per added block: a fold and a fused block launch
               over a quarter of the rows -- what a pair costs beyond the rows it moves;
  correction   Session.harmony_correct, one call: batch counts and sort, the ridge sums, beta, the m x K x d product.
--one runs three calls of one outer iteration with 10 passes and prints nothing else: the child of a
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/harmony_time.py --one` run.  With --kernel-stats DIR the kernels of that
run are listed with their launches and mean times, the share of the summed kernel time that the fused block kernel holds, and
the bytes a block launch has to move (its rows of Zc in, R and dist out; Y and the penalty table stay in L2) against its time,
beside the box's own streaming-copy rate.  profiles/harmony_time.txt is this script's output."""
import argparse
import csv
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
import sapca  # noqa: E402
from sapca import ops  # noqa: E402

D, K, B, PASS_LO, PASS_HI = 50, 100, 4, 5, 10


def scores(rows, seed=0):
    """cell types with a decaying spectrum and a shift per batch, like the leading principal components of several samples"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = 10.0 / torch.arange(1, D + 1, device="cuda", dtype=torch.float64).sqrt()
    centres = torch.randn((40, D), generator=g, device="cuda", dtype=torch.float64) * scale
    shift = torch.randn((B, D), generator=g, device="cuda", dtype=torch.float64) * 0.3 * scale
    which = torch.randint(0, 40, (rows,), generator=g, device="cuda")
    batch = torch.randint(0, B, (rows,), generator=g, device="cuda")
    x = centres[which] + shift[batch] + 0.35 * scale * torch.randn((rows, D), generator=g, device="cuda", dtype=torch.float64)
    return x.to(torch.float32).contiguous(), batch.to(torch.int32).contiguous()


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


def read_kernel_stats(root):
    """[(short kernel name, calls, mean ns)] of the library's kernels in the rocprofv3 kernel_stats CSV under root"""
    for base, _, files in os.walk(root):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                rows = []
                with open(os.path.join(base, f)) as fh:
                    for r in csv.DictReader(fh):
                        name = r["Name"]
                        if "sapca" in name or "rocprim" in name:
                            found = re.findall(r"(\w*kernel\w*)", name)
                            rows.append((("rocprim::" if "rocprim" in name else "") + (found[0] if found else name[:40]), int(r["Calls"]),
                                         float(r["AverageNs"])))
                return rows
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harmony_time.txt"))
    a = ap.parse_args()
    sess = ops.Session(stream=torch.cuda.current_stream().cuda_stream)
    x, batch = scores(a.rows)
    start = x[torch.arange(0, a.rows, a.rows // K, device="cuda")[:K]].clone()
    m = a.rows

    def run(passes, n_blocks=20):
        return sess.harmony(x, batch, n_clusters=K, n_batches=B, init=start, n_blocks=n_blocks, max_iter_harmony=1, max_iter_cluster=passes,
                            epsilon_cluster=0.0)

    if a.one:
        for _ in range(3):
            res = run(PASS_HI)[1]
        print(f"--one: passes {res.passes.tolist()}")
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    gbs = sapca.SparsePCABuilder.new().n_components(2).build().measure_copy_gbs(1 << 30, 5)
    say(f"Harmony on {m} x {D} score-like rows, K = {K}, B = {B}, f32, {torch.cuda.get_device_name(0)}; 1 warm-up + {a.reps} timed calls, "
        f"ms (best / median); streaming copy {gbs:.0f} GB/s (read + write)")
    held = {}
    per = {}
    for nb in (20, 80):
        t_lo = timed(lambda: held.__setitem__("lo", run(PASS_LO, nb)[1]), a.reps)
        t_hi = timed(lambda: held.__setitem__("hi", run(PASS_HI, nb)[1]), a.reps)
        ran = int(held["hi"].passes[0]) - int(held["lo"].passes[0])
        per[nb] = tuple((hi - lo) / max(ran, 1) for lo, hi in zip(t_lo, t_hi))
        say(f"n_blocks = {nb}: one outer iteration with {int(held['lo'].passes[0])} passes {t_lo[0]:.2f} / {t_lo[1]:.2f}, with "
            f"{int(held['hi'].passes[0])} passes {t_hi[0]:.2f} / {t_hi[1]:.2f}: a pass {per[nb][0]:.3f} / {per[nb][1]:.3f}, "
            f"{per[nb][0] / nb * 1e3:.1f} us per block of it")
    say(f"a fold | block launch pair beyond the rows it moves: {(per[80][0] - per[20][0]) / 60 * 1e3:.1f} us "
        f"(the pass at 80 blocks less the pass at 20, per added block)")
    R = held["hi"].R
    t_corr = timed(lambda: sess.harmony_correct(x, batch, B, R), a.reps)
    say(f"correction (one harmony_correct call): {t_corr[0]:.2f} / {t_corr[1]:.2f}")
    whole = timed(lambda: held.__setitem__("all", sess.harmony(x, batch, n_clusters=K, n_batches=B, init=start)[1]), 1)
    say(f"a whole run under the defaults from given centroids: {whole[0]:.1f} ms, passes {held['all'].passes.tolist()}, "
        f"converged {held['all'].converged}")
    if a.kernel_stats:
        rows = read_kernel_stats(a.kernel_stats)
        if rows is None:
            say(f"no kernel_stats.csv under {a.kernel_stats}")
        else:
            rows.sort(key=lambda r: -r[1] * r[2])
            total = sum(c * t for _, c, t in rows)
            say(f"per kernel, from a rocprofv3 --kernel-trace --stats run of `--one` (3 calls of one outer iteration, {PASS_HI} passes, 20 blocks):")
            for n, c, t in rows:
                say(f"    {n:32s} {c:6d} launches, {t / 1e3:9.2f} us each, {100.0 * c * t / total:5.1f} % of the kernel time")
            blk = [(c, t) for n, c, t in rows if n.startswith("hm_block_kernel")]
            if blk:
                share = sum(c * t for c, t in blk) / total
                c, t = max(blk, key=lambda r: r[0])           # the per-block launches (the initialisation's one launch over all rows aside)
                nbytes = (m / 20) * (D + 2 * K) * 4
                say(f"the fused block kernel holds {100.0 * share:.1f} % of the summed kernel time; a launch over {m // 20} rows has to move "
                    f"{nbytes / 1e6:.2f} MB (Zc in, R and dist out) in {t / 1e3:.1f} us: {nbytes / t:.0f} GB/s against the copy's {gbs:.0f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

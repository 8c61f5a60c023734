#!/usr/bin/env python3
"""What a k-means iteration costs (GPU): python tools/kmeans_time.py [--rows 50000,200000] [--clusters 8,64,256] [--reps 3]
                                                                   [--sklearn] [--kernel-stats DIR] [--out F]

Device time from events on the stream the Session runs on, around whole calls (launches, gaps and the call's final
synchronisation included), best and median of `reps` after a warm-up.  Per (m, k) on 50-column score-like rows, f32 and f64:
  seeding      Session.kmeans_seed, one call: k-means++, two launches per centre;
  iteration    (kmeans with 12 iterations - kmeans with 2) / 10 from the first k rows, tol = 0: both calls carry the same set-up
               and closing assignment, so the difference holds iterations and nothing else (the line says so if the run
               converged before 12 and the difference would hold no-ops);
  assign       Session.kmeans_assign, one call: norms, ranking, refine, distances, inertia, read-back; with the share of rows the
               ranking left to the f64 pass;
  update       Session.kmeans_update, one call: counting sort, sums, means.
Beside them two yardsticks that do not come from the code under test: the time to read x once at the rate of the box's own
streaming copy (sapca_measure_copy_gbs), and the issue-slot estimate of the ranking -- one 16x16x4 matrix-core instruction per
16 rows x 16 centroids x 4 columns, 32 cycles each (64 in f64) on 256 CUs x 4 SIMDs at 2.4 GHz -- which nobody had measured
when it was written down.  --one M,K,DTYPE runs three 12-iteration calls of one shape and prints nothing else: the child of a
rocprofv3 --kernel-trace --stats run per shape, written to DIR/M_K_DTYPE/.  With --kernel-stats DIR every line splits its
iteration into the mean kernel time of ranking (the centroids' norms and the matrix-core kernel), refine (the f64 pass over the
listed rows) and update (counting, scan, placing, sums, means, control step), and one shape is listed kernel by kernel with its
launches per iteration.
With --sklearn, for orientation only (another processor): scikit-learn's Lloyd iteration on the CPU at the same shapes.
profiles/kmeans_time.txt is this script's output."""
import argparse
import csv
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
import sapca  # noqa: E402
from sapca import ops  # noqa: E402

SIMDS, CLOCK = 256 * 4, 2.4e9
ITER_LO, ITER_HI = 2, 12


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


def ranking_estimate_ms(m, k, d, f64):
    instructions = -(-m // 16) * -(-k // 16) * -(-d // 4)
    return instructions * (64 if f64 else 32) / SIMDS / CLOCK * 1e3


RANKING, REFINE = ("km_rank_kernel", "knn_prepare_kernel"), ("km_refine_kernel",)
UPDATE = ("km_count_kernel", "km_place_kernel", "km_sums_kernel", "km_finalize_kernel", "km_step_kernel", "rocprim::")


def stats_file(root, m, k, name):
    """the kernel_stats CSV of the --one child of a shape under root, or None"""
    for base, _, files in os.walk(os.path.join(root, f"{m}_{k}_{name}")):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                return os.path.join(base, f)
    return None


def stage_split(path):
    """(ranking, refine, update) in us: the mean time of one launch of each of a stage's kernels, added up (every one of them
    runs once per iteration; the norms' mean includes the one larger launch per call over the rows)"""
    rows = read_kernel_stats(path)
    pick = lambda names: sum(a for n, _, a in rows if any(n.startswith(p) for p in names)) / 1e3   # noqa: E731
    return pick(RANKING), pick(REFINE), pick(UPDATE)


def read_kernel_stats(path):
    """[(short kernel name, calls, mean ns)] of the library's kernels in a rocprofv3 kernel_stats CSV"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            if "sapca" in name or "rocprim" in name:
                found = re.findall(r"(\w*kernel\w*)", name)
                short = found[0] if found else name[:40]
                rows.append((("rocprim::" if "rocprim" in name else "") + short, int(r["Calls"]), float(r["AverageNs"])))
    return rows


def digest_kernel_stats(path, calls, iterations):
    """launches and mean time per kernel of the --one child (calls x iterations iterations), the library's kernels only"""
    rows = read_kernel_stats(path)
    rows.sort(key=lambda r: -r[1] * r[2])
    out = [f"    {n:28s} {c / (calls * iterations):6.2f} launches / iteration, {a / 1e3:8.2f} us each" for n, c, a in rows]
    total = sum(c for _, c, _ in rows) / (calls * iterations)
    busy = sum(c * a for _, c, a in rows) / (calls * iterations) / 1e3
    out.append(f"    all of them: {total:.1f} launches per iteration (set-up and closing assignment spread over the {iterations}), "
               f"{busy:.1f} us of kernel time per iteration")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="50000,200000")
    ap.add_argument("--clusters", default="8,64,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--one", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernel-stats-shape", default="200000,64,f32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_time.txt"))
    a = ap.parse_args()
    sess = ops.Session(stream=torch.cuda.current_stream().cuda_stream)
    if a.one:
        m, k, name = a.one.split(",")
        x = scores(int(m), 50, torch.float32 if name == "f32" else torch.float64)
        for _ in range(3):
            n_iter = sess.kmeans(x, n_clusters=int(k), init=x[:int(k)], max_iter=ITER_HI, tol=0.0)[3]
        print(f"--one {a.one}: n_iter {n_iter}")
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    est = sapca.SparsePCABuilder.new().n_components(2).build()
    gbs = est.measure_copy_gbs(1 << 30, 5)
    say(f"k-means on score-like rows (d = 50), {torch.cuda.get_device_name(0)}; 1 warm-up + {a.reps} timed calls, ms (best / median); "
        f"streaming copy {gbs:.0f} GB/s (read + write)")
    for m in (int(v) for v in a.rows.split(",")):
        for k in (int(v) for v in a.clusters.split(",")):
            for dtype, name in ((torch.float32, "f32"), (torch.float64, "f64")):
                x = scores(m, 50, dtype)
                start = x[:k].clone()
                read_ms = x.numel() * x.element_size() / (gbs * 1e9) * 1e3
                rank_ms = ranking_estimate_ms(m, k, 50, name == "f64")
                t_seed = timed(lambda: sess.kmeans_seed(x, k, seed=1), a.reps)
                held = {}
                t_lo = timed(lambda: sess.kmeans(x, n_clusters=k, init=start, max_iter=ITER_LO, tol=0.0), a.reps)
                t_hi = timed(lambda: held.__setitem__("run", sess.kmeans(x, n_clusters=k, init=start, max_iter=ITER_HI, tol=0.0)), a.reps)
                it = tuple((hi - lo) / (ITER_HI - ITER_LO) for lo, hi in zip(t_lo, t_hi))
                labels, cen, _, n_iter = held["run"]
                t_assign = timed(lambda: held.__setitem__("assign", sess.kmeans_assign(x, cen)), a.reps)
                t_update = timed(lambda: sess.kmeans_update(x, labels, cen), a.reps)
                n_amb = held["assign"][3]
                trace = stats_file(a.kernel_stats, m, k, name) if a.kernel_stats else None
                split = "" if trace is None else "   kernels per iteration, us: ranking %.1f  refine %.1f  update %.1f" % stage_split(trace)
                say(f"m = {m} k = {k:3d} {name}: iteration {it[0]:7.3f} / {it[1]:7.3f}"
                    + ("" if n_iter == ITER_HI else f" (converged after {n_iter}: not an iteration's time)")
                    + split + f"   assign call {t_assign[0]:7.3f} / {t_assign[1]:7.3f} ({100.0 * n_amb / m:.2f} % of rows ambiguous)"
                    f"   update call {t_update[0]:7.3f} / {t_update[1]:7.3f}   seeding {t_seed[0]:8.2f} / {t_seed[1]:8.2f}"
                    f"   | read x once {read_ms:.3f}, ranking issue-slot estimate (unmeasured when stated) {rank_ms:.3f}")
                del x, start, held, labels, cen
    if a.kernel_stats:
        say(f"per kernel, from the rocprofv3 --kernel-trace --stats run of `--one {a.kernel_stats_shape}` (3 calls of {ITER_HI} iterations):")
        for line in digest_kernel_stats(stats_file(a.kernel_stats, *a.kernel_stats_shape.split(",")), 3, ITER_HI):
            say(line)
    if a.sklearn:
        from sklearn.cluster import KMeans
        for m in (int(v) for v in a.rows.split(",")):
            X = scores(m, 50, torch.float32).cpu().numpy()
            for k in (int(v) for v in a.clusters.split(",")):
                KMeans(n_clusters=k, init=X[:k], n_init=1, algorithm="lloyd", max_iter=1, tol=0.0).fit(X)   # (thread pool, caches)
                t, n = [], []
                for iters in (ITER_LO, ITER_HI):
                    t0 = time.perf_counter()
                    km = KMeans(n_clusters=k, init=X[:k], n_init=1, algorithm="lloyd", max_iter=iters, tol=0.0).fit(X)
                    t.append(time.perf_counter() - t0)
                    n.append(km.n_iter_)
                what = (f"{(t[1] - t[0]) / (n[1] - n[0]) * 1e3:.2f} ms per iteration" if n[1] > n[0]
                        else f"converged after {n[1]} iterations: no difference to take")
                say(f"  scikit-learn Lloyd, CPU, {os.environ.get('OMP_NUM_THREADS', '?')} threads, f32, m = {m} k = {k:3d}: {what} "
                    f"(for orientation only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

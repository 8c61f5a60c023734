#!/usr/bin/env python3
"""What a t-SNE epoch costs (GPU): python tools/tsne_time.py [--rows 50000,200000] [--reps 3] [--sklearn] [--out F]

Device time from events on the stream the Session runs on, around whole calls (launches, gaps and the call's final
synchronisation included), best and median of `reps` after a warm-up.  Per m (d_out = 2, f32 and f64), on 50-column score-like
rows at perplexity 30:
  affinities   Session.knn + Session.tsne_affinities, once each (stages 1-3);
  epoch        (tsne_embed with 105 epochs - tsne_embed with 5 epochs) / 100: no host synchronisation lies inside the loop, and
               both calls carry the same set-up and final evaluation, so the difference holds epochs and nothing else;
  attraction   the same difference on P minus the same difference on an EMPTY affinity matrix: the same launches in both,
               only the attraction kernel's work differs (what is left in the empty run is its launch);
  repulsion    tsne_gradient on the empty matrix, one call: the all-pairs kernel, its Z sums, an attraction launch, and
               the call's read-back and synchronisation (a few hundredths of a ms: the resolution of the next line);
  update       the empty-matrix epoch minus that call (gains, velocity, step, re-centring: four launches).
Beside them the instruction-issue estimate of the f32 repulsion -- about 13 VALU slots per pair on 256 CUs x 4 SIMDs x 16 lanes
at 2.4 GHz -- which nobody had measured when it was written down, and, with --sklearn, for orientation only (a different
algorithm on a different processor, not a bound), scikit-learn's Barnes-Hut TSNE on the CPU at doubling m until a run takes
more than a minute: the largest m it finishes within one.
profiles/tsne_time.txt is this script's output."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
from sapca import ops  # noqa: E402

SLOTS_PER_PAIR, LANES, CLOCK = 13.0, 256 * 4 * 16, 2.4e9


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
    ap.add_argument("--rows", default="50000,200000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_time.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sess = ops.Session(stream=torch.cuda.current_stream().cuda_stream)
    say(f"t-SNE on score-like rows (d = 50, perplexity 30, output_dim 2), {torch.cuda.get_device_name(0)}; 1 warm-up + {a.reps} timed calls, ms (best / median)")
    for m in (int(x) for x in a.rows.split(",")):
        est = SLOTS_PER_PAIR * m * m / LANES / CLOCK * 1e3
        say(f"m = {m}: issue-slot estimate of the f32 repulsion (unmeasured when stated): {SLOTS_PER_PAIR:.0f} slots x m^2 / {LANES} lanes / 2.4 GHz = {est:.2f} ms")
        for dtype, name in ((torch.float32, "f32"), (torch.float64, "f64")):
            x = scores(m, 50, dtype)
            held = {}
            t_knn = timed(lambda: held.__setitem__("nn", sess.knn(x, None, 90)), a.reps)
            t_aff = timed(lambda: held.__setitem__("P", sess.tsne_affinities(*held["nn"], 30.0)[0]), a.reps)
            P = held["P"]
            y = (torch.randn((m, 2), device="cuda", dtype=torch.float64) * 10.0).to(dtype)
            empty = ops.ResidentCsr.from_torch(sess, torch.zeros(m + 1, dtype=torch.int64, device="cuda"),
                                               torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=dtype, device="cuda"), (m, m))
            t_rep = timed(lambda: sess.tsne_gradient(empty, y), a.reps)
            blocks = {}
            for name_, G in (("P", P), ("empty", empty)):
                t5 = timed(lambda: sess.tsne_embed(G, epochs=5, init=y), a.reps)
                t105 = timed(lambda: sess.tsne_embed(G, epochs=105, init=y), a.reps)
                blocks[name_] = tuple((hi - lo) / 100.0 for lo, hi in zip(t5, t105))
            epoch, bare = blocks["P"], blocks["empty"]
            say(f"  {name}: knn (90 neighbours) {t_knn[0]:9.2f} / {t_knn[1]:9.2f}   affinities ({P.nnz} entries) {t_aff[0]:8.2f} / {t_aff[1]:8.2f}")
            say(f"  {name}: epoch {epoch[0]:9.3f} / {epoch[1]:9.3f}   repulsion {t_rep[0]:9.3f} / {t_rep[1]:9.3f}   attraction {epoch[0] - bare[0]:8.3f} / "
                f"{epoch[1] - bare[1]:8.3f}   update {bare[0] - t_rep[0]:8.3f} / {bare[1] - t_rep[1]:8.3f}"
                + (f"   (repulsion = {t_rep[0] / est:.2f} x the estimate)" if name == "f32" else ""))
            del x, y, P, empty, held
    if a.sklearn:
        from sklearn.manifold import TSNE
        m, last = 12500, None
        while True:
            X = scores(m, 50, torch.float32).cpu().numpy()
            t0 = time.perf_counter()
            TSNE(perplexity=30.0, max_iter=250, method="barnes_hut", init="random", random_state=0).fit(X)
            dt = time.perf_counter() - t0
            say(f"  scikit-learn Barnes-Hut TSNE (theta 0.5), CPU, {os.environ.get('OMP_NUM_THREADS', '?')} threads, m = {m}, 250 iterations (its minimum), "
                f"neighbour search included: {dt:.1f} s wall = {dt / 250 * 1e3:.1f} ms per iteration")
            if dt > 60.0 or m >= 400000:
                break
            last, m = m, 2 * m
        say(f"for orientation only: the largest m of this doubling that scikit-learn finishes within a minute is {last}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

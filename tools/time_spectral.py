#!/usr/bin/env python3
"""What the spectral embedding costs on the neighbour graph (GPU): python tools/time_spectral.py [--rows 200000] [--noise 1.2]
[--reps 5] [--out F]

Two graphs, each the fuzzy union (n_neighbors 15) of 200 000 rows of 50 columns, f32 values:
  headline   the scores of the headline workload itself (bench.py's c2: the gapped 200 000 x 20 000 matrix, density 0.03, seed 42,
             SparsePCA fit_transform with k = 50, p = 10, q = 4, QR).  Expected, and to be read off the output, not assumed: its
             planted clusters are well separated, so its graph may fall into more components than pairs are asked for, and the
             solve then locks all of them without a step;
  noise v    synthetic score-like rows (tools/umap_time.py's generator with the spread of a cluster as a parameter: 1.2 makes the
             clusters overlap and the graph connected), which is where the iteration, its steps and its split can be measured.
Device time from events on the stream around whole calls (launches, gaps and read-backs included), 1 warm-up + `reps` timed calls, ms as best / median.
  components     Session.graph_components
  scale          Session.spectral_scale, both kinds
  operator       one application y = S x on the scaled f64 copy: (the stage call with SAPCA_SPECTRAL_APPLY_REPS = 101 - the same
                 with 1) / 100, so the scale and the copy of the stage call cancel; with the short-row kernel at its own packing
                 and at every forced one, and with the wave-per-row k::spmv (SAPCA_SPECTRAL_SPMV_ROW) on the same matrix.  These
                 switches exist in the debug variant of the library only; this script loads it.
  solve          Session.spectral for 16 pairs of each kind, at least 3 timed calls: steps (the sum over the rounds), the whole
                 call, the same with single_round = 1 (the first round alone: what the closing round costs), a step's mean
                 (whole / steps), and its split BY SUBTRACTION, not by a measurement inside the step: the operator is the figure
                 of the line above for the route the step takes (k::spmv), the rest is the re-orthogonalisation (four passes over
                 the basis) and the host's checks.  The same solve with the short-row kernel in the step
                 (SAPCA_SPECTRAL_STEP_SHORT).  The largest residual |S v - theta v| (f64 graph, device arithmetic)
                 beside its bound tol + 64 steps eps.
profiles/spectral_time.txt is this script's output."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sapca import _lib as L  # noqa: E402
from sapca import ops  # noqa: E402
from umap_time import timed  # noqa: E402


def scores(rows, d, dtype, noise, seed=0):
    """tools/umap_time.py's score-like rows with the spread of a cluster as a parameter"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = 10.0 / torch.arange(1, d + 1, device="cuda", dtype=torch.float64).sqrt()
    centres = torch.randn((40, d), generator=g, device="cuda", dtype=torch.float64) * scale
    which = torch.randint(0, 40, (rows,), generator=g, device="cuda")
    x = centres[which] + noise * scale * torch.randn((rows, d), generator=g, device="cuda", dtype=torch.float64)
    return x.to(dtype).contiguous()


def headline_scores(rows):
    """bench.py's c2 workload, fitted and projected: the score rows the neighbour graph of the headline run is made of"""
    import sapca
    from sapca import synth
    n, density, k, p, q = 20_000, 0.03, 50, 10, 4
    ptr, idx, val = synth.gapped_csr(rows, n, density, k, seed=42, dtype=torch.float32, device="cuda:0")
    pca = (sapca.SparsePCABuilder.new().n_components(k).random_seed(42)
           .svd_method(sapca.SVDMethod.Random(p, q, sapca.PowerIterationNormalizer.QR)).build())
    return pca.fit_transform(sapca.DeviceCsr(ptr, idx, val, (rows, n))).clone().contiguous()


def env(**kw):
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)


def per_application(sess, G, x, kind, reps):
    env(SAPCA_SPECTRAL_APPLY_REPS=1)
    one = timed(lambda: sess.spectral_apply(G, x, kind), reps)
    env(SAPCA_SPECTRAL_APPLY_REPS=101)
    many = timed(lambda: sess.spectral_apply(G, x, kind), reps)
    env(SAPCA_SPECTRAL_APPLY_REPS=None)
    return (many[0] - one[0]) / 100.0, (many[1] - one[1]) / 100.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--noise", default="1.2")
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-eigen", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L.load()
    L._lib = L.load_debug()     # the switches above are the debug variant's
    torch.cuda.set_device(0)
    m = args.rows
    eps = np.finfo(np.float64).eps
    lines = [f"spectral embedding of the fuzzy union (n_neighbors 15) of {m} score-like rows (d = 50, f32), {torch.cuda.get_device_name(0)}; "
             f"1 warm-up + {args.reps} timed calls, ms (best / median)"]
    panels = ([] if args.no_headline else ["headline"]) + [float(v) for v in args.noise.split(",") if v]
    for noise in panels:
        sess = ops.Session()
        try:
            X = headline_scores(m) if noise == "headline" else scores(m, 50, torch.float32, noise)
        except L.SapcaError as e:
            lines.append(f"{noise}: no panel: {e}")
            continue
        idx, dist = sess.knn(X, n_neighbors=14)
        G = sess.umap_graph(idx, dist, 15)[0]
        labels, ncomp = sess.graph_components(G)
        lines.append(f"{'the headline workload scores' if noise == 'headline' else f'noise {noise}'}: graph {G.nnz} entries ({G.nnz / m:.1f} per row), {ncomp} components")
        t = timed(lambda: sess.graph_components(G), args.reps)
        lines.append(f"  components            {t[0]:9.3f} / {t[1]:9.3f}")
        for kind in ("normalized", "diffmap"):
            t = timed(lambda: sess.spectral_scale(G, kind), args.reps)
            lines.append(f"  scale, {kind:<14} {t[0]:9.3f} / {t[1]:9.3f}")
        x = torch.randn((m,), device="cuda", dtype=torch.float64)
        env(SAPCA_SPECTRAL_SPMV_ROW=1, SAPCA_SPECTRAL_GROUP=None)
        row = per_application(sess, G, x, "normalized", args.reps)
        env(SAPCA_SPECTRAL_SPMV_ROW=None)
        lines.append(f"  operator, k::spmv (a wave per row)      {row[0]:9.4f} / {row[1]:9.4f}")
        own = per_application(sess, G, x, "normalized", args.reps)
        lines.append(f"  operator, short-row kernel (its packing){own[0]:9.4f} / {own[1]:9.4f}   ratio to k::spmv {own[1] / row[1]:.3f} (median)")
        for g in (8, 16, 32, 64):
            env(SAPCA_SPECTRAL_GROUP=g)
            t = per_application(sess, G, x, "normalized", args.reps)
            lines.append(f"  operator, groups of {g:<2} lanes            {t[0]:9.4f} / {t[1]:9.4f}")
        env(SAPCA_SPECTRAL_GROUP=None)
        print("\n".join(lines[-9:]), flush=True)
        for kind in ("normalized", "diffmap"):
            try:
                evals, evecs, nc, steps = sess.spectral(G, n_eigen=args.n_eigen, kind=kind)
            except L.SapcaError as e:
                lines.append(f"  solve, {kind}: {e}")
                print(lines[-1], flush=True)
                continue
            whole = timed(lambda: sess.spectral(G, n_eigen=args.n_eigen, kind=kind), max(3, args.reps))
            one_steps = sess.spectral(G, n_eigen=args.n_eigen, kind=kind, single_round=True)[3]
            one = timed(lambda: sess.spectral(G, n_eigen=args.n_eigen, kind=kind, single_round=True), max(3, args.reps))
            env(SAPCA_SPECTRAL_STEP_SHORT=1)
            whole_short = timed(lambda: sess.spectral(G, n_eigen=args.n_eigen, kind=kind), max(3, args.reps))
            env(SAPCA_SPECTRAL_STEP_SHORT=None)
            # residuals on the f64 graph with the library's own operator
            d = G.as_device_csr()
            G64 = ops.ResidentCsr.from_torch(sess, d.row_offsets, d.col_indices, d.values.to(torch.float64), G.shape)
            ev64, E64, _, st64 = sess.spectral(G64, n_eigen=args.n_eigen, kind=kind)
            worst = 0.0
            for i in range(args.n_eigen):
                v = E64[:, i].contiguous()
                r = sess.spectral_apply(G64, v, kind) - float(ev64[i]) * v
                worst = max(worst, float(torch.linalg.norm(r)))
            line = (f"  solve, {kind:<10} {args.n_eigen} pairs: {min(nc, args.n_eigen)} locked, {steps} steps, whole call {whole[0]:9.2f} / {whole[1]:9.2f}")
            if steps:
                step = whole[1] / steps
                line += (f"; a step {step:.4f} on average, by subtraction: operator (k::spmv) {row[1]:.4f} ({100 * row[1] / step:.1f} %), "
                         f"re-orthogonalisation and checks {step - row[1]:.4f}; with the short-row kernel in the step "
                         f"{whole_short[0]:9.2f} / {whole_short[1]:9.2f}")
                line += f"; single_round = 1 (no closing round): {one_steps} steps, {one[0]:9.2f} / {one[1]:9.2f}"
            line += f"; largest residual {worst:.3e}, bound {1e-8 + 64 * st64 * eps:.3e} ({st64} steps, f64)"
            lines.append(line)
            lines.append(f"      eigenvalues {np.array2string(evals, precision=6, max_line_width=200)}")
            print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()

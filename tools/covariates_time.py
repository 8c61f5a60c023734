"""What regressing out per-row covariates costs a randomized fit on the headline (C2) matrix, 200k x 20k f32, k = 50, p = 10,
q = 4: fit() without covariates, with a design of rank 4 (3 batches + 1 continuous + the intercept), with 16 design columns
(8 batches + 7 continuous + the intercept: rank 15, one-hot codes beside the intercept are collinear) and with a full basis of
16 columns (16 continuous, center(False)); per-stage device times (collect_timings) and the best, median and worst wall-clock
of the timed fits after warm-up.     python tools/covariates_time.py [steps] [warmup]      (profiles/covariates_time.txt)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
import numpy as np
import torch
import sapca
from sapca import synth
from sapca import _lib as L

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
m, n, density, k, p, q = 200_000, 20_000, 0.03, 50, 10, 4
ptr, idx, val = synth.gapped_csr(m, n, density, k, seed=42, dtype=torch.float32, device="cuda")
x = sapca.DeviceCsr(ptr, idx, val, (m, n))
rng = np.random.default_rng(0)


def design(batches, cont):
    cols = [np.eye(batches)[rng.integers(0, batches, m)]] if batches else []
    return np.hstack(cols + [rng.standard_normal((m, cont))])


STAGES = ("prepare_ms", "stats_ms", "spmm_ms", "spmmt_ms", "ortho_ms", "small_svd_ms", "fit_total_ms")
print(f"C2: {m} x {n}, {x.nnz} stored entries, f32, k {k} p {p} q {q}; {warmup} warm-up + {steps} timed fits each", flush=True)
for name, center, Z in (("no covariates", True, None), ("rank 4 (3 batches + 1 continuous + intercept)", True, design(3, 1)),
                        ("rank 15 (8 batches + 7 continuous + intercept: 16 design columns)", True, design(8, 7)),
                        ("rank 16 (16 continuous, center = 0)", False, design(0, 16)),
                        ("no covariates, center = 0", False, None)):
    est = (sapca.SparsePCABuilder.new().n_components(k).random_seed(42).center(center).collect_timings(True)
           .transform_semantics(L.TRANSFORM_CENTERED).svd_method(sapca.SVDMethod.Random(p, q, sapca.PowerIterationNormalizer.QR)).build())
    if Z is not None:
        est.set_covariates(Z)
    wall, stage = [], {}
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        est.fit(x)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        if it >= warmup:
            wall.append(dt)
            t = est.timings()
            for f in STAGES:
                stage.setdefault(f, []).append(getattr(t, f))
    t = est.timings()
    print(f"{name}: covariate rank {est.covariate_rank_}\n"
          f"  wall per fit: best {min(wall):.3f} ms, median {np.median(wall):.3f} ms, worst {max(wall):.3f} ms\n"
          "  device, median per fit: " + "  ".join(f"{f[:-3]} {np.median(stage[f]):.3f}" for f in STAGES) + "\n"
          f"  sweeps: A x{t.n_spmm} median {np.median(t.spmm_sweep_ms[:t.n_spmm]):.3f} ms, A^T x{t.n_spmmt} median {np.median(t.spmmt_sweep_ms[:t.n_spmmt]):.3f} ms,"
          f" kernel {t.sweep_kernel}", flush=True)

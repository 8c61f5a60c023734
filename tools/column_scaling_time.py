"""What implicit column scaling costs a randomized fit on the headline (C2) matrix, 200k x 20k f32, k = 50, p = 10, q = 4:
fit() without scaling, with unit-variance scaling, with explicit weights, and without scaling again (set and cleared);
per-stage device times (collect_timings) and the best, median and worst wall-clock of the timed fits after warm-up.
The row scalings and the A^T-side finishing passes are booked under ortho_ms.
    python tools/column_scaling_time.py [steps] [warmup]      (profiles/column_scaling_time.txt)"""
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
weights = 10.0 ** np.random.default_rng(0).uniform(-1, 1, n)

STAGES = ("prepare_ms", "stats_ms", "spmm_ms", "spmmt_ms", "ortho_ms", "small_svd_ms", "fit_total_ms")
print(f"C2: {m} x {n}, {x.nnz} stored entries, f32, k {k} p {p} q {q}; {warmup} warm-up + {steps} timed fits each", flush=True)
est = (sapca.SparsePCABuilder.new().n_components(k).random_seed(42).collect_timings(True)
       .transform_semantics(L.TRANSFORM_CENTERED).svd_method(sapca.SVDMethod.Random(p, q, sapca.PowerIterationNormalizer.QR)).build())
for name, scaling in (("no scaling", None), ("unit variance", "unit_variance"), ("explicit weights", weights),
                      ("no scaling (set, then cleared)", None)):
    est.set_column_scaling(scaling)
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
    d = est.column_scale_
    print(f"{name}: {'no factors' if d is None else f'{np.count_nonzero(d)} live columns of {d.size}'}, total variance {est.total_variance_():.6g}\n"
          f"  wall per fit: best {min(wall):.3f} ms, median {np.median(wall):.3f} ms, worst {max(wall):.3f} ms\n"
          "  device, median per fit: " + "  ".join(f"{f[:-3]} {np.median(stage[f]):.3f}" for f in STAGES) + "\n"
          f"  sweeps: A x{t.n_spmm} median {np.median(t.spmm_sweep_ms[:t.n_spmm]):.3f} ms, A^T x{t.n_spmmt} median {np.median(t.spmmt_sweep_ms[:t.n_spmmt]):.3f} ms,"
          f" kernel {t.sweep_kernel}", flush=True)

"""Timing of the per-batch statistics and top-n entry points on the C2 matrix (200,000 x 20,000 f32, 3 %: 1.2e8 stored
entries).  HIP events on the handle's stream around each call (the call ends with its results on the host), best of
`--reps`, beside the bytes one read of the matrix moves and the device's own copy rate (sapca_measure_copy_gbs).  Kernel
times and the transposition's share come from a rocprofv3 --kernel-trace --stats run of this script (tools/README.md).

    python tools/batch_stats_time.py [--reps 5] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "single-algebra_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sapca  # noqa: E402,F401
from sapca import ops, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_stats_time.py needs a GPU")
    m, n, density, k = 200_000, 20_000, 0.03, 50
    ptr, idx, val = synth.gapped_csr(m, n, density, k, seed=42, dtype=torch.float32, device="cuda")
    nnz = int(val.numel())
    stream = torch.cuda.current_stream()
    sess = ops.Session(stream=stream.cuda_stream)
    R = ops.ResidentCsr(sess, (m, n), nnz, np.float32, ptr.data_ptr(), idx.data_ptr(), val.data_ptr())
    est = sapca.SparsePCABuilder.new().build()
    copy_gbs = est.measure_copy_gbs(1 << 30, 5)           # read + write counted
    read_bytes = nnz * 8 + (m + 1) * 8                    # one read of the indices, values and row offsets
    read_ms = read_bytes / (copy_gbs * 1e9) * 1e3
    rng = np.random.default_rng(0)
    row_codes = {b: rng.integers(0, b, m).astype(np.int32) for b in (3, 16)}
    col_codes = {b: rng.integers(0, b, n).astype(np.int32) for b in (3, 16)}

    def timed(fn):
        best = float("inf")
        fn()   # warm-up: code objects, buffers
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return best

    cases = [
        ("batch_stats axis 0 (rows labelled; transposition + kernel), 3 codes", lambda: R.batch_stats(0, row_codes[3], 3)),
        ("batch_stats axis 0, 16 codes", lambda: R.batch_stats(0, row_codes[16], 16)),
        ("batch_stats axis 1 (columns labelled), 3 codes", lambda: R.batch_stats(1, col_codes[3], 3)),
        ("batch_stats axis 1, 16 codes", lambda: R.batch_stats(1, col_codes[16], 16)),
        ("stats COLUMN (transposition + one row pass; for scale)", lambda: R.stats(ops.COLUMN)),
        ("sum_row_n_top n = 50", lambda: R.sum_row_n_top(50)),
        ("sum_row_n_top n = 50, 100, 200, 500", lambda: R.sum_row_n_top([50, 100, 200, 500])),
    ]
    print(f"C2 resident matrix: {m} x {n}, {nnz} stored entries, f32; copy rate {copy_gbs:.0f} GB/s; "
          f"one read of the matrix {read_bytes / 1e9:.3f} GB = {read_ms:.3f} ms at that rate")
    out = {"m": m, "n": n, "nnz": nnz, "copy_gbs": copy_gbs, "read_bytes": read_bytes, "read_ms": read_ms, "calls": {}}
    for name, fn in cases:
        t = timed(fn)
        out["calls"][name] = t
        print(f"{name:62s} {t:8.3f} ms   one matrix read / call time = {read_ms / t:5.2f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""Timing of the masked statistics entry point (sapca_masked_stats_csr_device_*) on the C2 matrix (200,000 x 20,000 f32,
3 %: 1.2e8 stored entries), with 50 % and 100 % of the rows (COLUMN) or columns (ROW) kept, beside the existing
statistics call.  HIP events on the handle's stream around each call (the call ends with its results on the host), best
of `--reps`, beside the one-read roofline -- 8 B (index + value) per kept entry at the device's own copy rate
(sapca_measure_copy_gbs).  Kernel times come from a rocprofv3 --kernel-trace --stats run of this script (tools/README.md).

    python tools/masked_stats_time.py [--reps 5] [--json out.json]
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
        raise SystemExit("masked_stats_time.py needs a GPU")
    m, n, density, k = 200_000, 20_000, 0.03, 50
    ptr, idx, val = synth.gapped_csr(m, n, density, k, seed=42, dtype=torch.float32, device="cuda")
    nnz = int(val.numel())
    lens = np.diff(ptr.cpu().numpy())
    col_counts = np.bincount(idx.cpu().numpy(), minlength=n)
    stream = torch.cuda.current_stream()
    sess = ops.Session(stream=stream.cuda_stream)
    R = ops.ResidentCsr(sess, (m, n), nnz, np.float32, ptr.data_ptr(), idx.data_ptr(), val.data_ptr())
    est = sapca.SparsePCABuilder.new().build()
    copy_gbs = est.measure_copy_gbs(1 << 30, 5)           # read + write counted
    rng = np.random.default_rng(0)
    half_rows, half_cols = rng.random(m) < 0.5, rng.random(n) < 0.5

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

    # (name, call, stored entries it has to read)
    cases = [
        ("masked COLUMN, 50 % of rows kept", lambda: R.masked_stats(ops.COLUMN, half_rows), int(lens[half_rows].sum())),
        ("masked COLUMN, 100 % kept (all-true mask)", lambda: R.masked_stats(ops.COLUMN, np.ones(m, bool)), nnz),
        ("masked COLUMN, no mask (var_col_chunk)", lambda: R.masked_stats(ops.COLUMN), nnz),
        ("stats COLUMN (transposition + row pass; for scale)", lambda: R.stats(ops.COLUMN), nnz),
        ("masked ROW, 50 % of columns kept", lambda: R.masked_stats(ops.ROW, half_cols), int(col_counts[half_cols].sum())),
        ("masked ROW, 100 % kept (all-true mask)", lambda: R.masked_stats(ops.ROW, np.ones(n, bool)), nnz),
        ("masked ROW, no mask (var_row_chunk)", lambda: R.masked_stats(ops.ROW), nnz),
        ("stats ROW (for scale)", lambda: R.stats(ops.ROW), nnz),
    ]
    print(f"C2 resident matrix: {m} x {n}, {nnz} stored entries, f32; copy rate {copy_gbs:.0f} GB/s")
    out = {"m": m, "n": n, "nnz": nnz, "copy_gbs": copy_gbs, "calls": {}}
    for name, fn, kept in cases:
        t = timed(fn)
        read_ms = kept * 8 / (copy_gbs * 1e9) * 1e3
        out["calls"][name] = {"ms": t, "kept_entries": kept, "roofline_ms": read_ms}
        print(f"{name:52s} {t:8.3f} ms   kept {kept / 1e6:6.1f} M   one read {read_ms:6.3f} ms = {read_ms / t:5.2f} of the call")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""Timing of the row selection (sapca_select_rows_csr_device_*) on the C2 matrix (200,000 x 20,000 f32, 3 %: 1.2e8 stored
entries): a 10 % mask, a 50 % mask, all rows, and a random permutation of all rows.  HIP events on the handle's stream
around each call (the call ends with the selection complete), best of `--reps` after a warm-up.  Beside each time: the
algorithmic bytes 2 * (4 + sizeof T) * nnz_out + 8 * (3 * n_rows + 2) -- every output entry read and written once, and
three 8-byte words per row (its index, its source offset, its new offset) -- and the rate they give as a share of the
device's own copy rate (sapca_measure_copy_gbs, read + write counted) taken in the same run.

Then what a caller without the entry point does for the 50 % case, with nothing but Session.upload: slice the host matrix
(scipy), widen the slice's indices to the library's usize layout, upload the slice; wall-clock, each part on its own.

--compact also runs one masked fit with an all-true mask, whose preparation compacts the same matrix (compact_columns:
the existing kernel with the nearest job), so that a `rocprofv3 --kernel-trace --stats` run of this script shows both.

    python tools/select_rows_time.py [--reps 5] [--compact] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "single-algebra_amd", "python"))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

import sapca  # noqa: E402,F401
from sapca import ops, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("select_rows_time.py needs a GPU")
    m, n, density, k = 200_000, 20_000, 0.03, 50
    ptr, idx, val = synth.gapped_csr(m, n, density, k, seed=42, dtype=torch.float32, device="cuda")
    nnz = int(val.numel())
    h_ptr = ptr.cpu().numpy()
    lens = np.diff(h_ptr)
    stream = torch.cuda.current_stream()
    sess = ops.Session(stream=stream.cuda_stream)
    R = ops.ResidentCsr(sess, (m, n), nnz, np.float32, ptr.data_ptr(), idx.data_ptr(), val.data_ptr())
    est = sapca.SparsePCABuilder.new().build()
    copy_gbs = est.measure_copy_gbs(1 << 30, 5)           # read + write counted
    rng = np.random.default_rng(0)
    tenth, half = rng.random(m) < 0.1, rng.random(m) < 0.5

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
        ("10 % mask", ops._row_list(tenth, m)),
        ("50 % mask", ops._row_list(half, m)),
        ("all rows", np.arange(m, dtype=np.uint64)),
        ("random permutation of all rows", rng.permutation(m).astype(np.uint64)),
    ]
    print(f"C2 resident matrix: {m} x {n}, {nnz} stored entries, f32; copy rate {copy_gbs:.0f} GB/s")
    out = {"m": m, "n": n, "nnz": nnz, "copy_gbs": copy_gbs, "calls": {}}
    for name, rows in cases:
        t = timed(lambda: R.select_rows(rows))
        nnz_out = int(lens[rows.astype(np.int64)].sum())
        assert R.select_rows(rows).nnz == nnz_out
        nbytes = 2 * (4 + 4) * nnz_out + 8 * (3 * rows.size + 2)
        gbs = nbytes / (t * 1e-3) / 1e9
        out["calls"][name] = {"ms": t, "n_rows": int(rows.size), "nnz_out": nnz_out, "bytes": nbytes, "gbs": gbs, "share_of_copy": gbs / copy_gbs}
        print(f"select_rows, {name:32s} {t:8.3f} ms   {rows.size:7d} rows {nnz_out / 1e6:6.1f} M entries   {nbytes / 1e9:6.3f} GB"
              f"   {gbs:7.0f} GB/s = {gbs / copy_gbs:5.2f} of the copy rate")

    # the 50 % case without the entry point: slice on the host, widen the indices, upload the slice
    A = sp.csr_matrix((val.cpu().numpy(), idx.cpu().numpy(), h_ptr), shape=(m, n))
    t0 = time.perf_counter()
    S = A[half]
    t1 = time.perf_counter()
    s_ptr, s_idx, s_val = ops.as_u64(S.indptr), ops.as_u64(S.indices), np.ascontiguousarray(S.data)
    t2 = time.perf_counter()
    host = ops.Session()
    best_up = float("inf")
    for _ in range(1 + max(1, a.reps // 2)):              # (the first upload allocates: best of the rest and it)
        torch.cuda.synchronize()
        u0 = time.perf_counter()
        U = host.upload(s_ptr, s_idx, s_val, S.shape[0], n)
        best_up = min(best_up, (time.perf_counter() - u0) * 1e3)
    assert U.nnz == out["calls"]["50 % mask"]["nnz_out"]
    sel = out["calls"]["50 % mask"]["ms"]
    out["host_path_50"] = {"slice_ms": (t1 - t0) * 1e3, "widen_ms": (t2 - t1) * 1e3, "upload_ms": best_up}
    print(f"host path, 50 % mask: scipy slice {(t1 - t0) * 1e3:8.1f} ms, indices to usize {(t2 - t1) * 1e3:8.1f} ms, "
          f"Session.upload of the slice {best_up:8.1f} ms (wall-clock)   upload alone / select_rows = {best_up / sel:6.1f}")

    if a.compact:
        from sapca import PowerIterationNormalizer as PIN
        from sapca import SVDMethod
        mk = (sapca.MaskedSparsePCABuilder.new().n_components(8).mask(np.ones(n, bool))
              .svd_method(SVDMethod.Random(4, 0, PIN.QR)).build())
        mk.fit(sapca.DeviceCsr(ptr, idx, val, (m, n)))
        torch.cuda.synchronize()
        print("ran one masked fit with an all-true mask (its preparation compacts the matrix: write_kept_kernel in a kernel trace)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

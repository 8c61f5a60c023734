"""Timing of the row-and-column selection (sapca_select_submatrix_csr_device_*) on the C2 matrix (200,000 x 20,000 f32,
3 %: 1.2e8 stored entries).  HIP events on the handle's stream around each call (the call ends with the selection
complete), one warm-up and `--reps` timed calls: best / median / worst.

The yardstick is sapca_select_rows_csr_device_* of all rows in the same run, and the device's own copy rate
(sapca_measure_copy_gbs, read + write counted).  Then the new call: identity; all rows x a 50 % random column mask; all rows
x a 10 % mask; a 50 % row mask x a 10 % column mask; all rows and columns without stored zeros.  Beside each time the
algorithmic bytes: per gathered entry 4 (the count pass reads its column; + sizeof T under the flag) + 4 + sizeof T (the
fill reads it), per kept entry 4 + sizeof T written, and three 8-byte words per row; identity and the yardstick move
2 * (4 + sizeof T) per entry.

Then the host route for the 50 % x 10 % case, wall-clock, each part on its own: device -> host copy of the matrix, scipy
slice, indices to the library's usize layout, Session.upload of the slice.  Last, sapca_timings.prepare_ms of one
randomized fit with the 10 % mask set on the source (sapca_set_mask: the preparation compacts the columns) beside the same
fit on the column-selected matrix.

Two conditions on the medians: identity <= 1.1 x the yardstick, all rows x 50 % mask <= 1.5 x the yardstick; the tool
prints whether each holds and exits 1 if one does not (--no-gate: report only).

    python tools/select_submatrix_time.py [--reps 7] [--no-gate] [--no-fits] [--json out.json]
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
from sapca import PowerIterationNormalizer as PIN  # noqa: E402
from sapca import SVDMethod  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-gate", action="store_true")
    ap.add_argument("--no-fits", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("select_submatrix_time.py needs a GPU")
    m, n, density, k = 200_000, 20_000, 0.03, 50
    ptr, idx, val = synth.gapped_csr(m, n, density, k, seed=42, dtype=torch.float32, device="cuda")
    nnz = int(val.numel())
    h_ptr, h_idx, h_val = ptr.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy()
    lens = np.diff(h_ptr)
    stream = torch.cuda.current_stream()
    sess = ops.Session(stream=stream.cuda_stream)
    R = ops.ResidentCsr(sess, (m, n), nnz, np.float32, ptr.data_ptr(), idx.data_ptr(), val.data_ptr())
    copy_gbs = sapca.SparsePCABuilder.new().build().measure_copy_gbs(1 << 30, 5)   # read + write counted
    rng = np.random.default_rng(0)
    rows_half = rng.random(m) < 0.5
    cols_half, cols_tenth = rng.random(n) < 0.5, rng.random(n) < 0.1
    all_rows = np.arange(m, dtype=np.uint64)

    def timed(fn):
        fn()   # warm-up: code objects, buffers
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return {"best_ms": ts[0], "median_ms": ts[len(ts) // 2], "worst_ms": ts[-1]}

    def kept_in(rows_mask, cols_mask):
        """(gathered entries, kept entries) of A[rows][:, cols] from the host copy"""
        sel = np.ones(nnz, bool) if rows_mask is None else np.repeat(rows_mask, lens)
        gathered = int(sel.sum())
        if cols_mask is not None:
            sel &= cols_mask[h_idx]
        return gathered, int(sel.sum())

    print(f"C2 resident matrix: {m} x {n}, {nnz} stored entries, f32; copy rate {copy_gbs:.0f} GB/s; {a.reps} timed calls after a warm-up")
    out = {"m": m, "n": n, "nnz": nnz, "copy_gbs": copy_gbs, "reps": a.reps, "calls": {}}

    def report(name, t, n_rows, gathered, kept, nbytes):
        gbs = nbytes / (t["median_ms"] * 1e-3) / 1e9
        out["calls"][name] = dict(t, n_rows=n_rows, gathered=gathered, nnz_out=kept, bytes=nbytes, gbs=gbs, share_of_copy=gbs / copy_gbs)
        print(f"{name:44s} {t['best_ms']:7.3f} / {t['median_ms']:7.3f} / {t['worst_ms']:7.3f} ms   {kept / 1e6:6.1f} M of {gathered / 1e6:6.1f} M entries"
              f"   {nbytes / 1e9:6.3f} GB   {gbs:6.0f} GB/s = {gbs / copy_gbs:4.2f} of the copy rate")

    t = timed(lambda: R.select_rows(all_rows))
    report("select_rows, all rows (the yardstick)", t, m, nnz, nnz, 2 * 8 * nnz + 8 * (3 * m + 2))
    yard = t["median_ms"]
    cases = [
        ("select, identity", None, None, False),
        ("select, all rows x 50 % column mask", None, cols_half, False),
        ("select, all rows x 10 % column mask", None, cols_tenth, False),
        ("select, 50 % row mask x 10 % column mask", rows_half, cols_tenth, False),
        ("select, all rows and columns, no stored zeros", None, None, True),
    ]
    zeros = int((h_val == 0).sum())
    for name, rmask, cmask, drop in cases:
        t = timed(lambda: R.select(rmask, cmask, drop_stored_zeros=drop))
        gathered, kept = kept_in(rmask, cmask)
        if drop:
            kept -= zeros
        S = R.select(rmask, cmask, drop_stored_zeros=drop)
        assert S.nnz == kept and S.shape == (m if rmask is None else int(rmask.sum()), n if cmask is None else int(cmask.sum()))
        if cmask is None and not drop:
            nbytes = 2 * 8 * kept + 8 * (3 * S.shape[0] + 2)
        else:
            nbytes = (4 + (4 if drop else 0) + 8) * gathered + 8 * kept + 8 * (3 * S.shape[0] + 2)
        report(name, t, S.shape[0], gathered, kept, nbytes)
    ident = out["calls"]["select, identity"]["median_ms"]
    half = out["calls"]["select, all rows x 50 % column mask"]["median_ms"]
    gates = {"identity <= 1.1 x select_rows of all rows": (ident, 1.1 * yard),
             "all rows x 50 % mask <= 1.5 x select_rows of all rows": (half, 1.5 * yard)}
    out["gates"] = {}
    for what, (got, bar) in gates.items():
        ok = got <= bar
        out["gates"][what] = {"median_ms": got, "bar_ms": bar, "ratio": got / yard, "holds": bool(ok)}
        print(f"{what}: {got:.3f} ms against {bar:.3f} ms (ratio {got / yard:.2f}): {'holds' if ok else 'MISSED'}")

    # the 50 % x 10 % case without the entry point
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    A = sp.csr_matrix((val.cpu().numpy(), idx.cpu().numpy(), ptr.cpu().numpy()), shape=(m, n))
    t1 = time.perf_counter()
    S = A[rows_half][:, np.flatnonzero(cols_tenth)]
    t2 = time.perf_counter()
    s_ptr, s_idx, s_val = ops.as_u64(S.indptr), ops.as_u64(S.indices), np.ascontiguousarray(S.data)
    t3 = time.perf_counter()
    host = ops.Session()
    torch.cuda.synchronize()
    host.upload(s_ptr, s_idx, s_val, S.shape[0], S.shape[1])                      # (the first upload allocates)
    torch.cuda.synchronize()
    u0 = time.perf_counter()
    U = host.upload(s_ptr, s_idx, s_val, S.shape[0], S.shape[1])
    up = (time.perf_counter() - u0) * 1e3
    sel = out["calls"]["select, 50 % row mask x 10 % column mask"]
    assert U.nnz == sel["nnz_out"]
    out["host_path_50x10"] = {"to_host_ms": (t1 - t0) * 1e3, "slice_ms": (t2 - t1) * 1e3, "widen_ms": (t3 - t2) * 1e3, "upload_ms": up}
    print(f"host route, 50 % x 10 %: device -> host {(t1 - t0) * 1e3:8.1f} ms, scipy slice {(t2 - t1) * 1e3:8.1f} ms, indices to usize "
          f"{(t3 - t2) * 1e3:8.1f} ms, Session.upload of the slice {up:8.1f} ms (wall-clock); select takes {sel['median_ms']:.3f} ms")

    if not a.no_fits:
        # the preparation of a masked fit compacts the columns every time; a fit of the column-selected matrix does not
        def fitted(builder, x):
            est = builder.n_components(8).svd_method(SVDMethod.Random(4, 1, PIN.QR)).collect_timings().build()
            est.fit(x)                                                            # (the first fit allocates)
            est.fit(x)
            return est.timings().prepare_ms
        masked = fitted(sapca.MaskedSparsePCABuilder.new().mask(cols_tenth), sapca.DeviceCsr(ptr, idx, val, (m, n)))
        SC = R.select_cols(cols_tenth)
        plain = fitted(sapca.SparsePCABuilder.new(), SC.as_device_csr())
        out["prepare_ms"] = {"masked_fit_of_the_source": masked, "fit_of_the_column_selection": plain}
        print(f"prepare_ms of a randomized fit (k = 8, 10 % of the columns): sapca_set_mask on the source {masked:8.2f} ms, "
              f"on select_cols' result {plain:8.2f} ms")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if not a.no_gate and not all(g["holds"] for g in out["gates"].values()):
        raise SystemExit(1)


if __name__ == "__main__":
    main()

"""Timing of the check / canonicalise gate (sapca_check_csr_device_*, sapca_canonicalize_csr_device_*) on the C2-shaped
matrix (200,000 x 20,000 f32, 3 %: 1.2e8 stored entries), adopted from torch tensors (ResidentCsr.from_torch):

    the check;  canonicalize of a canonical matrix;  canonicalize with 1 % and with 100 % of the rows shuffled;
    canonicalize with 1 % duplicated entries (sorted rows, the copies next to their originals).

HIP events on the handle's stream around each call (every call ends complete), `--reps` timed calls after a warm-up;
printed: best, median and worst (the spread).  Two yardsticks beside them: the identity select_rows of the same matrix
(it reads and writes exactly the bytes a full copy does), and the host route the gate replaces -- device -> host copy,
scipy's sorted_indices() and sum_duplicates(), Session.upload -- wall-clock, once, on the fully shuffled matrix.

    python tools/canonical_time.py [--reps 7] [--no-host] [--out profiles/canonical_time.txt] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "single-algebra_amd", "python"))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

import sapca  # noqa: E402,F401
from sapca import ops, synth  # noqa: E402


def shuffled_rows(ptr, idx, val, share, seed):
    """the entries of a `share` of the rows in random order inside their row (on the device)"""
    g = torch.Generator(device=idx.device).manual_seed(seed)
    m, nnz = ptr.numel() - 1, idx.numel()
    lens = ptr[1:] - ptr[:-1]
    row = torch.repeat_interleave(torch.arange(m, device=idx.device), lens)
    pos = torch.arange(nnz, device=idx.device) - ptr[:-1][row]
    pick = torch.rand(m, device=idx.device, generator=g) < share
    key = torch.where(pick[row], torch.rand(nnz, device=idx.device, generator=g, dtype=torch.float64),
                      pos.double() / lens[row].double())
    order = torch.argsort(row.double() + key)
    return idx[order].contiguous(), val[order].contiguous(), int(pick.sum())


def duplicated_entries(ptr, idx, val, share, seed, n):
    """a `share` of the entries stored twice (half the value each), rows still sorted"""
    g = torch.Generator(device=idx.device).manual_seed(seed)
    m, nnz = ptr.numel() - 1, idx.numel()
    row = torch.repeat_interleave(torch.arange(m, device=idx.device), ptr[1:] - ptr[:-1])
    twice = torch.rand(nnz, device=idx.device, generator=g) < share
    v = torch.where(twice, val * 0.5, val)
    row2, idx2, val2 = torch.cat([row, row[twice]]), torch.cat([idx, idx[twice]]), torch.cat([v, v[twice]])
    order = torch.argsort(row2 * n + idx2.long(), stable=True)
    ptr2 = torch.zeros(m + 1, dtype=torch.int64, device=idx.device)
    ptr2[1:] = torch.cumsum(torch.bincount(row2, minlength=m), 0)
    return ptr2, idx2[order].contiguous(), val2[order].contiguous(), int(twice.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rows", type=int, default=200_000)   # (a smaller matrix for a rehearsal)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("canonical_time.py needs a GPU")
    m, n, density, k = a.rows, 20_000, 0.03, 50
    ptr, idx, val = synth.gapped_csr(m, n, density, k, seed=42, dtype=torch.float32, device="cuda")
    idx = idx.to(torch.int32)
    nnz = int(val.numel())
    stream = torch.cuda.current_stream()
    sess = ops.Session(stream=stream.cuda_stream)
    est = sapca.SparsePCABuilder.new().build()
    copy_gbs = est.measure_copy_gbs(1 << 30, 5)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

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
        return {"best": min(ts), "median": statistics.median(ts), "worst": max(ts)}

    def row(name, t, note=""):
        say(f"{name:52s} {t['best']:9.3f} {t['median']:9.3f} {t['worst']:9.3f} ms   {note}")

    out = {"m": m, "n": n, "nnz": nnz, "copy_gbs": copy_gbs, "reps": a.reps, "calls": {}}
    say(f"C2-shaped matrix: {m} x {n}, {nnz} stored entries, f32; copy rate {copy_gbs:.0f} GB/s (read + write); {a.reps} timed calls each")
    say(f"{'':52s} {'best':>9s} {'median':>9s} {'worst':>9s}")
    X = ops.ResidentCsr.from_torch(sess, ptr, idx, val, (m, n))
    read_gb = (8 * nnz + 8 * (m + 1)) / 1e9
    t = out["calls"]["check"] = timed(X.check)
    assert X.check().canonical
    row("check", t, f"{read_gb:.3f} GB read: {read_gb / (t['best'] * 1e-3):.0f} GB/s")
    t = out["calls"]["canonicalize, canonical input"] = timed(X.canonicalize)
    assert X.canonicalize()[0] is X
    row("canonicalize, canonical input", t)
    t = out["calls"]["select_rows, all rows (identity)"] = timed(lambda: X.select_rows(np.arange(m, dtype=np.uint64)))
    row("select_rows, all rows (identity: a full copy)", t, f"{2 * read_gb:.3f} GB moved: {2 * read_gb / (t['best'] * 1e-3):.0f} GB/s")
    ident = t
    shuffled_all = None
    for share in (0.01, 1.0):
        sidx, sval, picked = shuffled_rows(ptr, idx, val, share, 7)
        S = ops.ResidentCsr.from_torch(sess, ptr, sidx, sval, (m, n))
        name = f"canonicalize, {share:.0%} of the rows shuffled"
        t = out["calls"][name] = timed(S.canonicalize)
        Cn, rep = S.canonicalize()
        d = Cn.as_device_csr()
        assert torch.equal(d.col_indices, idx) and torch.equal(d.values, val) and rep.duplicate_entries == 0
        row(name, t, f"{rep.unsorted_rows} unsorted rows of {picked} picked; result equals the original")
        if share == 1.0:
            shuffled_all = (sidx, sval)
        del S, Cn, d
    dptr, didx, dval, twice = duplicated_entries(ptr, idx, val, 0.01, 9, n)
    D = ops.ResidentCsr.from_torch(sess, dptr, didx, dval, (m, n))
    t = out["calls"]["canonicalize, 1 % duplicated entries"] = timed(D.canonicalize)
    Cn, rep = D.canonicalize()
    d = Cn.as_device_csr()
    assert rep.duplicate_entries == twice and Cn.nnz == nnz and torch.equal(d.col_indices, idx) and torch.equal(d.values, val)
    row("canonicalize, 1 % duplicated entries", t, f"{twice} entries merged; result equals the original")
    chk = out["calls"]["check"]
    say(f"check / identity selection = {chk['best'] / ident['best']:.2f}; canonical input / identity selection = "
        f"{out['calls']['canonicalize, canonical input']['best'] / ident['best']:.2f}; 1 % shuffled / (identity selection + check) = "
        f"{out['calls']['canonicalize, 1% of the rows shuffled']['best'] / (ident['best'] + chk['best']):.2f}")
    del D, Cn, d, dptr, didx, dval

    if not a.no_host:   # the route the gate replaces, on the fully shuffled matrix, once
        sidx, sval = shuffled_all
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        A = sp.csr_matrix((sval.cpu().numpy(), sidx.cpu().numpy(), ptr.cpu().numpy()), shape=(m, n))
        t1 = time.perf_counter()
        A.has_sorted_indices = False
        A = A.sorted_indices()
        A.sum_duplicates()
        t2 = time.perf_counter()
        host = ops.Session()
        U = host.upload(A.indptr, A.indices, A.data, m, n)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        assert U.nnz == nnz
        out["host_route"] = {"download_ms": (t1 - t0) * 1e3, "scipy_ms": (t2 - t1) * 1e3, "upload_ms": (t3 - t2) * 1e3}
        say(f"host route, 100 % shuffled: device -> host {(t1 - t0) * 1e3:.0f} ms, scipy sorted_indices + sum_duplicates {(t2 - t1) * 1e3:.0f} ms, "
            f"Session.upload {(t3 - t2) * 1e3:.0f} ms (wall-clock, once; the first upload allocates)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

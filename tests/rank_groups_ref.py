"""Host restatement of the rank-groups operator (include/sapca.h, "Rank groups"; sapca_rank_sums_csr_device_* and
sapca_rank_groups_csr_device_*) in numpy, with the sparse formulas of the header: the stored non-zero values of the included
rows are ranked, the zeros (stored or implicit) enter as one block, rows whose label is outside [0, K) are left out.  Needs
neither a GPU nor the library; tests/test_rank_groups_cpu.py holds it to scipy's rankdata, mannwhitneyu and ttest_ind."""
import math

import numpy as np

# the length classes of the rank pass (csrc/rankgroups.h), hard-coded for the shapes of tests/test_gpu_rank_groups.py; the CPU
# test reads the header and holds these to it
WAVE_MAX = 256        # kRankWaveMax: a stored column up to this long is sorted by one wave
LDS_MAX = 4096        # kRankLdsMax: up to this long by one workgroup in LDS; longer: segmented radix sort in global scratch
WALK_CHUNK = 256      # kRankWalkChunk: positions a workgroup takes per step of the long class's walk
MAX_GROUPS = 1024     # SAPCA_RANK_MAX_GROUPS; also the codes of one launch of the labelled statistics

EPS = float(np.finfo(np.float64).eps)


def _columns(ptr, idx, val, m, n):
    """(rows, values) of every column, rows ascending: the CSR read column-wise"""
    ptr = np.asarray(ptr, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
    order = np.argsort(idx, kind="stable")
    bounds = np.searchsorted(idx[order], np.arange(n + 1))
    return [(rows[order[bounds[j]:bounds[j + 1]]], val[order[bounds[j]:bounds[j + 1]]]) for j in range(n)]


def rank_sums(ptr, idx, val, m, n, labels, K):
    """{"group_rows": K, "rank_sum2": K x n int64, "nonzero": K x n, "tie_sum": n float64 (an exact integer while below 2^53)}"""
    labels = np.asarray(labels, dtype=np.int64)
    inc = (labels >= 0) & (labels < K)
    group = np.bincount(labels[inc], minlength=K).astype(np.int64)
    M = int(group.sum())
    rs2 = np.zeros((K, n), dtype=np.int64)
    nz = np.zeros((K, n), dtype=np.int64)
    tie = np.zeros(n)
    for j, (r, v) in enumerate(_columns(ptr, idx, val, m, n)):
        keep = inc[r] & (v != 0)
        v, g = v[keep], labels[r[keep]]
        L = v.size
        a = int((v < 0).sum())
        Z = M - L
        if L == 0:                                       # every included row is in the zero block
            rs2[:, j] = group * (1 + Z)
            tie[j] = float(Z ** 3 - Z)
            continue
        order = np.argsort(v, kind="stable")
        sv, g = v[order], g[order]
        start = np.ones(L, dtype=bool)
        start[1:] = sv[1:] != sv[:-1]
        run = np.cumsum(start) - 1                       # the tie run of every sorted position
        first = np.flatnonzero(start)
        last = np.append(first[1:], L) - 1
        pos = np.arange(L, dtype=np.int64) + 1
        pos[a:] += Z                                     # ranks behind the zero block
        np.add.at(rs2[:, j], g, pos[first[run]] + pos[last[run]])
        np.add.at(nz[:, j], g, 1)
        rs2[:, j] += (group - nz[:, j]) * ((a + 1) + (a + Z))
        t = [int(x) for x in (last - first + 1)] + [Z]
        tie[j] = float(sum(x ** 3 - x for x in t))
    return {"group_rows": group, "rank_sum2": rs2, "nonzero": nz, "tie_sum": tie}


def wilcoxon(rank_sum2, group_rows, tie_sum, tie_correct):
    """(z, p) of the header's formula from the exact quantities (the library's own, or rank_sums' above)"""
    group = np.asarray(group_rows, dtype=np.int64)
    K, n = rank_sum2.shape
    M = int(group.sum())
    z = np.zeros((K, n))
    p = np.ones((K, n))
    for g in range(K):
        ng, nr = int(group[g]), M - int(group[g])
        if ng == 0 or nr == 0:
            continue
        for j in range(n):
            T = 1.0 - tie_sum[j] / (float(M) * float(M) * float(M) - float(M)) if tie_correct else 1.0
            sd = math.sqrt(float(ng) * float(nr) * float(M + 1) / 12.0 * T)
            if sd > 0.0:
                z[g, j] = 0.5 * float(int(rank_sum2[g, j]) - ng * (M + 1)) / sd
                p[g, j] = math.erfc(abs(z[g, j]) / math.sqrt(2.0))
    return z, p


def moments(ptr, idx, val, m, n, labels, K):
    """(s, q): K x n sums and sums of squares of each group's stored entries, in f64"""
    labels = np.asarray(labels, dtype=np.int64)
    inc = (labels >= 0) & (labels < K)
    s = np.zeros((K, n))
    q = np.zeros((K, n))
    for j, (r, v) in enumerate(_columns(ptr, idx, val, m, n)):
        v = v[inc[r]].astype(np.float64)
        g = labels[r[inc[r]]]
        np.add.at(s[:, j], g, v)
        np.add.at(q[:, j], g, v * v)
    return s, q


def _sample_var(s, q, k):
    if k < 2:
        return np.zeros_like(s)
    return np.maximum(0.0, (q - s * s / k) / (k - 1))


def welch(s, q, group_rows):
    """{"mean", "var", "t", "df"}: K x n, the header's formulas from the group sums"""
    group = np.asarray(group_rows, dtype=np.int64)
    K, n = s.shape
    M = int(group.sum())
    s_tot, q_tot = np.zeros(n), np.zeros(n)
    for g in range(K):   # the totals: over g = 0 .. K - 1 in that order
        s_tot += s[g]
        q_tot += q[g]
    out = {k: np.zeros((K, n)) for k in ("mean", "var", "t", "df")}
    for g in range(K):
        ng, nr = int(group[g]), M - int(group[g])
        if ng:
            out["mean"][g] = s[g] / ng
        out["var"][g] = _sample_var(s[g], q[g], ng)
        if ng == 0 or nr == 0:
            continue
        sr, qr = s_tot - s[g], q_tot - q[g]
        out["t"][g], out["df"][g] = welch_pair(out["mean"][g], out["var"][g], ng, sr / nr, _sample_var(sr, qr, nr), nr)
    return out


def welch_pair(mean_g, var_g, ng, mean_r, var_r, nr):
    """(t, df) of two samples from their means, variances and sizes (arrays over the columns)"""
    vg, vr = var_g / ng, var_r / nr
    sd = np.sqrt(vg + vr)
    ok = sd > 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(ok, (mean_g - mean_r) / sd, 0.0)
        if ng >= 2 and nr >= 2:
            df = np.where(ok, (vg + vr) * (vg + vr) / (vg * vg / (ng - 1) + vr * vr / (nr - 1)), 0.0)
        else:
            df = np.zeros_like(t)
    return t, df


def rank_groups(ptr, idx, val, m, n, labels, K, tie_correct=False):
    """everything sapca_rank_groups_csr_device_* returns, by the names of its arguments"""
    r = rank_sums(ptr, idx, val, m, n, labels, K)
    z, p = wilcoxon(r["rank_sum2"], r["group_rows"], r["tie_sum"], tie_correct)
    w = welch(*moments(ptr, idx, val, m, n, labels, K), r["group_rows"])
    return {"group_rows": r["group_rows"], "mean": w["mean"], "var": w["var"], "nonzero": r["nonzero"], "t_score": w["t"],
            "t_df": w["df"], "z_score": z, "z_pvalue": p}


def names(scores, n_top=None):
    """per group the column indices by descending score, ties to the lower index"""
    order = np.argsort(-scores, axis=1, kind="stable")
    return order if n_top is None else order[:, :n_top]


def fixture(m, n, K, seed, dtype, kind="counts", density=0.3):
    """A labelled CSR with what the edge rules name: (ptr, idx, val, labels).  kind "counts": small integers with heavy ties;
    "real": real values, negatives among them.  Both carry stored zeros and -0.0, an all-zero column (0), a column stored in
    every row (1), an all-distinct column (2, when n > 2), an empty group (K - 1 when K > 2) and rows labelled -1 and K."""
    rng = np.random.default_rng(seed)
    if kind == "counts":
        D = (rng.random((m, n)) < density) * rng.integers(1, 5, (m, n)).astype(np.float64)
    else:
        D = (rng.random((m, n)) < density) * rng.normal(0.3, 2.0, (m, n))
    stored = D != 0
    stored |= rng.random((m, n)) < 0.02                  # stored zeros
    D[:, 0] = 0.0
    stored[:, 0] = False
    if n > 1:
        D[:, 1] = rng.integers(1, 4, m) if kind == "counts" else rng.normal(0.0, 1.0, m)
        stored[:, 1] = True
    if n > 2:
        D[:, 2] = rng.permutation(m) - m // 3            # all distinct, negatives, one zero
        stored[:, 2] = True
    r, c = np.nonzero(stored)
    val = D[r, c].astype(dtype)
    neg0 = (val == 0) & (rng.random(val.size) < 0.5)
    val[neg0] = -0.0
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int64)
    labels = rng.integers(0, max(K - 1, 1) if K > 2 else K, m).astype(np.int32)
    out = rng.random(m) < 0.05
    labels[out] = np.where(rng.random(int(out.sum())) < 0.5, -1, K)
    return ptr, c.astype(np.int64), val, labels

"""Host restatement of the variable-genes operators (include/sapca.h, "Variable genes": sapca_hvg_moments_csr_device_*,
sapca_loess_f64, sapca_hvg_csr_device_*) in numpy, with the formulas of the header.  Needs neither a GPU nor the library;
tests/test_hvg_cpu.py holds it to independent code: pandas.cut for the bins, numpy.polyfit for the local regression, a dense
two-line version for the clipped variance, and a hand-made table for the rank combination.

`reverse=True` sums every column and every loess window in the opposite order: the spread between the two runs is the
rounding freedom of the statement itself, and the GPU tests derive their bounds from it."""
import warnings

import numpy as np

CLIP, EXPM1 = 0, 1
SEURAT_V3, SEURAT = 0, 1
MAX_BATCHES = 1024    # SAPCA_HVG_MAX_BATCHES


# ---- fixtures -------------------------------------------------------------------------------------------------------------
def fixture(m, n, seed, dtype=np.float32):
    """(ptr, idx, val) of negative-binomial counts, about 35 % stored, with what the operators have to survive:
    six planted outlier cells (so that the clip has something to clip), five never-stored columns, one constant column,
    an empty row, stored zeros, two identical columns with a high mean and one column with a very high mean (the seurat
    flavour's zero-std bin and one-gene bin)."""
    rng = np.random.default_rng(seed)
    mu = np.exp(rng.uniform(np.log(0.05), np.log(4.0), n))
    r = 1.0
    lam = rng.gamma(r, mu[None, :] / r, size=(m, n))
    X = rng.poisson(lam).astype(np.int64)
    cells = rng.choice(m, 6, replace=False)
    genes = rng.choice(n, n // 5, replace=False)
    for c in cells:                                       # outlier cells: hundreds of counts in a fifth of the genes
        g = rng.choice(genes, genes.size // 2, replace=False)
        X[c, g] += rng.integers(150, 400, g.size)
    never = np.arange(7, 7 + 5 * 11, 11)                  # never stored
    X[:, never] = 0
    const = 3
    X[:, const] = 3                                       # constant, stored in every row
    X[:, n - 2] = rng.poisson(rng.gamma(4.0, 25.0 / 4.0, m))
    X[:, n - 3] = X[:, n - 2]                             # identical columns
    X[:, n - 1] = rng.poisson(rng.gamma(4.0, 60.0, m))    # alone at the top of the mean range
    stored = X > 0
    stored |= (rng.random((m, n)) < 0.01) & ~np.isin(np.arange(n), never)[None, :]   # stored zeros
    empty_row = m // 3
    stored[empty_row, :] = False
    X[empty_row, :] = 0
    ptr = np.concatenate([[0], np.cumsum(stored.sum(axis=1))]).astype(np.int64)
    rows, idx = np.nonzero(stored)
    val = X[rows, idx].astype(dtype)
    return ptr, idx.astype(np.int32), val


def batch_labels(m, K, seed):
    """int32 labels in [0, K) with a twentieth of the rows excluded, by -1 and by K .. K + 2"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, K, m).astype(np.int32)
    out = rng.random(m) < 0.05
    lab[out] = np.where(rng.random(int(out.sum())) < 0.5, -1, K + rng.integers(0, 3, int(out.sum())))
    lab[1], lab[2] = -1, K
    return lab


def log1p_normalized(ptr, val, target=1e4):
    """log1p of the rows scaled to `target` (an empty or all-zero row stays as it is), in the values' own type"""
    v64 = val.astype(np.float64)
    sums = np.add.reduceat(np.concatenate([v64, [0.0]]), np.minimum(ptr[:-1], v64.size))
    sums[np.diff(ptr) == 0] = 0.0
    scale = np.where(sums > 0, target / np.where(sums > 0, sums, 1.0), 1.0)
    return np.log1p(v64 * np.repeat(scale, np.diff(ptr))).astype(val.dtype)


def columns(ptr, idx, val, m, n):
    """(rows, values) of every column, rows ascending: the CSR read column-wise"""
    ptr = np.asarray(ptr, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
    order = np.argsort(idx, kind="stable")
    bounds = np.searchsorted(idx[order], np.arange(n + 1))
    return [(rows[order[bounds[j]:bounds[j + 1]]], val[order[bounds[j]:bounds[j + 1]]]) for j in range(n)]


def included_rows(m, labels=None, batch=None, K=None):
    """the row mask: every row without labels; label == batch; or, batch None, a label in [0, K)"""
    if labels is None:
        return np.ones(m, dtype=bool)
    labels = np.asarray(labels)
    return labels == batch if batch is not None else (labels >= 0) & (labels < K)


# ---- 1. transformed column moments --------------------------------------------------------------------------------------
def transformed(v, transform, clip_j=None):
    """f_j(x) of the stored values of one column, in f64"""
    x = np.asarray(v).astype(np.float64)
    if transform == CLIP:
        return np.minimum(x, clip_j)
    if transform == EXPM1:
        return np.expm1(x)
    return x


def moments(cols, rows_mask, transform, clip=None, reverse=False):
    """(sum, sum_squared, n_clipped) per column over the stored entries of the rows of rows_mask"""
    n = len(cols)
    s, q, c = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    for j, (r, v) in enumerate(cols):
        v = v[rows_mask[r]]
        if reverse:
            v = v[::-1]
        f = transformed(v, transform, None if clip is None else clip[j])
        s[j], q[j] = f.sum(), (f * f).sum()
        if transform == CLIP:
            c[j] = int((v.astype(np.float64) > clip[j]).sum())
    return s, q, c


# ---- 2. local quadratic regression --------------------------------------------------------------------------------------
def loess_window(span, n):
    return min(n, max(3, int(np.floor(span * n + 1e-5))))


def loess_point(x, y, i, q, reverse=False):
    """the fit at x[i] (x sorted or not): the header's definition"""
    d = np.abs(x - x[i])
    h = np.partition(d, q - 1)[q - 1]
    if h > 0:
        sel = np.nonzero(d < h)[0]
        sel = sel[np.argsort(x[sel], kind="stable")]
        if reverse:
            sel = sel[::-1]
        w = (1.0 - (d[sel] / h) ** 3) ** 3
        sel, w = sel[w > 0], w[w > 0]
        distinct = np.unique(x[sel]).size
    else:
        distinct = 1
    if distinct >= 3:
        t, ys = (x[sel] - x[i]) / h, y[sel]
        wt = w * t
        wt2 = wt * t
        S = [w.sum(), wt.sum(), wt2.sum(), (wt2 * t).sum(), (wt2 * t * t).sum()]
        T = [(w * ys).sum(), (wt * ys).sum(), (wt2 * ys).sum()]
        A = np.array([[S[0], S[1], S[2]], [S[1], S[2], S[3]], [S[2], S[3], S[4]]])
        return float(np.linalg.solve(A, np.array(T))[0])
    if distinct == 2:
        t, ys = (x[sel] - x[i]) / h, y[sel]
        wt = w * t
        S0, S1, S2, T0, T1 = w.sum(), wt.sum(), (wt * t).sum(), (w * ys).sum(), (wt * ys).sum()
        return float((T0 * S2 - T1 * S1) / (S0 * S2 - S1 * S1))
    same = y[x == x[i]]
    return float((same[::-1] if reverse else same).sum() / same.size)


def loess_degree(x, i, q):
    """2, 1 or 0 (the plain mean): the branch the fit at x[i] takes"""
    d = np.abs(x - x[i])
    h = np.partition(d, q - 1)[q - 1]
    if not h > 0:
        return 0
    w = (1.0 - (d[d < h] / h) ** 3) ** 3
    return min(np.unique(x[d < h][w > 0]).size, 3) - 1


LOESS_CASES = ("n5", "n64", "n65", "n4000", "half_tied", "all_equal")


def loess_fixture(kind):
    """(x, y) of the GPU test's loess cases, x in random order: n' = 5 (q = 3), 64, 65, 4000 (a window wider than a
    workgroup), a half-tied x whose points take the h == 0 branch and the two-abscissae branch, and an all-equal x"""
    rng = np.random.default_rng(151 + LOESS_CASES.index(kind))
    if kind == "half_tied":   # q = 60 of 200: 70 ties (h == 0); 40 + 15 + 5 -> the 5 sit at distance h: two weighted abscissae
        x = np.concatenate([np.zeros(70), np.full(40, 5.0), np.full(15, 5.5), np.full(5, 9.0), 12.0 + 18.0 * rng.random(70)])
    elif kind == "all_equal":
        x = np.full(100, 2.0)
    else:
        x = rng.normal(0.0, 1.0, int(kind[1:]))
    x = rng.permutation(x)
    y = 0.5 * x * x - x + rng.normal(0.0, 0.3, x.size)
    return x, y


def loess(x, y, span, reverse=False, at=None):
    """fitted values at every point (or at the positions `at`)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.size
    if n == 0:
        return np.zeros(0)
    q = loess_window(span, n)
    where = range(n) if at is None else at
    return np.array([loess_point(x, y, i, q, reverse) for i in where])


# ---- 3. the chain ------------------------------------------------------------------------------------------------------------
def mean_var(s, ss, N):
    mean = s / N
    var = (ss / N - mean * mean) * (N / (N - 1.0))
    return mean, var


def seurat_v3_batch(cols, rows_mask, span, reverse=False):
    """one batch of seurat_v3: {mean, var, est, reg_std, clip, s, ss, n_clipped, norm_var}"""
    N = float(rows_mask.sum())
    s, ss, _ = moments(cols, rows_mask, None, reverse=reverse)
    mean, var = mean_var(s, ss, N)
    ok = var > 0
    est = np.zeros(mean.size)
    est[ok] = loess(np.log10(mean[ok]), np.log10(var[ok]), span, reverse)
    reg_std = np.sqrt(10.0 ** est)
    clip = reg_std * np.sqrt(N) + mean
    cs, css, nclip = moments(cols, rows_mask, CLIP, clip, reverse)
    norm_var = ((N * (mean * mean) + css) - 2.0 * cs * mean) / ((N - 1.0) * (reg_std * reg_std))
    return {"N": N, "mean": mean, "var": var, "est": est, "reg_std": reg_std, "clip": clip, "s": cs, "ss": css, "n_clipped": nclip,
            "norm_var": norm_var}


def rank_desc(v, n_top):
    """position of every column in a stable descending sort of v (NaN last, ties by index); NaN from n_top on"""
    order = np.argsort(-np.asarray(v, dtype=np.float64), kind="stable")
    rank = np.full(order.size, np.nan)
    rank[order[:n_top]] = np.arange(min(n_top, order.size), dtype=np.float64)
    return rank


def combine_v3(norm_vars, n_top):
    """(rank, n_batches_hv, variances_norm, highly_variable) from the K x n norm_var table"""
    norm_vars = np.atleast_2d(np.asarray(norm_vars, dtype=np.float64))
    K, n = norm_vars.shape
    ranks = np.stack([rank_desc(norm_vars[b], n_top) for b in range(K)])
    nhv = (~np.isnan(ranks)).sum(axis=0).astype(np.uint32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        rank = np.nanmedian(ranks, axis=0)
    vnorm = np.zeros(n)
    for b in range(K):
        vnorm = vnorm + norm_vars[b]
    vnorm = vnorm / K
    order = np.lexsort((np.arange(n), -nhv.astype(np.int64), np.where(np.isnan(rank), np.inf, rank)))
    hv = np.zeros(n, dtype=np.uint8)
    hv[order[:n_top]] = 1
    return rank, nhv, vnorm, hv


def cut_edges(x, n_bins):
    """the edges of pandas.cut(x, bins = n_bins) (right-closed)"""
    mn, mx = float(np.min(x)), float(np.max(x))
    if mn == mx:
        mn -= 0.001 * abs(mn) if mn != 0 else 0.001
        mx += 0.001 * abs(mx) if mx != 0 else 0.001
        return np.linspace(mn, mx, n_bins + 1)
    edges = np.linspace(mn, mx, n_bins + 1)
    edges[0] -= (mx - mn) * 0.001
    return edges


def cut_bins(x, n_bins):
    """bin of every value: edges[i] < x <= edges[i + 1]"""
    return np.searchsorted(cut_edges(x, n_bins), x, side="left") - 1


def nan_to_num(v):
    return np.nan_to_num(v)


def within_cutoffs(mean, norm, min_mean, max_mean, min_disp, max_disp):
    d = np.where(np.isnan(norm), 0.0, norm)
    return (mean > min_mean) & (mean < max_mean) & (d > min_disp) & (d < max_disp)


def seurat_batch(s, ss, N, n_top, n_bins, cutoffs):
    """one batch of the seurat flavour from its EXPM1 moments: {mean, var, disp, norm, hv, bins, bin_count, bin_std}"""
    mean, var = mean_var(s, ss, float(N))
    mean = np.where(mean == 0, 1e-12, mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        disp = var / mean
        disp = np.where(disp == 0, np.nan, disp)
        disp = np.log(disp)
        mean = np.log1p(mean)
        bins = cut_bins(mean, n_bins)
        bmean, bstd, bcnt = np.zeros(n_bins), np.zeros(n_bins), np.zeros(n_bins, dtype=np.int64)
        for i in range(n_bins):
            d = disp[(bins == i) & ~np.isnan(disp)]
            bcnt[i] = d.size
            if d.size >= 2:
                bmean[i] = d.sum() / d.size
                bstd[i] = np.sqrt(((d - bmean[i]) ** 2).sum() / (d.size - 1))
            else:
                bstd[i] = d[0] if d.size else np.nan
                bmean[i] = 0.0
        norm = (disp - bmean[bins]) / bstd[bins]
    if n_top:
        valid = np.sort(norm[~np.isnan(norm)])[::-1]
        hv = (nan_to_num(norm) >= valid[min(n_top, valid.size) - 1]) if valid.size else np.zeros(norm.size, dtype=bool)
    else:
        hv = within_cutoffs(mean, norm, *cutoffs)
    return {"mean": mean, "var": var, "disp": disp, "norm": norm, "hv": hv.astype(np.uint8), "bins": bins, "bin_count": bcnt,
            "bin_std": bstd}


def nanmean_rows(table):
    table = np.asarray(table, dtype=np.float64)
    ok = ~np.isnan(table)
    cnt = ok.sum(axis=0)
    acc = np.zeros(table.shape[1])
    for b in range(table.shape[0]):
        acc = acc + np.where(ok[b], table[b], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, acc / cnt, np.nan)


DEFAULT_CUTOFFS = (0.0125, 3.0, 0.5, np.inf)


def hvg(ptr, idx, val, m, n, labels=None, K=1, flavor=SEURAT_V3, n_top=2000, span=0.3, n_bins=20, cutoffs=DEFAULT_CUTOFFS,
        reverse=False):
    """sapca_hvg_csr_device_*: the eight outputs by name, and "batches": what every batch computed on the way"""
    cols = columns(ptr, idx, val, m, n)
    K = K if labels is not None else 1
    masks = [included_rows(m, labels, b if labels is not None else None, K) for b in range(K)]
    nan = np.full(n, np.nan)
    if flavor == SEURAT_V3:
        bs = [seurat_v3_batch(cols, mk, span, reverse) for mk in masks]
        rank, nhv, vnorm, hv = combine_v3([b["norm_var"] for b in bs], n_top)
        if K == 1:
            mean, var = bs[0]["mean"], bs[0]["var"]
        else:
            all_rows = included_rows(m, labels, None, K)
            s, ss, _ = moments(cols, all_rows, None, reverse=reverse)
            mean, var = mean_var(s, ss, float(all_rows.sum()))
        return {"means": mean, "variances": var, "variances_norm": vnorm, "dispersions": nan, "dispersions_norm": nan, "rank": rank,
                "n_batches_hv": nhv, "highly_variable": hv, "batches": bs}
    bs = []
    for mk in masks:
        s, ss, _ = moments(cols, mk, EXPM1, reverse=reverse)
        bs.append(seurat_batch(s, ss, mk.sum(), n_top, n_bins, cutoffs))
    nhv = np.sum([b["hv"] for b in bs], axis=0).astype(np.uint32)
    if K == 1:
        mean, var, disp, norm, hv = (bs[0][k] for k in ("mean", "var", "disp", "norm", "hv"))
    else:
        mean, var, disp, norm = (nanmean_rows([b[k] for b in bs]) for k in ("mean", "var", "disp", "norm"))
        if n_top:
            order = np.lexsort((np.arange(n), np.where(np.isnan(norm), np.inf, -norm), -nhv.astype(np.int64)))
            hv = np.zeros(n, dtype=np.uint8)
            hv[order[:n_top]] = 1
        else:
            hv = within_cutoffs(mean, norm, *cutoffs).astype(np.uint8)
    return {"means": mean, "variances": var, "variances_norm": nan, "dispersions": disp, "dispersions_norm": norm, "rank": nan,
            "n_batches_hv": nhv, "highly_variable": hv, "batches": bs}


def cut_gap(values, n_top):
    """relative gap across the cut of a descending sort: (v[n_top - 1] - v[n_top]) / |v[n_top - 1]|, inf when nothing is cut"""
    v = np.sort(np.asarray(values, dtype=np.float64)[~np.isnan(values)])[::-1]
    if n_top >= v.size:
        return np.inf
    return float((v[n_top - 1] - v[n_top]) / abs(v[n_top - 1]))

"""Per-batch means / variances and top-n row sums on a device-resident matrix (-m gpu), through the C ABI
(sapca_batch_stats_csr_device_*, sapca_sum_row_n_top_csr_device_*) against the host restatement in batch_stats_ref.py.

Bars: counts exact; means and variances within 1e-9 relative (f64 accumulation of values exact in f64, another order);
top-n sums bitwise on integer-valued data."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import batch_stats_ref as B
import sapca
import sapca_oracle as O
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

BIG_CODES = 1100   # more codes than one launch of the labelled statistics holds (1,024): two launches


def _resident(A, sess=None):
    sess = sess or ops.Session()
    A = A.tocsr()
    A.sort_indices()
    return sess, sess.upload(A.indptr, A.indices, A.data, A.shape[0], A.shape[1])


def _mixed(m, n, density, seed, dtype, integer=False):
    """stored explicit zeros, negative values, an empty row and an empty column"""
    rng = np.random.default_rng(seed)
    D = (rng.random((m, n)) < density) * (rng.integers(-4, 12, (m, n)) if integer else rng.normal(1.5, 4.0, (m, n)))
    stored = (D != 0) | (rng.random((m, n)) < 0.01)
    stored[7, :] = False
    stored[:, 3] = False
    r, c = np.nonzero(stored)
    A = sp.csr_matrix((D[r, c].astype(dtype), (r, c)), shape=(m, n))
    A.sort_indices()
    return A


def _arrays(A):
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data


def _close(got, want, what):
    scale = max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * scale, err_msg=what)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n_batches", [1, 3, BIG_CODES])
@pytest.mark.parametrize("axis", [0, 1])
def test_batch_stats_against_the_restatement(dt, n_batches, axis):
    m, n = 2600, 900
    A = _mixed(m, n, 0.05, 11 + n_batches, dt)
    ptr, idx, val = _arrays(A)
    rng = np.random.default_rng(n_batches)
    ln = m if axis == 0 else n
    codes = rng.integers(0, n_batches, ln).astype(np.int32)      # labels scattered over the rows / columns, not runs
    if n_batches > 2:
        codes[codes == 1] = 0                                     # one code that never occurs
    sess, R = _resident(A)
    got = R.batch_stats(axis, codes, n_batches)
    mean, var, cnt = B.batch_stats(ptr, idx, val, m, n, axis, codes, n_batches)
    np.testing.assert_array_equal(got["count"], cnt)
    _close(got["mean"], mean, "mean")
    _close(got["var"], var, "var")
    if n_batches > 2:
        assert not got["mean"][1].any() and not got["var"][1].any() and not got["count"][1].any()


def test_wrapper_methods_with_string_labels():
    m, n = 1500, 400
    A = _mixed(m, n, 0.08, 5, np.float32)
    ptr, idx, val = _arrays(A)
    rng = np.random.default_rng(2)
    row_labels = [["donor-a", "donor-b", "donor-c", "solo"][j] for j in rng.integers(0, 3, m)]
    row_labels[100] = "solo"                                       # a batch of one row: variance 0 everywhere
    col_labels = [("chip", int(j)) for j in rng.integers(0, 4, n)]
    sess, R = _resident(A)
    for fn, labels, axis, what in ((R.var_batch_row, row_labels, 0, 1), (R.mean_batch_col, row_labels, 0, 0),
                                   (R.var_batch_col, col_labels, 1, 1), (R.mean_batch_row, col_labels, 1, 0)):
        names, codes = B.dense_codes(labels)
        want = B.to_dict(names, B.batch_stats(ptr, idx, val, m, n, axis, codes, len(names))[what])
        got = fn(labels)
        assert set(got) == set(want)
        for k in want:
            _close(got[k], want[k], f"{fn.__name__}[{k}]")
    assert not R.var_batch_row(row_labels)["solo"].any()


def _top_n_matrix(dt):
    """integer count data: one row of 110,000 entries, rows around the register tile (1,024), rows of many ties,
    stored zeros and negative values, empty rows"""
    n = 120_000
    rng = np.random.default_rng(9)
    lens = [110_000, 0, 1, 5, 63, 64, 65, 1000, 1024, 1025, 4000, 20_000, 0, 3000, 700, 2048]
    rows, cols, vals = [], [], []
    for r, L_ in enumerate(lens):
        c = np.sort(rng.choice(n, L_, replace=False))
        if r in (3, 13, 14):
            v = rng.integers(0, 3, L_)                              # ties at the threshold everywhere
        elif r == 15:
            v = np.full(L_, 2)                                      # one value only
        else:
            v = rng.negative_binomial(1, 0.3, L_) - (rng.random(L_) < 0.1) * 7
        rows.append(np.full(L_, r))
        cols.append(c)
        vals.append(v)
    A = sp.csr_matrix((np.concatenate(vals).astype(dt), (np.concatenate(rows), np.concatenate(cols))), shape=(len(lens), n))
    A.sort_indices()
    return A


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_sum_row_n_top_is_bitwise_on_count_data(dt):
    A = _top_n_matrix(dt)
    ptr, idx, val = _arrays(A)
    assert np.diff(ptr).max() >= 100_000 and (val == 0).any() and (val < 0).any()
    sess, R = _resident(A)
    ns = [0, 1, 2, 3, 50, 100, 200, 500, 1024, 1025, 5000, 100_000, 200_000]
    got = R.sum_row_n_top(ns)
    assert got.shape == (len(ns), A.shape[0])
    for i, k in enumerate(ns):
        np.testing.assert_array_equal(got[i], B.sum_row_n_top(ptr, val, k), err_msg=f"n = {k}")
    np.testing.assert_array_equal(R.sum_row_n_top(50), got[ns.index(50)])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_sum_row_n_top_on_real_values(dt):
    A = _mixed(700, 3000, 0.2, 4, dt)
    ptr, idx, val = _arrays(A)
    sess, R = _resident(A)
    for k in (1, 7, 300, 599, 2000):
        np.testing.assert_allclose(R.sum_row_n_top(k), B.sum_row_n_top(ptr, val, k), rtol=1e-12, atol=1e-10)


def test_at_the_c4_shard_size_row_sampled():
    """125,000 x 30,000 at 3 % (1.1e8 stored entries, one GPU's share of C4): batch statistics on both axes and top-n,
    sampled lines against the restatement"""
    m, n = 125_000, 30_000
    p, i, v = synth.flat_csr(m, n, 0.03, seed=17, dtype=torch.float32, device="cuda")
    ptr, idx = p.cpu().numpy().astype(np.int64), i.cpu().numpy().astype(np.int64)
    val = np.round(v.cpu().numpy())                                # integer values in [-10, 10], stored zeros among them
    del p, i, v
    torch.cuda.empty_cache()
    assert len(val) > 1.0e8
    sess = ops.Session()
    R = sess.upload(ptr, idx, val, m, n)
    rng = np.random.default_rng(1)
    nb = 8
    row_codes = rng.integers(0, nb, m).astype(np.int32)
    col_codes = rng.integers(0, nb, n).astype(np.int32)
    # per-column results (codes label the rows): a sample of columns
    got = R.batch_stats(0, row_codes, nb)
    cols = np.sort(rng.choice(n, 40, replace=False))
    keep = np.isin(idx, cols)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))[keep]
    sub = sp.csr_matrix((val[keep].astype(np.float64), (rows, np.searchsorted(cols, idx[keep]))), shape=(m, len(cols)))
    sub.sort_indices()
    mean, var, cnt = B.batch_stats(sub.indptr, sub.indices, sub.data, m, len(cols), 0, row_codes, nb)
    np.testing.assert_array_equal(got["count"][:, cols], cnt)
    _close(got["mean"][:, cols], mean, "mean (per column)")
    _close(got["var"][:, cols], var, "var (per column)")
    del got, keep, rows
    # per-row results (codes label the columns) and top-n: a sample of rows
    got = R.batch_stats(1, col_codes, nb)
    rs = np.sort(rng.choice(m, 300, replace=False))
    sub = sp.csr_matrix((val, idx, ptr), shape=(m, n))[rs]
    sub.sort_indices()
    mean, var, cnt = B.batch_stats(sub.indptr, sub.indices, sub.data.astype(np.float64), len(rs), n, 1, col_codes, nb)
    np.testing.assert_array_equal(got["count"][:, rs], cnt)
    _close(got["mean"][:, rs], mean, "mean (per row)")
    _close(got["var"][:, rs], var, "var (per row)")
    del got
    ns = [20, 50, 100, 200, 500, 2000]
    top = R.sum_row_n_top(ns)
    for j, k in enumerate(ns):
        np.testing.assert_array_equal(top[j, rs], B.sum_row_n_top(ptr, val, k, rows=rs), err_msg=f"n = {k}")


def test_errors():
    A = _mixed(40, 30, 0.2, 1, np.float64)
    sess, R = _resident(A)
    good = np.zeros(40, dtype=np.int32)
    with pytest.raises(L.SapcaError) as e:
        R.batch_stats(0, good[:39], 1, want=("var",))
    assert str(e.value) == "Batch vector length (39) doesn't match matrix row count (40)" and e.value.status == L.ERR_ARG
    with pytest.raises(L.SapcaError) as e:
        R.batch_stats(1, good[:31], 1, want=("mean",))
    assert str(e.value) == "Number of batch identifiers (31) must match number of columns (30)"
    bad = good.copy()
    bad[17] = 3
    with pytest.raises(L.SapcaError, match="outside") as e:
        R.batch_stats(0, bad, 3)
    assert e.value.status == L.ERR_ARG
    bad[17] = -1
    with pytest.raises(L.SapcaError, match="outside"):
        R.batch_stats(0, bad, 3)
    with pytest.raises(L.SapcaError, match="grouped_axis") as e:
        R.batch_stats(2, good, 1)
    assert e.value.status == L.ERR_ARG
    ns = np.zeros(1, dtype=np.uint64)
    out = np.zeros(40)
    st = L.load().sapca_sum_row_n_top_csr_device_f64(*R._args(), ops._p(ns, ops.C.c_uint64), ops.C.c_uint32(0), ops._p(out, ops.C.c_double))
    assert st == L.ERR_ARG
    with pytest.raises(ValueError, match="row count"):
        R.var_batch_row(["a"] * 41)
    # the handle still works after the errors
    np.testing.assert_array_equal(R.batch_stats(0, good, 1)["count"][0], np.bincount(A.indices, minlength=30))


def test_end_to_end_batch_aware_gene_selection_then_masked_pca():
    """upload -> normalize -> log1p -> var_batch_row -> mask of the top-k genes by mean per-batch variance ->
    MaskedSparsePCA fit on the same resident arrays; the mask against the host restatement, the fit against O.fit"""
    m, n, k, p, q, top = 4000, 900, 8, 6, 2, 300
    ptr, idx, val = (x.cpu().numpy() for x in synth.gapped_csr(m, n, 0.05, k, seed=21, dtype=torch.float32))
    ptr, idx = ptr.astype(np.int64), idx.astype(np.int64)
    sess, R = _resident(sp.csr_matrix((val, idx, ptr), shape=(m, n)))
    R.normalize(R.stats(ops.ROW)[0], 1e3, ops.ROW).log1p()
    rng = np.random.default_rng(8)
    donors = [f"donor{j}" for j in rng.integers(0, 4, m)]
    per_batch = R.var_batch_row(donors)
    score = np.mean([per_batch[b] for b in sorted(per_batch)], axis=0)
    mask = np.zeros(n, dtype=bool)
    mask[np.argsort(-score, kind="stable")[:top]] = True
    # the host restatement on the values as they are on the device
    v2 = R.values().astype(np.float64)
    names, codes = B.dense_codes(donors)
    hv = B.to_dict(names, B.batch_stats(ptr, idx, v2, m, n, 0, codes, len(names))[1])
    hscore = np.mean([hv[b] for b in sorted(hv)], axis=0)
    order = np.argsort(-hscore, kind="stable")
    assert hscore[order[top - 1]] > hscore[order[top]] * (1 + 1e-6)     # the cut is not a near tie
    want_mask = np.zeros(n, dtype=bool)
    want_mask[order[:top]] = True
    np.testing.assert_array_equal(mask, want_mask)
    om = synth.gaussian_panel(top, k + p, 5).numpy()
    est = (sapca.MaskedSparsePCABuilder.new().n_components(k).mask(mask)
           .svd_method(SVDMethod.Random(p, q, PIN.QR)).build().set_omega(om))
    est.fit(R.as_device_csr())
    want = O.fit(ptr, idx, v2, m, n, n_components=k, n_oversamples=p, n_power_iterations=q, omega=om, mask=mask)
    assert O.subspace_angle(est.components_(np.float64), want.components) < 1e-4
    np.testing.assert_allclose(est.singular_values_(np.float64), want.singular_values, rtol=1e-4)

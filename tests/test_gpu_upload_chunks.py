"""The chunked host upload at its chunk boundaries (-m gpu).

Every host entry point goes through upload() in csrc/api.cpp: column indices narrowed on a few host threads, sent in chunks
through a two-slot page-locked ring, and per chunk one launch of the column-statistics kernel (csrc/upstats.hip) on the rows
the chunk touches, its first and last row clipped to the chunk's entries.  The release chunk is 2^24 entries; the debug
variant reads SAPCA_UP_CHUNK on every upload, which puts chunk boundaries where these tests want them on small matrices.

Bars: bit for bit.  The statistics are exact integer accumulations rounded once, so every chunking gives the correctly
rounded exact sums (exact_sums_ref.py); the uploaded arrays equal the input; a fit does not see the chunking."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import sapca
from exact_sums_ref import exact_column_sums
from sapca import _lib as L
from sapca import ops, synth
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod

pytestmark = pytest.mark.gpu

N_A = 10241                                   # eight full 1,280-column tiles of the accumulators and one column
EDGE_COLS = (0, 1279, 1280, 2559, 2560, N_A - 1)
LONG = 10000                                  # the row that spans several chunks


def _layout_a():
    """row lengths of the matrix of group (a): runs of empty rows at the start, in the middle and at the end; rows of 1, 63, 64,
    65 entries (one probe round of the 64-ary search and its edges), 4095, 4096, 4097 (two rounds and the first length that
    takes a third) and one of 10,000; short rows in between"""
    rng = np.random.default_rng(20)
    short = lambda k: rng.integers(0, 63, k).tolist()   # noqa: E731
    lens = ([0, 0, 0] + short(300) + [63, 64, 65, 1] + short(300) + [4095, 0, 0, 0, 0, 4096] + short(300) + [7, LONG, 4097]
            + short(400) + [0, 0, 0])
    lens = np.asarray(lens, dtype=np.int64)
    if lens.sum() % 2 == 0:   # an odd number of entries: nnz - 1 splits into two equal chunks ("one_before_the_end")
        lens[3] += 1
    return lens


@functools.lru_cache(maxsize=None)
def _matrix_a():
    """(ptr, idx) of group (a): columns ascending and unique per row; every row of 63 entries or more holds the columns at the
    edges of the first tiles and the last column"""
    lens = _layout_a()
    rng = np.random.default_rng(21)
    rest = np.setdiff1d(np.arange(N_A), EDGE_COLS)
    cols = []
    for k in lens.tolist():
        if k >= 63:
            c = np.concatenate([np.asarray(EDGE_COLS), rng.choice(rest, k - len(EDGE_COLS), replace=False)])
        else:
            c = rng.choice(N_A, k, replace=False)
        cols.append(np.sort(c))
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate(cols).astype(np.int64)
    ptr.setflags(write=False)
    idx.setflags(write=False)
    return ptr, idx


@functools.lru_cache(maxsize=None)
def _values_a(dtype):
    """The recipe of test_statistics_gathered_behind_the_upload_are_the_exact_sums (cancelling pairs, a stored +0.0 and -0.0, a
    subnormal) with the exponents spread over the format: every column has a ceiling anywhere in the range (f32: the whole
    finite range, f64: +-400 binades), its entries lie up to 30 binades below it and, one in three, up to 200 below.  The
    edge columns have the upload's largest magnitude as their ceiling, so their pieces land both in the LDS window of the
    accumulators (70 binades below the largest value) and straight in memory."""
    ptr, idx = _matrix_a()
    rng = np.random.default_rng(22)
    nnz = idx.size
    lo, hi = (-149, 127) if dtype == np.float32 else (-400, 400)
    ceil = rng.integers(lo, hi + 1, N_A)
    ceil[list(EDGE_COLS)] = hi
    below = np.where(rng.random(nnz) < 2 / 3, rng.integers(0, 31, nnz), rng.integers(0, 201, nnz))
    for c in EDGE_COLS:
        e = np.flatnonzero(idx == c)
        below[e] = np.resize([0, 100, 3, 180, 20, 76, 29, 71], e.size)
    expo = np.maximum(ceil[idx] - below, lo)             # (f32: the bottom of the range is subnormal)
    v = (1.0 + rng.random(nnz)) * np.where(rng.random(nnz) < 0.5, -1.0, 1.0) * np.exp2(expo.astype(np.float64))
    v = v.astype(dtype)                                    # (below 2 * 2^127 / 2^400: finite, and so are the squares in f64)
    kk = (nnz - 1) // 7
    order = np.argsort(idx, kind="stable")                 # neighbours in this order share a column: the pairs cancel exactly
    a, b = order[0:7 * kk:7], order[1:7 * kk + 1:7]
    same = idx[a] == idx[b]
    v[a[same]] = -v[b[same]]
    v[5], v[6] = 0.0, -0.0                                 # stored zeros count as entries
    v[11] = np.float32(1e-42) if dtype == np.float32 else 5e-324
    assert np.isfinite(v).all() and same.sum() > 1000
    mag = np.abs(v.astype(np.float64))
    top = np.log2(mag.max())
    near = np.bincount(idx[mag > 0][np.log2(mag[mag > 0]) > top - 30], minlength=N_A) > 0
    far = np.bincount(idx[mag > 0][np.log2(mag[mag > 0]) < top - 75], minlength=N_A) > 0
    assert (near & far)[list(EDGE_COLS)].all()             # window and memory in one column
    want_s, want_sq = exact_column_sums(idx, v.astype(np.float64), N_A)
    assert np.isfinite(want_sq).all()
    with np.errstate(over="ignore"):                       # f32: what leaves the library is the f64 result narrowed
        want = (want_s.astype(dtype), want_sq.astype(dtype), np.bincount(idx, minlength=N_A).astype(np.uint64))
    v.setflags(write=False)
    return v, want


def _chunk_length(label, ptr, lens):
    """the chunk length a label of group (a) stands for, with the property that gives it its name asserted"""
    nnz = int(ptr[-1])
    if isinstance(label, int):
        return label
    if label in ("nnz-1", "nnz", "nnz+1"):
        return nnz + {"nnz-1": -1, "nnz": 0, "nnz+1": 1}[label]
    if label == "on_empty_rows":        # the first boundary falls where rows r-2 and r-1 are empty: ptr[r-2] == ptr[r-1] == ptr[r]
        r = int(np.flatnonzero(lens == 4096)[0])
        assert lens[r - 1] == 0 and lens[r - 2] == 0 and 0 < ptr[r] < nnz and ptr[r - 2] == ptr[r]
        return int(ptr[r])
    if label == "at_row_start":         # the first boundary is the start of a row that has entries, after one that has entries
        r = int(np.flatnonzero(lens == LONG)[0])
        assert lens[r] > 0 and lens[r - 1] > 0 and 0 < ptr[r] < nnz
        return int(ptr[r])
    if label == "inside_long_row":      # three boundaries strictly inside the 10,000-entry row
        r = int(np.flatnonzero(lens == LONG)[0])
        for c in range(2501, 5000):
            inside = [b for b in range(c, nnz, c) if ptr[r] < b < ptr[r + 1]]
            if len(inside) == 3:
                return c
        raise AssertionError("no chunk length puts three boundaries inside the long row")
    if label == "one_before_the_end":   # the last chunk holds one entry, and it is not the nnz-1 case (two full chunks before it)
        c = (nnz - 1) // 2
        assert (nnz - 1) % c == 0 and (nnz - 1) // c == 2 and lens[np.flatnonzero(lens)[-1]] > 1
        return c
    raise KeyError(label)


CHUNKS_A = [64, 1000, 4097, 70000, "nnz-1", "nnz", "nnz+1", "on_empty_rows", "at_row_start", "inside_long_row", "one_before_the_end"]


def test_the_matrix_of_group_a_is_what_the_cases_need():
    ptr, idx = _matrix_a()
    lens = np.diff(ptr)
    assert 5.5e4 < idx.size < 6.5e4 and idx.size % 2 == 1            # (odd: nnz - 1 splits into two equal chunks)
    assert {0, 1, 63, 64, 65, 4095, 4096, 4097, LONG} <= set(lens.tolist())
    empty = lens == 0
    runs = empty[:-2] & empty[1:-1] & empty[2:]
    assert runs[0] and runs[-1] and runs[300:-300].any()
    assert all((idx == c).sum() >= 7 for c in EDGE_COLS)
    rows = np.repeat(np.arange(lens.size), lens)
    asc = (np.diff(idx) > 0) | (np.diff(rows) > 0)
    assert asc.all() and idx.min() == 0 and idx.max() == N_A - 1
    assert len({_chunk_length(c, ptr, lens) for c in CHUNKS_A}) == len(CHUNKS_A)


@pytest.mark.parametrize("chunk", CHUNKS_A, ids=str)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_statistics_are_exact_at_every_chunking(debug_switches, monkeypatch, dtype, chunk):
    """(a) one matrix, many chunkings: sums, sums of squares and counts equal the exact reference and the unswitched run"""
    ptr, idx = _matrix_a()
    val, want = _values_a(dtype)
    m = ptr.size - 1
    length = _chunk_length(chunk, ptr, np.diff(ptr))
    sess = ops.Session()
    monkeypatch.setenv("SAPCA_UP_CHUNK", str(length))
    got = sess.colstats(ptr, idx, val, m, N_A)
    monkeypatch.delenv("SAPCA_UP_CHUNK")
    plain = sess.colstats(ptr, idx, val, m, N_A)
    for name, g, p, w in zip(("sum", "sum of squares", "count"), got, plain, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (f"{name}, chunk {length}: {bad.size} columns differ from the exact reference, first {bad[:5]}: "
                               f"{g[bad[:5]]} for {w[bad[:5]]}")
        assert np.array_equal(p, w), f"{name} without the switch differs from the exact reference"
        assert np.array_equal(g, p), f"{name}: chunk {length} differs from the run without the switch"


def _read_back(R):
    d = R.as_device_csr()
    return d.row_offsets.cpu().numpy(), d.col_indices.cpu().numpy(), d.values.cpu().numpy()


def _assert_arrived(R, ptr, idx, val):
    p, i, v = _read_back(R)
    assert p.dtype == np.int64 and i.dtype == np.int32 and v.dtype == val.dtype
    assert np.array_equal(p, ptr), "row offsets"
    assert np.array_equal(i, idx.astype(np.int32)), f"column indices differ first at entry {int(np.flatnonzero(i != idx)[0])}"
    bits = np.uint32 if val.dtype == np.float32 else np.uint64
    assert np.array_equal(v.view(bits), val.view(bits)), "value bits"


@functools.lru_cache(maxsize=None)
def _matrix_four_chunks():
    """278,000 stored entries, small-integer values: four chunks of 70,000 (each ring slot used twice), every one of them
    above the 65,536 entries at which the narrowing runs on several threads -- the last one too (68,000)"""
    m, n = 5000, 2000
    A = sp.random(m, n, density=0.0278, format="csr", random_state=31, dtype=np.float64)
    A.sort_indices()
    ptr, idx = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    val = np.random.default_rng(32).integers(-9, 10, idx.size).astype(np.float32)
    assert idx.size == 278000 and idx.size - 3 * 70000 >= 1 << 16
    for a in (ptr, idx, val):
        a.setflags(write=False)
    return m, n, ptr, idx, val


@pytest.mark.parametrize("chunk", [64, 4097])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_uploaded_arrays_arrive_intact(debug_switches, monkeypatch, dtype, chunk):
    """(b) offsets, column indices (as int32) and value bits on the device equal the input"""
    ptr, idx = _matrix_a()
    val, _ = _values_a(dtype)
    monkeypatch.setenv("SAPCA_UP_CHUNK", str(chunk))
    sess = ops.Session()
    _assert_arrived(sess.upload(ptr, idx, val, ptr.size - 1, N_A), ptr, idx, val)


def test_uploaded_arrays_arrive_intact_through_reused_slots_and_threaded_narrowing(debug_switches, monkeypatch):
    m, n, ptr, idx, val = _matrix_four_chunks()
    monkeypatch.setenv("SAPCA_UP_CHUNK", "70000")
    sess = ops.Session()
    _assert_arrived(sess.upload(ptr, idx, val, m, n), ptr, idx, val)


def _fit_outputs(est, A):
    t = est.fit_transform(A)
    return est.mean_(np.float64), est.explained_variance_ratio(np.float64), est.components_(np.float64), t


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_a_fit_does_not_see_the_chunking(debug_switches, monkeypatch, masked):
    """(c) the statistics are order-independent and the uploaded matrix is the same: mean, explained variance ratio,
    components and projection of a host fit are bit-identical with a dozen chunks and with one"""
    m, n, k, p, q = 20000, 1500, 10, 6, 2
    ptr, idx, val = (x.numpy() for x in synth.gapped_csr(m, n, 0.04, 10, dtype=torch.float32))
    A = sp.csr_matrix((val, idx.astype(np.int64), ptr.astype(np.int64)), shape=(m, n))
    assert A.nnz == val.size and A.nnz > 10 * 100003
    mask = synth.bernoulli_mask(n, 0.6, 7).numpy() if masked else None
    om = synth.gaussian_panel(int(mask.sum()) if masked else n, k + p, 3).numpy()

    def estimator():
        b = sapca.MaskedSparsePCABuilder.new().mask(mask) if masked else sapca.SparsePCABuilder.new()
        return b.n_components(k).random_seed(42).svd_method(SVDMethod.Random(p, q, PIN.QR)).build().set_omega(om)

    monkeypatch.setenv("SAPCA_UP_CHUNK", "100003")
    chunked = _fit_outputs(estimator(), A)
    monkeypatch.delenv("SAPCA_UP_CHUNK")
    plain = _fit_outputs(estimator(), A)
    for name, a, b in zip(("mean_", "explained_variance_ratio", "components_", "projection"), chunked, plain):
        assert np.isfinite(a).all() and np.array_equal(a, b), name


def test_a_bad_column_in_any_chunk_is_refused_and_the_session_goes_on(debug_switches, monkeypatch):
    """(d) four chunks of 70,000: a column index equal to n in the last eighth of the last chunk (the last narrowing thread's
    share), and one of 2^32 + 3 in the second chunk, which narrows to a valid 3 -- the host check on the 64-bit value is what
    refuses it.  The same Session then gives the exact statistics of the clean matrix (small integers: bincount in f64 is
    exact)."""
    m, n, ptr, idx, val = _matrix_four_chunks()
    nnz = idx.size
    monkeypatch.setenv("SAPCA_UP_CHUNK", "70000")
    sess = ops.Session()
    last = nnz - 3 * 70000
    ends = ptr[1:][np.diff(ptr) > 0] - 1                       # last entry of every row with entries
    at_end = int(ends[ends >= nnz - last // 8][0])
    assert nnz - last // 8 <= at_end < nnz
    in_second = int(ends[ends >= 70000 + 35000][0])
    assert 70000 <= in_second < 140000
    for pos, col in ((at_end, n), (in_second, 2 ** 32 + 3)):
        bad = idx.copy()
        bad[pos] = col
        assert col % 2 ** 32 in (n, 3)                          # what the narrowing makes of it
        with pytest.raises(L.SapcaError, match="column index out of range") as e:
            sess.colstats(ptr, bad, val, m, n)
        assert e.value.status == L.ERR_ARG
    s, sq, cnt = sess.colstats(ptr, idx, val, m, n)
    v64 = val.astype(np.float64)
    assert np.array_equal(s, np.bincount(idx, weights=v64, minlength=n).astype(np.float32))
    assert np.array_equal(sq, np.bincount(idx, weights=v64 * v64, minlength=n).astype(np.float32))
    assert np.array_equal(cnt.astype(np.int64), np.bincount(idx, minlength=n))


def test_the_release_chunk_length_once():
    """(e) the release library and its constant: 2^24 + 300,784 entries in rows of 1,000, so the one chunk boundary falls
    strictly inside a row.  Small-integer values: the column sums are integers below 2^24 (their f32 results are exact too),
    and np.bincount in f64 is the exact reference."""
    cut, n, per = 1 << 24, 4000, 1000
    m = 17078
    nnz = m * per
    assert nnz - cut == 300784
    ptr = np.arange(m + 1, dtype=np.int64) * per
    r = int(np.searchsorted(ptr, cut, side="right")) - 1
    assert ptr[r] < cut < ptr[r + 1]                                  # the boundary is strictly inside row r
    rows = np.arange(m, dtype=np.int64)[:, None]
    j = np.arange(per, dtype=np.int64)[None, :]
    idx = (4 * j + rows % 4).reshape(-1)                              # ascending and unique in every row, every column used
    val = ((rows * 7 + j * 13) % 17 - 8).astype(np.float32).reshape(-1)
    sess = ops.Session()
    s, sq, cnt = sess.colstats(ptr, idx, val, m, n)
    v64 = val.astype(np.float64)
    want_s, want_sq = np.bincount(idx, weights=v64, minlength=n), np.bincount(idx, weights=v64 * v64, minlength=n)
    assert np.abs(want_s).max() < 1 << 24 and want_sq.max() < 1 << 24
    assert np.array_equal(s, want_s.astype(np.float32)) and np.array_equal(sq, want_sq.astype(np.float32))
    assert np.array_equal(cnt.astype(np.int64), np.bincount(idx, minlength=n))
    d = sess.upload(ptr, idx, val, m, n).as_device_csr()
    assert np.array_equal(d.col_indices[cut - 4:cut + 4].cpu().numpy(), idx[cut - 4:cut + 4].astype(np.int32))
    assert np.array_equal(d.col_indices[-4:].cpu().numpy(), idx[-4:].astype(np.int32))
    assert np.array_equal(d.values[cut - 4:cut + 4].cpu().numpy(), val[cut - 4:cut + 4])
    assert np.array_equal(d.values[-4:].cpu().numpy(), val[-4:])


def test_edges_of_the_final_rounding():
    """(f) the long accumulator is rounded once, at the precision the result can hold: subnormal sums of squares (a value
    above a tie, a true tie), sums of squares around 2^-1022, a sum that cancels to zero across 600 binades, and squares that
    overflow beside a finite sum.  The last column's sum of squares is inf: exact_column_sums cannot say so (a Fraction that
    large does not convert), so the test states it."""
    t = 2.0 ** -512
    big = np.finfo(np.float64).max / 2
    columns = [
        [2.0 ** -537, 2.0 ** -537, 2.0 ** -538, 2.0 ** -538, 2.0 ** -600],   # 2.5 ulp + 2^-1200 -> 3 ulp (two roundings: 2)
        [2.0 ** -537, 2.0 ** -537, 2.0 ** -538, 2.0 ** -538],                # 2.5 ulp exactly, a tie -> 2 ulp
        [t, t, t, t * (1 - 2.0 ** -51)],                                     # 2^-1022 - 2^-1074 + 2^-1126: the largest subnormal
        [t, t, t, t * (1 - 2.0 ** -52)],                                     # 2^-1022 - 2^-1075 + 2^-1128: rounds up into the normals
        [t, t, t, t * (1 + 2.0 ** -52)],                                     # 2^-1022 + 2^-1075 + 2^-1128: the next normal
        [2.0 ** 300, 2.0 ** -300, -(2.0 ** 300), -(2.0 ** -300)],            # sum exactly 0
        [big, -big, big, -big],                                              # sum 0, squares overflow
    ]
    ulp = 2.0 ** -1074
    n = len(columns)
    r, c, v = zip(*[(i, j, x) for j, col in enumerate(columns) for i, x in enumerate(col)])
    A = sp.csr_matrix((np.array(v), (np.array(r), np.array(c))), shape=(5, n))
    A.sort_indices()
    ptr, idx, val = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data
    assert val.size == sum(len(col) for col in columns)
    finite = idx < n - 1
    want_s, want_sq = exact_column_sums(idx[finite], val[finite], n)
    want_s[n - 1], want_sq[n - 1] = 0.0, np.inf
    assert want_sq[:5].tolist() == [3 * ulp, 2 * ulp, 2.0 ** -1022 - ulp, 2.0 ** -1022, 2.0 ** -1022 + ulp]   # the reference itself
    assert want_s[5] == 0.0 and want_sq[5] == 2.0 ** 601
    s, sq, cnt = ops.Session().colstats(ptr, idx, val, 5, n)
    assert [x / ulp for x in sq[:2]] == [3.0, 2.0], "subnormal sums of squares, in units of 2^-1074"
    assert np.array_equal(sq, want_sq), (sq.tolist(), want_sq.tolist())
    assert np.array_equal(s, want_s), (s.tolist(), want_s.tolist())
    assert cnt.tolist() == [len(col) for col in columns]


def test_a_matrix_too_wide_for_the_accumulators():
    """(g) f64 with 680,000 columns: the accumulators would pass 1 GiB, so the upload gathers nothing and the statistics come
    from the row sums of the transposed matrix (the bar of test_colstats_large_matches_oracle); a narrow matrix on the same
    Session is exact again"""
    m, n, per = 400, 680000, 50
    assert n * (67 + 133) * 8 > 1 << 30
    rng = np.random.default_rng(41)
    ptr = np.arange(m + 1, dtype=np.int64) * per
    idx = np.sort(rng.integers(0, n // per, (m, per)) + (n // per) * np.arange(per)[None, :], axis=1).reshape(-1).astype(np.int64)
    val = rng.uniform(-10, 10, m * per)
    idx[-1] = n - 1
    sess = ops.Session()
    s, sq, cnt = sess.colstats(ptr, idx, val, m, n)
    np.testing.assert_allclose(s, np.bincount(idx, weights=val, minlength=n), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(sq, np.bincount(idx, weights=val * val, minlength=n), rtol=1e-12)
    assert np.array_equal(cnt.astype(np.int64), np.bincount(idx, minlength=n))
    n2 = 1500
    idx2 = idx % 30 + 30 * np.arange(per)[None, :].repeat(m, 0).reshape(-1)     # ascending and unique in every row
    v2 = val * np.exp2(rng.integers(-40, 41, val.size))
    s2, sq2, cnt2 = sess.colstats(ptr, idx2, v2, m, n2)
    want_s, want_sq = exact_column_sums(idx2, v2, n2)
    assert np.array_equal(s2, want_s) and np.array_equal(sq2, want_sq)
    assert np.array_equal(cnt2.astype(np.int64), np.bincount(idx2, minlength=n2))

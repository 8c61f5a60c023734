"""The matrices and masks of tests/masked_prep_cases.py meet the conditions tests/test_gpu_masked_prep.py relies on, checked
without a GPU: integer values on ascending columns, the edge row lengths, the all-dropped and all-kept rows, every forced mask
pattern, the exact n_used, sums that stay exact in f32, a gap of at least 2 at the k each fit asks for (the angle assertions have
no escape clause), and the boundaries restated from the sources on the side of the case that its name says."""
import numpy as np
import pytest

import masked_prep_cases as C
import sapca_oracle as O

ALL = tuple(C.SHAPES) + ("nothing_kept",)
STRUCTURED = ("map_lds_k16", "map_gather_k32", "tail_word", "nothing_dropped", "tall_scatter")


@pytest.mark.parametrize("name", ALL)
def test_values_are_integers_on_ascending_columns(name):
    c = C.case(name)
    assert c.ptr[0] == 0 and c.ptr[-1] == c.nnz and len(c.ptr) == c.m + 1 and c.m & (c.m - 1) == 0
    assert np.array_equal(c.val, np.rint(c.val)) and np.abs(c.val).min() >= 1 and np.abs(c.val).max() == 8
    assert c.idx.min() >= 0 and c.idx.max() < c.n
    inside = np.ones(c.nnz, bool)
    inside[c.ptr[1:-1][c.ptr[1:-1] < c.nnz]] = False          # (the first entry of a row has no left neighbour)
    inside[0] = False
    assert np.all(np.diff(c.idx)[inside[1:]] > 0)
    assert c.csr().has_canonical_format


@pytest.mark.parametrize("name", ALL)
def test_edge_rows(name):
    c = C.case(name)
    lens = np.diff(c.ptr)
    assert C.EDGE_LENGTHS == (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
    assert (C.WRITE_BATCH, C.COUNT_BATCH) == (256, 512)
    assert tuple(lens[:len(C.EDGE_LENGTHS)]) == C.EDGE_LENGTHS
    lo, hi = C.REST.get(name, (20, 120))
    rest = lens[len(C.LENGTHS):]
    assert rest.min() >= lo and rest.max() <= hi
    kept_of = lambda r: c.mask[c.idx[c.ptr[r]:c.ptr[r + 1]]]
    n_kept, n_dropped = int(c.mask.sum()), int((~c.mask).sum())
    if name == "nothing_kept":         # (nothing_dropped's matrix: every entry sits on a column this mask drops)
        assert not c.mask[c.idx].any()
        return
    # a row of 300 entries (a second trip of write_kept_kernel's loop with 44 lanes busy) on dropped columns alone, and one on
    # kept columns alone; where the mask leaves fewer such columns, as many as there are
    if name == "nothing_dropped":      # (no entry on a dropped column, by construction: that row is empty)
        n_dropped = 0
    assert lens[C.DROPPED_ROW] == min(300, n_dropped) and not kept_of(C.DROPPED_ROW).any()
    assert lens[C.KEPT_ROW] == min(300, n_kept) and kept_of(C.KEPT_ROW).all()
    if name in STRUCTURED and name != "nothing_dropped":
        assert lens[C.DROPPED_ROW] == 300 and lens[C.KEPT_ROW] == 300
        mixed = [r for r in range(len(C.EDGE_LENGTHS)) if 0 < kept_of(r).sum() < lens[r]]
        assert len(mixed) >= 10      # (the long edge rows hold kept and dropped entries side by side: the ballots interleave)


@pytest.mark.parametrize("name", STRUCTURED)
def test_mask_patterns(name):
    c = C.case(name)
    m, n, n_used, first, last, _ = C.SHAPES[name]
    assert c.mask.shape == (n,) and int(c.mask.sum()) == n_used == c.n_used
    assert c.mask[0] == first and c.mask[n - 1] == last
    assert set(c.where) == set(C.PATTERNS)
    for kind, w in c.where.items():
        assert 0 < w and 32 * (w + 3) <= n - n % 32
        assert C.pattern_present(c.mask, kind, w), (kind, w)
    # what the patterns are for: words with no kept column (before[w] = 0 in load_column_map), a full word, a lone bit 0 / 31
    words = np.pad(c.mask, (0, -n % 32)).reshape(-1, 32)
    count = words.sum(1)
    assert (count == 0).any() and (count == 32).any()
    assert ((count == 1) & words[:, 0]).any() and ((count == 1) & words[:, 31]).any() and ((count == 31) & ~words[:, 0]).any()


def test_degenerate_masks():
    a, o, nd, nk = (C.case(x) for x in ("all_true", "one_column", "nothing_dropped", "nothing_kept"))
    assert a.mask.all() and a.n_used == a.n
    assert int(o.mask.sum()) == 1 and o.mask[C.ONE_COLUMN] and C.ONE_COLUMN % 32 == 31
    assert np.count_nonzero(o.idx == C.ONE_COLUMN) > 100          # (sigma_1 is the norm of a well-filled column)
    stored = np.bincount(nd.idx, minlength=nd.n) > 0
    assert nd.mask[stored].all() and int((~nd.mask).sum()) == 603 and not stored[~nd.mask].any()      # dropped pair count 0
    assert nd.used().nnz == nd.nnz
    assert nk.used().nnz == 0 and nk.n_used == 603 and nk.nnz > 30000                                  # nnz_used = 0


def test_boundaries_fall_where_the_names_say():
    lds, gather, tail, tall = (C.case(x) for x in ("map_lds_k16", "map_gather_k32", "tail_word", "tall_scatter"))
    assert C.MAP_LDS_MAX_COLS == 196608
    assert C.map_in_lds(lds.n) and not C.map_in_lds(lds.n + 1) and not C.map_in_lds(gather.n) and gather.n == lds.n + 1
    assert lds.n % 32 == 0 and gather.n % 32 == 1 and tail.n % 32 == 7            # a full last word, and partial ones
    assert C.key_bits(lds.n_used) == 16 and C.key_bits(gather.n_used) == 17 and gather.n_used == lds.n_used + 1
    assert C.at_route(lds.n_used, True, 2) == "FormatFromCompacted" and C.at_route(gather.n_used, True, 2) == "CompactedTransposed"
    assert C.at_route(lds.n_used, True, 2, at_sort=True) == C.at_route(lds.n_used, False, 2) == C.at_route(lds.n_used, True, 1) == "CompactedTransposed"
    # the sort of the dropped (column, value) pairs takes its key width from n, the transposition from n_used
    for c in (lds, gather, tail, tall):
        assert 0 < c.used().nnz < c.nnz
    assert tall.m > C.COMPACT_WAVES == 8192 and C.scatter_route(tall.m, tall.n_used, tall.used().nnz) and not C.map_in_lds(tall.n)
    assert not any(C.scatter_route(C.case(x).m, C.case(x).n_used, 1) for x in C.RANDOM_CASES)
    # the entries reach the last kept column, so a key cut to 16 bits (65536 -> 0) cannot go unnoticed
    assert gather.used().indices.max() == 65536 and lds.used().indices.max() == 65535


@pytest.mark.parametrize("name", tuple(C.SHAPES))
def test_sums_are_exact_in_f32(name):
    c = C.case(name)
    s, q = C.column_sums(c)
    print(f"{name}: nnz {c.nnz}, kept {c.used().nnz}, largest |column sum| {np.abs(s).max():.0f}, sum of squares {q.max():.0f}")
    assert np.abs(s).max() * c.m < 2 ** 24 and q.max() * c.m < 2 ** 24 * c.m      # (sum / m: an f32 holds it; so it does the squares' sum)
    mean = s / c.m
    assert np.array_equal(mean.astype(np.float32).astype(np.float64), mean)


@pytest.mark.parametrize("name,k,centred", [(x, C.k_of(x), True) for x in C.RANDOM_CASES] + [(C.LANCZOS_CASE, C.K_LANCZOS, False)])
def test_gap_is_at_least_two(name, k, centred):
    c = C.case(name)
    s, g = C.gap(c, k, centred)
    print(f"{name}{' centred' if centred else ''}: sigma {np.array2string(s, precision=1)}  sigma_{k} / sigma_{k + 1} = {g:.3f}")
    assert g >= 2.0
    assert np.all(s[:k - 1] / s[1:k] > 1.02)


def test_gap_helper_against_the_dense_answer():
    c = C.case("tail_word")
    D = c.used().toarray()
    for centred in (False, True):
        want = np.linalg.svd(D - D.mean(0) if centred else D, compute_uv=False)
        s, g = C.gap(c, C.K_RANDOM, centred)
        np.testing.assert_allclose(s, want[:C.K_RANDOM + 1], rtol=1e-10)


@pytest.mark.parametrize("name", tuple(C.SHAPES))
def test_oracle_statistics_are_the_exact_ones_bit_for_bit(name):
    """the oracle's mean is sum / m and its total variance the sequential f64 formula of finish_statistics, to the last bit:
    the GPU test can hold the library to either"""
    c = C.case(name)
    s, _ = C.column_sums(c)
    cols = np.flatnonzero(c.mask)
    mean, tv = O.mean_and_total_var(c.ptr, c.idx, c.val, c.m, c.n, True, cols)
    assert np.array_equal(mean, s / c.m)
    assert float(tv) == C.total_variance(c)
    mean32, _ = O.mean_and_total_var(c.ptr, c.idx, c.val.astype(np.float32), c.m, c.n, True, cols[:1])
    assert mean32.dtype == np.float32 and np.array_equal(mean32.astype(np.float64), s / c.m)
    cu, o2m = O.mask_index_maps(c.mask)
    assert np.array_equal(cu, cols.astype(np.uint64)) and np.array_equal(o2m[cols], np.arange(len(cols))) and (o2m[~c.mask] == -1).all()

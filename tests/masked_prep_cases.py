"""Host-only helper of tests/test_gpu_masked_prep.py: the matrices and masks that put the preparation of a masked fit
(single-algebra_amd/csrc/prep.hip compact_columns, sums_by_column, transpose_csr; engine.cpp plan_preparation) exactly at the
sizes where it changes behaviour, and their exact references.  Needs neither a GPU nor the library:
tests/test_masked_prep_cases_cpu.py holds every case to its conditions on the CPU.

The matrices are integer "ledgers": m is a power of two and every stored value a small integer, so every column sum, sum of
squares and mean (sum / m) is exact in f32 and f64 whatever the order of the additions.  Each route of the preparation has to
deliver them bit for bit, and two routes that hand the sweeps the same operator have to give the same bytes."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sapca_oracle as O

# ---- the boundaries, restated (file: the line each mirrors)
WAVE = 64                            # prep.hip: constexpr int WAVE = 64 (a wave walks a row)
MAP_LDS_BYTES = 48 * 1024            # prep.hip compact_columns: if (lds > 48 * 1024) { words = 0; lds = 0; }
#                                      with words = (A.cols + 31) / 32 and lds = 2 * words * sizeof(uint32_t)
MAP_LDS_MAX_COLS = MAP_LDS_BYTES // 8 * 32    # = 196608: the last n whose column map (bits[] + before[]) stays in LDS
WRITE_BATCH = 4 * WAVE               # prep.hip write_kept_kernel: for (base = e0; base < e1; base += 4 * WAVE)
COUNT_BATCH = 8 * WAVE               # prep.hip count_kept_kernel: for (eb = ptr[r] + lane; eb < e1; eb += 8 * WAVE)
COMPACT_GRID = 2048                  # prep.hip compact_columns: grid_for(A.rows * WAVE, 256, 2048): 4 waves a workgroup, so the
COMPACT_WAVES = COMPACT_GRID * 256 // WAVE    # grid-stride loop over rows turns with more than 8192 rows
KEY16_MAX_COLS = 1 << 16             # prep.hip transpose_csr: while ((1ll << bits) < A.cols) ++bits;  if (bits <= 16) / k16 = bits <= 16
DIRECT_MAX_USED = 65536              # engine.cpp plan_preparation: bucket_route && n_used <= 65536 ? FormatFromCompacted : CompactedTransposed
SCATTER_MIN_ROWS = 4096              # engine.cpp plan_preparation: lz_scatter = Lanczos && n_used <= m && m >= 4096 && nnz > 0
SCATTER_BYTES = 150 * 1024           # scatter.hip scatter_fits: cols * sizeof(long long) <= kScatterLds

# the lengths of the leading rows: nothing, one entry, either side of a wave (64), of write_kept_kernel's batch (256) and its
# second and fourth trips, of count_kept_kernel's batch (512) and its second and fourth trips
EDGE_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
# (length, where): "any" draws from every column, "dropped" / "kept" from the columns the mask drops / keeps alone
LENGTHS = tuple((n, "any") for n in EDGE_LENGTHS) + ((300, "dropped"), (300, "kept"))
DROPPED_ROW, KEPT_ROW = len(EDGE_LENGTHS), len(EDGE_LENGTHS) + 1
HOT = 64                             # hot columns per row cluster
CLUSTERS = 4                         # row r belongs to cluster r mod 4; its hot entries hold 8 - cluster


def map_in_lds(n):
    """prep.hip compact_columns: does the column map of n columns stay in LDS?"""
    return 2 * ((n + 31) // 32) * 4 <= MAP_LDS_BYTES


def key_bits(cols):
    """prep.hip transpose_csr: the radix sort's key width for an operator of `cols` columns"""
    bits = 1
    while (1 << bits) < cols:
        bits += 1
    return bits


def at_route(n_used, f32, variant, at_sort=False):
    """engine.cpp plan_preparation: where a masked randomized fit takes A^T from"""
    bucket = f32 and variant == 2        # staged_sweep_ldp: variant 1 never stages, variant 2 always does
    return "FormatFromCompacted" if bucket and n_used <= DIRECT_MAX_USED and not at_sort else "CompactedTransposed"


def scatter_route(m, n_used, nnz):
    return 0 < n_used <= m and m >= SCATTER_MIN_ROWS and nnz > 0 and n_used * 8 <= SCATTER_BYTES


# ---- structured masks
PATTERNS = ("words_dropped", "words_kept", "bit0_kept", "bit31_kept", "bit0_dropped", "alternating")
_SLOT = 4      # words per pattern slot: a pattern takes up to three of them, the fourth keeps neighbours apart


def _force(mask, kind, w):
    """writes the pattern into the words from w on and returns the columns it owns"""
    c = 32 * w
    if kind == "words_dropped":
        mask[c:c + 96] = False
        return c, c + 96
    if kind == "words_kept":
        mask[c:c + 96] = True
        return c, c + 96
    if kind in ("bit0_kept", "bit31_kept", "bit0_dropped"):
        for i in range(2):
            word = np.zeros(32, bool) if kind != "bit0_dropped" else np.ones(32, bool)
            word[31 if kind == "bit31_kept" else 0] = kind != "bit0_dropped"
            mask[c + 32 * i:c + 32 * i + 32] = word
        return c, c + 64
    assert kind == "alternating"
    mask[c:c + 64] = np.arange(64) % 2 == 1
    return c, c + 64


def structured_mask(n, n_used, seed, first, last):
    """(mask, {pattern: first word}): a random mask with n_used kept columns of n that holds every pattern of PATTERNS at a
    whole-word position, column 0 set to `first` and column n - 1 to `last`; random positions outside the patterns are then
    flipped until exactly n_used columns are kept"""
    rng = np.random.default_rng(seed)
    mask = np.zeros(n, bool)
    mask[rng.choice(n, n_used, replace=False)] = True
    whole = n // 32
    slots = rng.choice(np.arange(1, (whole - 1) // _SLOT), len(PATTERNS), replace=False)    # (word 0 and the last words stay free)
    where, fixed = {}, np.zeros(n, bool)
    for kind, slot in zip(PATTERNS, slots):
        w = int(slot) * _SLOT
        lo, hi = _force(mask, kind, w)
        fixed[lo:hi] = True
        where[kind] = w
    mask[0], mask[n - 1] = first, last
    fixed[0] = fixed[n - 1] = True
    excess = int(mask.sum()) - n_used
    free = np.flatnonzero(~fixed & (mask if excess > 0 else ~mask))
    mask[rng.choice(free, abs(excess), replace=False)] = excess < 0
    assert int(mask.sum()) == n_used
    return mask, where


def pattern_present(mask, kind, w):
    """the CPU test's reading of a pattern, written apart from _force"""
    words = mask[32 * w:32 * w + 96].reshape(3, 32)
    if kind == "words_dropped":
        return not words.any()
    if kind == "words_kept":
        return bool(words.all())
    two = words[:2]
    if kind == "bit0_kept":
        return bool(two[:, 0].all()) and int(two.sum()) == 2
    if kind == "bit31_kept":
        return bool(two[:, 31].all()) and int(two.sum()) == 2
    if kind == "bit0_dropped":
        return not two[:, 0].any() and int(two.sum()) == 62
    return bool(np.array_equal(two.ravel(), np.arange(64) % 2 == 1))


# ---- the ledger
def ledger(m, n, mask, seed, lengths=LENGTHS, rest=(20, 120), hot_rows=None):
    """(ptr, idx, val) of an m x n CSR of small integers, int64 / int64 / float64, columns ascending within a row.

    Row r belongs to cluster r mod 4.  A cluster owns 64 hot columns drawn from the kept ones (fewer where the mask keeps
    fewer than 256; all of them where it keeps fewer than 4); a hot entry is present with probability 0.7 and holds
    8 - cluster.  Background entries hold +1 or -1 on uniformly drawn other columns.  Row r < len(lengths) has exactly
    lengths[r][0] entries, drawn from every column, from the dropped columns or from the kept columns alone (lengths[r][1];
    cut to the columns there are); the other rows have between rest[0] and rest[1]: the hot entries first, background up
    to the length.  hot_rows: only that many leading rows hold hot entries (default: all)."""
    assert m & (m - 1) == 0, "a power of two: sum / m is exact"
    hot_rows = m if hot_rows is None else hot_rows
    rng = np.random.default_rng(seed)
    mask = np.asarray(mask, bool)
    kept, dropped = np.flatnonzero(mask), np.flatnonzero(~mask)
    h = min(HOT, len(kept) // CLUSTERS)
    perm = rng.permutation(len(kept))
    hot = [np.sort(kept[perm[c * h:(c + 1) * h]]) if h else kept for c in range(CLUSTERS)]
    everything = np.arange(n)
    cols, vals, counts = [], [], np.zeros(m, np.int64)
    for r in range(m):
        c = r % CLUSTERS
        length, where = lengths[r] if r < len(lengths) else (int(rng.integers(rest[0], rest[1] + 1)), "any")
        pool = {"any": everything, "kept": kept, "dropped": dropped}[where]
        length = min(length, len(pool))
        # (a "kept" / "dropped" row takes the first and the last such column: entries reach both ends of either numbering)
        must = np.unique(pool[[0, -1]]) if where != "any" and length >= 2 else pool[:0]
        hc = hot[c][rng.random(len(hot[c])) < 0.7] if where != "dropped" and r < hot_rows else hot[c][:0]
        hc = hc[~np.isin(hc, must)]
        if len(hc) > length - len(must):
            hc = np.sort(rng.choice(hc, length - len(must), replace=False))
        need = length - len(hc) - len(must)
        taken = np.concatenate([hc, must])
        if need:
            extra = rng.choice(pool, min(len(pool), need + len(taken)), replace=False)     # (enough to lose the taken ones among them)
            extra = extra[~np.isin(extra, taken)][:need]
        else:
            extra = hc[:0]
        assert len(extra) == need
        extra = np.concatenate([must, extra])
        cc = np.concatenate([hc, extra])
        vv = np.concatenate([np.full(len(hc), 8.0 - c), rng.choice([-1.0, 1.0], len(extra))])
        o = np.argsort(cc)
        cols.append(cc[o])
        vals.append(vv[o])
        counts[r] = length
    ptr = np.zeros(m + 1, np.int64)
    ptr[1:] = np.cumsum(counts)
    return ptr, np.concatenate(cols).astype(np.int64), np.concatenate(vals)


# ---- the cases
# name: (m, n, n_used, first column kept, last column kept, seed)
SHAPES = {
    "map_lds_k16": (512, MAP_LDS_MAX_COLS, KEY16_MAX_COLS, True, False, 11),           # last n in LDS; 16-bit keys; FormatFromCompacted
    "map_gather_k32": (512, MAP_LDS_MAX_COLS + 1, KEY16_MAX_COLS + 1, False, True, 12),   # o2m gathered; 32-bit keys; CompactedTransposed
    "tail_word": (512, 4103, 2000, True, True, 13),                                     # 4103 = 128 * 32 + 7: a last word of 7 columns
    "nothing_dropped": (512, 4103, 3500, False, True, 14),
    "all_true": (512, 4103, 4103, True, True, 15),
    "one_column": (512, 4103, 1, False, False, 16),
    "tall_scatter": (16384, MAP_LDS_MAX_COLS + 1, 4000, True, False, 17),              # Lanczos scatter route; 16384 rows > 8192 waves
}
REST = {"tall_scatter": (10, 30)}
# tall_scatter: hot entries in its first 512 rows alone, as many as the other cases have -- 16384 rows of them would put the hot
# columns' sums at 2e4, and max |sum| * m has to stay below 2^24
HOT_ROWS = {"tall_scatter": 512}
K_RANDOM, K_LANCZOS = 3, 4         # centred randomized fits / uncentred Lanczos fits (the issue's spectra: gaps 2.9 and 2.8)
ONE_COLUMN = 2015                  # bit 31 of word 62


class Case:
    __slots__ = ("name", "m", "n", "n_used", "mask", "where", "ptr", "idx", "val")

    def csr(self, dtype=np.float64):
        return sp.csr_matrix((self.val.astype(dtype), self.idx, self.ptr), shape=(self.m, self.n))

    def used(self):
        """the operator the fit sees: the kept columns, renumbered (the oracle's MaskedCSRMatrix::new)"""
        p, i, v, nu = O.masked_csr(self.ptr, self.idx, self.val, self.n, self.mask)
        return sp.csr_matrix((v, i, p), shape=(self.m, nu))

    @property
    def nnz(self):
        return len(self.val)


@functools.lru_cache(maxsize=None)
def case(name):
    c = Case()
    c.name = name
    if name == "nothing_kept":
        # nothing_dropped's matrix under the complement of its mask: the kept columns store no entry (nnz_used = 0)
        nd = case("nothing_dropped")
        c.m, c.n, c.mask, c.where = nd.m, nd.n, ~nd.mask, {}
        c.n_used = int(c.mask.sum())
        c.ptr, c.idx, c.val = nd.ptr, nd.idx, nd.val
        return c
    m, n, n_used, first, last, seed = SHAPES[name]
    c.m, c.n, c.n_used = m, n, n_used
    if name == "all_true":
        c.mask, c.where = np.ones(n, bool), {}
    elif name == "one_column":
        c.mask, c.where = np.zeros(n, bool), {}
        c.mask[ONE_COLUMN] = True
    else:
        c.mask, c.where = structured_mask(n, n_used, seed, first, last)
    if name == "nothing_dropped":
        # a ledger over the kept columns alone, spread over them in ascending order: the mask is true on every column that
        # stores an entry and false on 603 empty ones (whole words, bit 0, bit 31 among them); no (column, value) pair is dropped
        ptr, idx, val = ledger(m, n_used, np.ones(n_used, bool), seed)
        c.ptr, c.idx, c.val = ptr, np.flatnonzero(c.mask)[idx], val
    else:
        c.ptr, c.idx, c.val = ledger(m, n, c.mask, seed, rest=REST.get(name, (20, 120)), hot_rows=HOT_ROWS.get(name))
    return c


RANDOM_CASES = ("map_lds_k16", "map_gather_k32", "tail_word", "nothing_dropped", "all_true", "one_column")
LANCZOS_CASE = "tall_scatter"
ROUTE_CASES = ("map_lds_k16", "map_gather_k32", "tail_word")


def k_of(name, lanczos=False):
    return 1 if name == "one_column" else K_LANCZOS if lanczos else K_RANDOM


# ---- exact statistics
def column_sums(c):
    """(sum, sum of squares) of every column of the case's matrix: integers in f64, exact"""
    s = np.bincount(c.idx, weights=c.val, minlength=c.n)
    q = np.bincount(c.idx, weights=c.val * c.val, minlength=c.n)
    assert np.array_equal(s, np.rint(s)) and np.array_equal(q, np.rint(q))
    return s, q


def total_variance(c):
    """engine.cpp finish_statistics, in its order: over cols_to_use ascending, mean = sum / m,
    total += (sumsq - mean * sum) / (m - 1), all f64"""
    s, q = column_sums(c)
    mg, total = float(c.m), 0.0
    for j in np.flatnonzero(c.mask):
        mean = s[j] / mg
        total += (q[j] - mean * s[j]) / (mg - 1.0)
    return total


# ---- the gap of the operator a fit sees
def gap(c, k, centred):
    """(sigma[:k + 1], sigma_k / sigma_{k+1}) of the compacted matrix A (centred: of A - 1 mu^T) from the Gram matrix of its
    smaller side; m x m as A A^T - (A mu) 1^T - 1 (A mu)^T + (mu^T mu) 1 1^T, formed from the sparse A -- m x n_used is never
    densified.  More than 2048 on both sides (uncentred only): scipy's svds.  inf where the operator has only k columns."""
    A = c.used()
    m, nu = A.shape
    if min(m, nu) <= k:
        s = np.linalg.svd(A.toarray() - (A.toarray().mean(0) if centred else 0.0), compute_uv=False)[:k]
        return s, np.inf
    if min(m, nu) > 2048:
        assert not centred
        s = np.sort(spla.svds(A, k=k + 1, tol=0, random_state=0)[1])[::-1]
        return s, float(s[k - 1] / s[k])
    if m <= nu:
        G = (A @ A.T).toarray()
        if centred:
            mu = np.asarray(A.mean(0)).ravel()
            amu = A @ mu
            G = G - amu[:, None] - amu[None, :] + float(mu @ mu)
    else:
        G = (A.T @ A).toarray()
        if centred:
            mu = np.asarray(A.mean(0)).ravel()
            G = G - m * np.outer(mu, mu)
    w = np.linalg.eigvalsh(G)[::-1]
    s = np.sqrt(np.maximum(w[:k + 1], 0.0))
    return s, float(s[k - 1] / s[k])

"""The preparation of a masked fit at its map, key and route edges (csrc/prep.hip compact_columns, sums_by_column,
transpose_csr; engine.cpp plan_preparation), on the integer ledgers of tests/masked_prep_cases.py (held to their conditions on
the CPU by tests/test_masked_prep_cases_cpu.py).

Every fit injects Omega and reads a DeviceCsr, so every route computes its own statistics.  Checked:
  (a) exactly, with no tolerance: mean_ = T(sum / m) at full width, the mask index maps, total_variance_() = the sequential f64
      formula of finish_statistics -- the sums are integers, so every order of additions gives the same bits;
  (b) against oracle.fit(..., mask=...) with the same Omega at the tolerances of test_masked_randomized_fit_vs_oracle (f64:
      sigma rtol 1e-9, angle 1e-8; f32: 1e-4, 1e-4) and test_g6_lanczos_* (sigma 1e-5, angle 1e-4); fit_transform scores
      against O.transform_masked_fast to 1e-9 (f64) / 2e-4 (f32) of their maximum.  One entry of 5..8 misplaced among sigma
      near 400 moves an f64 sigma by 1e-4 or so: (b) in f64 is the per-entry check, (a) the per-column one;
  (c) route against route: the same bytes;
  (d) the degenerate masks; (e) fit + transform against fit_transform."""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import masked_prep_cases as C
import sapca
import sapca_oracle as O
from sapca import _lib as L
from sapca import PowerIterationNormalizer as PIN
from sapca import SVDMethod, synth

pytestmark = pytest.mark.gpu

P, Q = 8, 3                                # oversampling and power iterations: those of test_masked_randomized_fit_vs_oracle
TOL = {np.float64: (1e-9, 1e-8, 1e-9), np.float32: (1e-4, 1e-4, 2e-4)}      # dtype -> (sigma rtol, angle, scores / max)
TOL_LANCZOS = (1e-5, 1e-4)                                                   # test_g6_lanczos_*: sigma rtol, angle
BOTH = [np.float64, np.float32]
SWITCHES = ("SAPCA_AT_SORT", "SAPCA_AT_NATURAL", "SAPCA_TRANSPOSE_GATHER", "SAPCA_MASK_STATS_INLINE", "SAPCA_LANCZOS_TRANSPOSE")

Fit = collections.namedtuple("Fit", "sigma comps scores mean total_var est label")


@functools.lru_cache(maxsize=None)
def _device(name, dtype):
    c = C.case(name)
    t = torch.float64 if dtype == np.float64 else torch.float32
    return sapca.DeviceCsr(torch.from_numpy(c.ptr).cuda(), torch.from_numpy(c.idx.astype(np.int32)).cuda(),
                           torch.from_numpy(c.val).to(t).cuda(), (c.m, c.n))


@functools.lru_cache(maxsize=None)
def _omega(name):
    return synth.gaussian_panel(C.case(name).n_used, C.k_of(name) + P, 5).numpy()


@functools.lru_cache(maxsize=None)
def _oracle(name, lanczos=False):
    """the f64 oracle's fit of the case (its values are integers: the f32 fits see the same matrix); computed once, read only"""
    c = C.case(name)
    if lanczos:
        return O.fit(c.ptr, c.idx, c.val, c.m, c.n, n_components=C.k_of(name, True), method="LANCZOS", mask=c.mask)
    return O.fit(c.ptr, c.idx, c.val, c.m, c.n, n_components=C.k_of(name), n_oversamples=P, n_power_iterations=Q,
                 omega=_omega(name), mask=c.mask)


def _estimator(name, variant=2, lanczos=False, masked=True):
    c = C.case(name)
    b = sapca.MaskedSparsePCABuilder.new().mask(c.mask) if masked else sapca.SparsePCABuilder.new()
    if lanczos:
        return b.n_components(C.k_of(name, True)).svd_method(SVDMethod.Lanczos()).build()
    return b.n_components(C.k_of(name)).spmm_variant(variant).svd_method(SVDMethod.Random(P, Q, PIN.QR)).build().set_omega(_omega(name))


def _set_mask(est, mask):
    m8 = np.ascontiguousarray(mask, dtype=np.uint8)
    L.check(est._h, L.load().sapca_set_mask(est._h, m8.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.c_size_t(m8.size)))
    est._mask = np.asarray(mask, dtype=bool).copy()


def _fit(name, dtype, variant=2, lanczos=False, masked=True, est=None, note=""):
    est = est or _estimator(name, variant, lanczos, masked)
    t = est.fit_transform(_device(name, dtype))
    label = f"{name} {np.dtype(dtype).name} {'lanczos' if lanczos else f'variant {variant}'}{note}"
    return Fit(est.singular_values_(np.float64), est.components_(np.float64), t.cpu().numpy().astype(np.float64),
               est.mean_(np.float64), est.total_variance_(), est, label)


def _switched(monkeypatch, name, dtype, *switches, lanczos=False):
    """one fit with exactly the given switches set (they need the debug_switches fixture) and the rows in their natural order"""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s in switches:
        assert s in SWITCHES
        monkeypatch.setenv(s, "1")
    monkeypatch.setenv("SAPCA_NO_ROWSORT", "1")
    return _fit(name, dtype, 2, lanczos, note=f" [{' '.join(s[6:] for s in switches) or 'default'}]")


def _exact_statistics(f, name, dtype):
    """(a)"""
    c = C.case(name)
    s, _ = C.column_sums(c)
    T = np.float32 if dtype == np.float32 else np.float64
    np.testing.assert_array_equal(f.mean, (s / c.m).astype(T).astype(np.float64), err_msg=f.label)      # full width
    cols, o2m = f.est.mask_index_maps()
    want_cols, want_o2m = O.mask_index_maps(c.mask)
    assert cols.dtype == want_cols.dtype and o2m.dtype == want_o2m.dtype
    np.testing.assert_array_equal(cols, want_cols, err_msg=f.label)
    np.testing.assert_array_equal(o2m, want_o2m, err_msg=f.label)
    assert f.total_var == C.total_variance(c), (f.label, f.total_var, C.total_variance(c))


def _against_oracle(f, name, dtype, lanczos=False):
    """(b)"""
    c = C.case(name)
    want = _oracle(name, lanczos)
    srel, ang, trel = TOL[dtype]
    if lanczos:
        srel, ang = TOL_LANCZOS
    k = f.sigma.size
    assert f.comps.shape == (k, c.n_used) and f.mean.shape == (c.n,) and f.scores.shape == (c.m, k)
    angle = O.subspace_angle(f.comps, want.components)
    tw = O.transform_masked_fast(c.ptr, c.idx, c.val, c.m, c.n, f.comps, f.mean, True, c.mask)
    tmax = float(np.abs(tw).max())
    print(f"{f.label}: sigma rel err {np.max(np.abs(f.sigma / want.singular_values[:k] - 1)):.3e}  angle {angle:.3e}"
          f"  scores {np.abs(f.scores - tw).max() / tmax:.3e} of their maximum")
    np.testing.assert_allclose(f.sigma, want.singular_values[:k], rtol=srel, err_msg=f.label)
    assert angle < ang, (f.label, angle)
    np.testing.assert_allclose(f.scores, tw, atol=trel * tmax, err_msg=f.label)


def _same_bytes(a, b):
    for x, y, what in zip(a[:4], b[:4], Fit._fields):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {a.label} vs {b.label}")
    assert a.total_var == b.total_var, (a.label, b.label)


# ------------------------------------------------------------------ (a) + (b)
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("name", ["map_lds_k16", "map_gather_k32", "tail_word", "nothing_dropped"])
def test_randomized_fit_statistics_exactly_and_operator_against_the_oracle(name, dtype, variant):
    """map_lds_k16 (n = 196608, n_used = 65536): the last column map that stays in LDS (2 * 6144 words = 48 KiB), 16-bit sort
    keys, f32 variant 2 on FormatFromCompacted.  map_gather_k32 (196609, 65537): o2m gathered from memory, 17-bit keys in 32-bit
    words, f32 variant 2 on CompactedTransposed, the last kept column (compact index 65536: 0 once cut to 16 bits) alone in the
    last word.  tail_word (4103, 2000): a last word of 7 columns.  nothing_dropped: no (column, value) pair is dropped, the
    memset branch of sums_by_column.  Variant 1 sweeps the compacted CSR and its natural-order transposition with the row
    kernel, variant 2 the tile-major formats.  All of them: rows of 0 .. 2049 entries around the 256- and 512-entry batches of
    write_kept_kernel and count_kept_kernel, a row dropped whole and one kept whole, mask words that are empty, full, bit 0 or
    bit 31 alone."""
    c = C.case(name)
    assert C.map_in_lds(c.n) == (name != "map_gather_k32") and (C.key_bits(c.n_used) > 16) == (name == "map_gather_k32")
    f = _fit(name, dtype, variant)
    _exact_statistics(f, name, dtype)
    _against_oracle(f, name, dtype)


@pytest.mark.parametrize("dtype", BOTH)
def test_lanczos_on_the_scatter_route_behind_a_compaction_of_more_rows_than_waves(dtype):
    """tall_scatter (16384 x 196609, 4000 kept): 2048 workgroups of four waves walk 16384 rows, two turns of the grid-stride loop
    of both compaction kernels, o2m gathered from memory, max |a| = 8 gathered by write_kept_kernel for the fixed-point scales
    (16384 * 8 * 2^43 = 2^60: the integer sums of scatter.hip are exact), the masked-out columns' statistics straight from A."""
    c = C.case(C.LANCZOS_CASE)
    assert C.scatter_route(c.m, c.n_used, c.used().nnz) and c.m > C.COMPACT_WAVES
    f = _fit(C.LANCZOS_CASE, dtype, lanczos=True)
    assert f.est.timings().lanczos_steps >= C.K_LANCZOS
    _exact_statistics(f, C.LANCZOS_CASE, dtype)
    _against_oracle(f, C.LANCZOS_CASE, dtype, lanczos=True)


# ------------------------------------------------------------------ (c)
@pytest.mark.parametrize("name", C.ROUTE_CASES)
def test_f32_routes_to_the_transposed_format_give_the_same_bytes(debug_switches, monkeypatch, name):
    """f32, variant 2, natural row order: the default (map_lds_k16, tail_word: the builder on the compacted matrix,
    FormatFromCompacted; map_gather_k32: its transposition, 32-bit keys, rows packed tile-major), SAPCA_AT_SORT (the
    transposition everywhere: 16-bit keys at 65536 columns), with SAPCA_AT_NATURAL (natural rows through pack_rows_kernel), and
    SAPCA_MASK_STATS_INLINE (the dropped pairs' sums in front of the first sweep).  The kept columns' sums come from the
    builder's histogram pass or from row sums of the transposed CSR: integers either way, so the same means, the same
    format and the same fit to the last bit."""
    base = _switched(monkeypatch, name, np.float32)
    _exact_statistics(base, name, np.float32)
    _against_oracle(base, name, np.float32)
    for sw in (("SAPCA_AT_SORT",), ("SAPCA_AT_SORT", "SAPCA_AT_NATURAL"), ("SAPCA_MASK_STATS_INLINE",)):
        f = _switched(monkeypatch, name, np.float32, *sw)
        _exact_statistics(f, name, np.float32)
        _same_bytes(f, base)


@pytest.mark.parametrize("name", C.ROUTE_CASES)
def test_f64_routes_to_the_transposed_csr_give_the_same_bytes(debug_switches, monkeypatch, name):
    """f64, variant 2, natural row order: the default (12-byte payload, tile-major rows, 16-bit keys up to 65536 kept columns),
    SAPCA_AT_NATURAL (pack_rows64_kernel), SAPCA_TRANSPOSE_GATHER (permutation + gather; natural rows: plan_preparation) and
    SAPCA_MASK_STATS_INLINE."""
    base = _switched(monkeypatch, name, np.float64)
    _exact_statistics(base, name, np.float64)
    _against_oracle(base, name, np.float64)
    for sw in (("SAPCA_AT_NATURAL",), ("SAPCA_TRANSPOSE_GATHER",), ("SAPCA_MASK_STATS_INLINE",)):
        f = _switched(monkeypatch, name, np.float64, *sw)
        _exact_statistics(f, name, np.float64)
        _same_bytes(f, base)


@pytest.mark.parametrize("dtype", BOTH)
def test_lanczos_scatter_route_against_the_transposed_operator(debug_switches, monkeypatch, dtype):
    """tall_scatter on the scatter route and with SAPCA_LANCZOS_TRANSPOSE=1 (compaction, transposition, the dropped pairs'
    sums): mean_ and total_variance_ to the bit (fixed-point sums of integers against f64 sums of integers), sigma to 1e-5."""
    a = _switched(monkeypatch, C.LANCZOS_CASE, dtype, lanczos=True)
    b = _switched(monkeypatch, C.LANCZOS_CASE, dtype, "SAPCA_LANCZOS_TRANSPOSE", lanczos=True)
    for f in (a, b):
        _exact_statistics(f, C.LANCZOS_CASE, dtype)
    np.testing.assert_array_equal(a.mean, b.mean)
    assert a.total_var == b.total_var
    np.testing.assert_allclose(a.sigma, b.sigma, rtol=1e-5)
    _against_oracle(b, C.LANCZOS_CASE, dtype, lanczos=True)


# ------------------------------------------------------------------ (d)
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("dtype", BOTH)
def test_a_mask_of_ones_is_the_unmasked_estimator(dtype, variant):
    """all_true: compaction and (column, value) pairs with nothing to drop, against SparsePCA on the same matrix"""
    f = _fit("all_true", dtype, variant)
    _exact_statistics(f, "all_true", dtype)
    _against_oracle(f, "all_true", dtype)
    u = _fit("all_true", dtype, variant, masked=False, note=" unmasked")
    srel, ang, _ = TOL[dtype]
    np.testing.assert_array_equal(f.mean, u.mean)
    assert f.total_var == u.total_var
    np.testing.assert_allclose(f.sigma, u.sigma, rtol=srel)
    assert O.subspace_angle(f.comps, u.comps) < ang


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("dtype", BOTH)
def test_a_mask_that_keeps_one_column(dtype, variant):
    """one_column (bit 31 of word 62): k = 1, sigma_1 = the norm of the centred column, the component is +1"""
    c = C.case("one_column")
    f = _fit("one_column", dtype, variant)
    _exact_statistics(f, "one_column", dtype)
    col = np.asarray(c.used().todense()).ravel()
    srel, _, trel = TOL[dtype]
    np.testing.assert_allclose(f.sigma, [np.linalg.norm(col - col.mean())], rtol=srel)
    np.testing.assert_allclose(f.sigma, _oracle("one_column").singular_values[:1], rtol=srel)
    np.testing.assert_allclose(f.comps, [[1.0]], rtol=0, atol=1e-12 if dtype == np.float64 else 1e-6)
    tw = O.transform_masked_fast(c.ptr, c.idx, c.val, c.m, c.n, f.comps, f.mean, True, c.mask)
    np.testing.assert_allclose(f.scores, tw, atol=trel * np.abs(tw).max())


@pytest.mark.parametrize("dtype", BOTH)
def test_a_mask_that_keeps_only_empty_columns_is_the_rank_error_and_leaves_the_handle_sound(dtype):
    """nothing_kept (nothing_dropped's matrix under the complement of its mask: 603 kept columns, nnz_used = 0).  The path, as
    read: count_kept_kernel writes zeros, write_kept_kernel drops every pair; transpose_csr returns from its nnz == 0 branch
    behind a memset of the row offsets (no sort, no launch sized by nnz); row_sums and spmv_launch size their grids by rows
    (603 and 512), spmv_narrow_indices returns on nnz == 0; nothing divides by an entry count.  at_format_direct (f32 staged
    sweeps) returns before it touches the builder, and quad_geometry / eligible refuse an empty operator.  The Lanczos fit
    of the zero operator is the documented rank error (include/sapca.h, deviation 5), the mask maps are still answered, and
    the handle then fits tail_word's mask to the bytes of a fresh handle."""
    nk, tw = C.case("nothing_kept"), C.case("tail_word")
    assert nk.used().nnz == 0 and (nk.m, nk.n) == (tw.m, tw.n)
    est = sapca.MaskedSparsePCABuilder.new().mask(nk.mask).n_components(2).svd_method(SVDMethod.Lanczos()).build()
    with pytest.raises(L.SapcaError, match="SVD computation failed") as e:
        est.fit(_device("nothing_dropped", dtype))
    assert e.value.status == L.ERR_SVD
    cols, o2m = est.mask_index_maps()
    want_cols, want_o2m = O.mask_index_maps(nk.mask)
    assert np.array_equal(cols, want_cols) and np.array_equal(o2m, want_o2m)
    _set_mask(est, tw.mask)
    again = _fit("tail_word", dtype, est=est, note=" on the handle that failed")
    fresh = _fit("tail_word", dtype, est=sapca.MaskedSparsePCABuilder.new().mask(tw.mask).n_components(2).svd_method(SVDMethod.Lanczos()).build())
    _same_bytes(again, fresh)
    _exact_statistics(again, "tail_word", dtype)


# ------------------------------------------------------------------ (e)
def test_fit_then_transform_is_fit_transform_past_both_boundaries():
    """map_gather_k32 in f64: fit, then transform of the same matrix (the projection's own use of the prepared operator), against
    fit_transform"""
    name = "map_gather_k32"
    both = _fit(name, np.float64)
    est = _estimator(name)
    x = _device(name, np.float64)
    est.fit(x)
    t = est.transform(x).cpu().numpy()
    np.testing.assert_array_equal(est.singular_values_(np.float64), both.sigma)
    np.testing.assert_array_equal(est.mean_(np.float64), both.mean)
    np.testing.assert_allclose(t, both.scores, atol=1e-9 * np.abs(both.scores).max())
    _against_oracle(both._replace(scores=t, label=both.label + " fit + transform"), name, np.float64)

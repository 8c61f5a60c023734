"""The panels of tests/dense_tail_cases.py meet the conditions tests/test_gpu_rotation.py and tests/test_gpu_normalize_extras.py
rely on, checked without a GPU: everything the integer cases sum stays exact in f32, the normalised panels have full rank with
a small condition number, every rotation column either ties exactly or has its maximum clear of the product's rounding, the
tie columns tie where they say they do, and the margins of the QR checks are eight times what the reference leaves."""
import numpy as np
import pytest

import dense_tail_cases as C

EXACT_F32 = 2 ** 24


def test_geometry():
    """the shapes the issue names, by the predicates restated from the sources"""
    assert [C.ldk_of(k) for _, k in C.ROTATION_PAIRS] == [16, 32, 64, 48, 112, 112, 128, 160, 272]
    assert [C.pad(l) for l, _ in C.ROTATION_PAIRS] == [16, 32, 64, 64, 112, 128, 128, 256, 320]
    assert C.two_stage(4096, 50) and not C.two_stage(4095, 50) and C.two_stage(4097, 17)
    assert not any(C.two_stage(n, 40) for n in C.FULL_N)          # ldk = 48: the one-kernel route at every n
    assert C.sign_geometry(4097, 50) == (64, 4, 65) and 4097 - 64 * 64 == 1      # 65 blocks, the last one holding one row
    assert C.sign_geometry(16400, 50) == (65, 4, 253) and 16400 - 252 * 65 == 20
    assert C.sign_geometry(16400, 17) == (65, 8, 253)
    assert -(-16368 // 16) == 1023 and -(-16369 // 16) == 1024 == C.GEMM_WIDE_TILES
    assert len(C.rotation_shapes()) == 2 * 10 + 7 * 2
    assert [C.pad(l) for l in C.NORMALIZE_L] == [64, 128, 48, 192]
    assert 8200 > 512 * 16                                        # gram.hip slab_blocks: 512 workgroups of 16 rows a trip
    assert len(C.normalize_shapes()) == 4 * (8 + 3 * 2)


@pytest.mark.parametrize("l,k,n", C.rotation_shapes())
def test_integer_rotations_are_exact(l, k, n):
    P, M = C.integer_rotation(l, k, n)
    assert P.shape == (n, l) and M.shape == (l, k) and np.abs(P).max() <= 8 and np.abs(M).max() <= 3
    assert (np.abs(P) @ np.abs(M)).max() < EXACT_F32
    # an integer column either ties exactly or has a gap of at least one: the product is exact, its bound is zero
    Y = P @ M
    assert np.array_equal(Y.astype(np.float32).astype(np.int64), Y)


@pytest.mark.parametrize("l,k,n", C.TIE_SHAPES)
def test_tie_columns_tie_where_they_say(l, k, n):
    seen = set()
    for P, M, marks in C.tie_panels(l, k, n):
        assert np.abs(P).max() <= 8 and np.abs(M).max() <= 3 and (np.abs(P) @ np.abs(M)).max() < EXACT_F32
        Y = P @ M
        _, signs = C.flip_reference(Y.astype(np.float64))
        for c, (name, r1, r2, s) in marks.items():
            if name == "zero":
                assert not Y[:, c].any() and signs[c] == 1.0
                continue
            top = np.abs(Y[:, c]).max()
            assert np.flatnonzero(np.abs(Y[:, c]) == top).tolist() == [r1, r2]
            assert Y[r1, c] == s * top and Y[r2, c] == -s * top and signs[c] == s
            seen.add((name, s))
    assert seen == {(name, s) for name in C.tie_positions(n, k) for s in (1, -1)}
    if k > 1:
        assert any(name == "zero" for _, _, marks in C.tie_panels(l, k, n) for name, *_ in marks.values())


def test_tie_positions_reach_every_reduction():
    for l, k, n in C.TIE_SHAPES:
        rpb, ng, nblocks = C.sign_geometry(n, k)
        pos = C.tie_positions(n, k)
        assert pos["first and last row"] == (0, n - 1)
        if C.two_stage(n, k):
            r1, r2 = pos["same thread"]
            assert r1 // rpb == r2 // rpb and (r2 - r1) % ng == 0
            r1, r2 = pos["row groups"]
            assert r1 // rpb == r2 // rpb and (r1 % rpb) % ng < (r2 % rpb) % ng
            r1, r2 = pos["row groups, later group first"]
            assert r1 // rpb == r2 // rpb and (r1 % rpb) % ng > (r2 % rpb) % ng
            r1, r2 = pos["blocks"]
            assert r1 // rpb != r2 // rpb
            assert pos["rows 4095 and 4096"] == (4095, 4096)
            if n == 16400:
                for name in ("short last block, same thread", "short last block, row groups"):
                    assert all(r // rpb == nblocks - 1 for r in pos[name])
            else:
                assert n - (nblocks - 1) * rpb == 1 and pos["rows 4095 and 4096"][1] == n - 1    # the one-row last block
        elif n > 256:
            r1, r2 = pos["same thread"]
            assert r1 % 256 == r2 % 256
            r1, r2 = pos["threads, later thread first"]
            assert r1 % 256 > r2 % 256
    assert {C.two_stage(n, k) for _, k, n in C.TIE_SHAPES} == {True, False}
    assert {C.two_stage(n, k) for _, k, n in C.NAN_SHAPES} == {True, False} and {n for _, _, n in C.NAN_SHAPES} == {17, 4097}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gaussian_rotation_has_clear_maxima(dtype):
    """the gap between the two largest |values| of every column is above the error bound of either: no rounding within the
    bound moves the maximum, so the reference's signs are the signs"""
    l, k, n = C.GAUSSIAN_SHAPE
    P, M, Y, absprod = C.gaussian_rotation(dtype)
    assert P.dtype == np.dtype(dtype) and C.two_stage(n, k)
    bound = C.rotation_error_bound(dtype, l, Y, absprod)
    A = np.abs(Y)
    order = np.argsort(-A, axis=0)[:2]
    cols = np.arange(k)
    gap = A[order[0], cols] - A[order[1], cols]
    room = bound[order[0], cols] + bound[order[1], cols]
    print(f"{dtype}: smallest gap {gap.min():.3e}, largest bound on a pair {room.max():.3e}")
    assert np.all(gap > room)


@pytest.mark.parametrize("l,rows,nsplit", C.normalize_shapes())
def test_normalize_cases_are_exact_and_well_conditioned(l, rows, nsplit):
    case = C.normalize_case(l, rows, nsplit)
    slabs, mu, sv, w = case["slabs"], case["mu"], case["sv"], case["w"]
    assert slabs.shape == (nsplit, rows, l) and np.abs(slabs).max() <= 8 and w.min() >= 0 and w.max() <= 3
    partial = np.abs(np.cumsum(slabs, axis=0)).max() + np.abs(np.outer(mu, sv)).max()
    assert partial < EXACT_F32
    for centred in (False, True):
        P = C.panel_of(case, centred)
        assert (w @ np.abs(P)).max() < EXACT_F32 and np.abs(P).sum(0).max() < EXACT_F32     # the column sums as T
        assert (np.abs(P) ** 2).sum(0).max() < 2 ** 53                                       # the Gram in f64 (its diagonal bounds it)
        if rows >= l:
            s = np.linalg.svd(P.astype(np.float64), compute_uv=False)
            assert s[-1] > 0 and s[0] / s[-1] < 100, (centred, s[0] / s[-1])


def test_rank_deficient_case():
    case = C.normalize_case(60, 200, 3, rank_deficient=True)
    for centred in (False, True):
        P = C.panel_of(case, centred)
        assert np.array_equal(P[:, 59], P[:, 3]) and np.linalg.matrix_rank(P.astype(np.float64)) == 59


def test_margins_are_eight_times_the_reference():
    """MARGIN: 8 x the largest figure numpy.linalg.qr in f64, rounded once to the dtype, leaves on the panels of the QR checks"""
    for dtype in ("float64", "float32"):
        worst = [0.0, 0.0]
        for l, rows, nsplit in C.normalize_shapes():
            if rows < l:
                continue
            case = C.normalize_case(l, rows, nsplit)
            for centred in (False, True):
                for w in (case["w"], np.ones(rows, np.int64)):
                    res, vec = C.qr_reference(C.panel_of(case, centred), w, dtype)
                    worst = [max(worst[0], res), max(worst[1], vec)]
        print(f"{dtype}: numpy.linalg.qr leaves residual {worst[0]:.4e}, vec {worst[1]:.4e} (margins {C.MARGIN[dtype]})")
        for got, margin in zip(worst, C.MARGIN[dtype]):      # (room for another LAPACK build's rounding, none for another figure)
            assert 0.5 * margin <= 8 * got <= 2 * margin

"""What the chains of tests/handle_reuse_cases.py claim, asserted from the matrices' own numbers (no GPU): every fit's operator
has sigma_k / sigma_{k+1} >= 2 by a dense SVD (asserted, never skipped), every chain walks the panel widths, leading
dimensions and routes it declares, both up and down, and the special steps are what they say they are.

The geometry is handle_reuse_cases.panel_geometry / staged_floor / lanczos_route / q3_statistic: restatements of
single-algebra_amd/csrc/engine.cpp:34-44, 128, 234-235, 250-251, 628 and 785-788 (change those lines and these change too)."""
import math

import numpy as np
import pytest

import handle_reuse_cases as H

STEPS = [(name, i) for name, ch in H.CHAINS.items() for i in range(len(ch.steps))]
RANDOMIZED = [name for name, ch in H.CHAINS.items() if ch.cfg["method"] == "random"]
LANCZOS = [name for name, ch in H.CHAINS.items() if ch.cfg["method"] == "lanczos"]


@pytest.mark.parametrize("name,i", STEPS, ids=[f"{n}-{i}" for n, i in STEPS])
def test_every_fit_has_a_gap_of_two(name, i):
    """sigma_k / sigma_{k+1} >= 2 of the dense operator the fit sees (mask, scaling, covariates, centring applied), as
    _gapped_case of test_gpu_parity.py certifies its cases: the f32 bars of the GPU tests then apply unchanged"""
    ch = H.CHAINS[name]
    st, k = ch.steps[i], ch.cfg["k"]
    if st.call == "remask_transform":
        mk, prev = H.made(name, i), H.made(name, i - 1)
        assert mk.mask.sum() == prev.mask.sum() and (mk.mask != prev.mask).sum() == 2     # as many columns, other ones
        return
    D = H.operator_seen(name, i)
    assert max(D.shape) <= 5000 and D.size <= 4000 * 1500, D.shape                           # a dense SVD on the CPU stays cheap
    sv = np.linalg.svd(D, compute_uv=False)
    assert k < len(sv), (D.shape, k)
    assert sv[k - 1] >= 2.0 * sv[k], f"{name}[{i}] {st.recipe}: gap {sv[k - 1] / sv[k]:.2f}"


@pytest.mark.parametrize("name", list(H.CHAINS))
def test_one_early_matrix_is_scaled_by_two_to_the_forty_exactly(name):
    ch = H.CHAINS[name]
    big = [i for i, st in enumerate(ch.steps) if st.scale != 1.0]
    assert big and big[0] == 0 and all(ch.steps[i].scale == 2.0 ** 40 for i in big)
    for i in big:
        st, mk = ch.steps[i], H.made(name, i)
        base, _ = H._recipe(st.recipe, ch.cfg["k"], ch.cfg["center"] if ch.cfg["method"] == "random" else ch.cfg["lanczos_center"])
        assert np.array_equal(mk.A.data / st.dtype(2.0 ** 40), base.data.astype(st.dtype))    # exact in the step's dtype
        assert np.isfinite(mk.A.data).all() and np.abs(mk.A.data).max() > 1e12


@pytest.mark.parametrize("name", RANDOMIZED)
def test_a_chain_walks_the_widths_and_routes_it_declares(name):
    """l, ld and the sweep route of every step (engine.cpp:785-788, :128, :34-44), and that they move both ways"""
    ch = H.CHAINS[name]
    fits = [i for i, st in enumerate(ch.steps) if st.call != "remask_transform"]
    got = [H.panel_geometry(name, i) for i in range(len(ch.steps))]
    assert got == list(ch.walk), got
    for i in fits:
        l, ld, route = got[i]
        assert ch.cfg["k"] <= l <= ld and ld % 16 == 0
    if name.startswith(("R-", "M", "S-")):                                                    # (M, S: l moves; ld cannot -- the staged sweep's is 64 up to l = 64, and k + p = 10 stays below 16)
        seq = [(got[i][0], got[i][1]) for i in fits]
        moves = [b > a for a, b in zip(seq, seq[1:]) if a != b]
        assert True in moves and False in moves, seq                                          # rising and falling
    if name.startswith(("R-row", "R-staged")):
        assert len({(got[i][0], got[i][1]) for i in fits}) >= 3, got
    if name.startswith("R-wide"):
        assert got[0][0] > 64 >= got[1][0]                                                    # two column passes, then one
    sizes = [H.made(name, i).A.shape for i in fits]
    assert len(set(sizes)) >= (2 if name.startswith(("R-auto", "R-wide")) else 3)             # (those two alternate two shapes)


def test_the_row_chain_runs_all_three_dtype_patterns_over_the_same_steps():
    a, b, c = (H.CHAINS[n].steps for n in ("R-row-f32", "R-row-f64", "R-row-mixed"))
    assert [s.recipe for s in a] == [s.recipe for s in b] == [s.recipe for s in c]
    assert {s.dtype for s in a} == {np.float32} and {s.dtype for s in b} == {np.float64}
    assert [s.dtype for s in c] == [np.float32, np.float64] * 3
    for steps in (a, b, c):
        assert {s.entry for s in steps} == {"host", "device", "resident"}
    mk = H.made("R-row-f32", 3)                                                               # the ragged step
    lens = np.diff(mk.A.indptr)
    m, n = mk.A.shape
    assert 0.04 * m <= (lens == 0).sum() <= 0.06 * m and (lens == n).sum() == 1
    assert H.made("R-row-f32", 2).A.shape[0] == 40 and H.CHAINS["R-row-f32"].cfg["k"] == 12


def test_the_staged_chain_descends_and_ascends_and_sorts_once():
    ch = H.CHAINS["R-staged-f32"]
    nnz = [H.made(ch.name, i).A.nnz for i in range(len(ch.steps))]
    assert nnz[0] > nnz[1] > nnz[2] > nnz[3] < nnz[4] < nnz[5] < nnz[6] < nnz[7], nnz
    assert {H.made(ch.name, i).A.shape for i in range(len(ch.steps))} >= {(1027, 333), (37, 1200), (5, 70), (2051, 65)}
    sorts = [i for i, st in enumerate(ch.steps) if "SAPCA_ROWSORT_ALWAYS" in st.env]
    assert sorts == [6] and all("SAPCA_NO_ROWSORT" in ch.steps[i].env for i in (5, 7))
    lens = np.diff(H.made(ch.name, 6).A.indptr)
    assert lens.max() > 3 * np.median(lens) and np.percentile(lens, 99) > 2 * np.median(lens)   # a long tail of long rows
    assert ch.debug and ch.cfg["k"] <= 5 and [s.dtype for s in H.CHAINS["R-staged-f64"].steps] == [np.float64] * 8


def test_the_auto_chain_alternates_about_the_staged_sweeps_floor():
    """variant 0 with SAPCA_TILED_MIN_ENTRIES = 30000 in the debug library: both conditions of engine.cpp:42"""
    ch = H.CHAINS["R-auto"]
    assert ch.debug and ch.cfg["variant"] == 0
    sides = []
    for i, st in enumerate(ch.steps):
        assert st.env == {"SAPCA_TILED_MIN_ENTRIES": "30000"} and st.dtype == np.float32
        A = H.made(ch.name, i).A
        m, n = A.shape
        chunks = math.ceil(m / 512) * math.ceil(n * 256 / (80 * 1024))
        dense, many = A.nnz * 64 >= chunks * 80 * 1024, A.nnz >= 30000
        assert H.staged_floor(m, n, A.nnz, 4, "30000") == (dense and many)
        assert not H.staged_floor(m, n, A.nnz, 4)                                              # the release floor: never
        sides.append(dense and many)
        if not (dense and many):
            assert dense and not many                                                         # below the entry floor alone
    assert sides == [True, False, True, False, True]
    assert [g[1] for g in ch.walk] == [64, 32, 64, 32, 64]


def test_the_masked_chain():
    ch = H.CHAINS["M"]
    assert ch.cfg["masked"] and ch.cfg["center"] and ch.cfg["semantics"] == "reference" and ch.cfg["variant"] == 2
    keeps = [st.mask[0] for st in ch.steps[:3]]
    assert keeps == [0.9, 0.2, 0.6]
    assert ch.steps[1].reuse_input and ch.steps[1].recipe == ch.steps[0].recipe and ch.steps[1].entry == "resident"
    # q3_cancels (engine.cpp:628): (sum a)^2 > m sum a^2 / 4 in some kept column -- set by the heavy step alone, which stands
    # between two ordinary ones
    for i, st in enumerate(ch.steps):
        stat = H.q3_statistic("M", i)
        assert (stat > 0.25) == (i == H.M_HEAVY_STEP), (i, stat)
        assert st.dtype == np.float32                                                         # (the two-sweep Q3 route is f32 only)
    mk = H.made("M", H.M_HEAVY_STEP)
    heavy = [j for j in H.heavy_columns(mk.A.shape[1], 12) if mk.mask[j]]
    assert len(heavy) >= 4
    D = mk.A64.toarray()[:, heavy]
    assert (D != 0).all() and np.abs(D - 1000.0).max() < 0.1                                   # well filled, small spread
    z = H.made("M", 4).A.data
    assert (z == 0).sum() == 300 and np.signbit(z[z == 0]).sum() == 150                        # stored +0.0 and -0.0
    assert ch.steps[-1].call == "remask_transform" and ch.steps[-1].reuse_input


@pytest.mark.parametrize("name", LANCZOS)
def test_the_lanczos_chains(name):
    ch = H.CHAINS[name]
    shapes = [H.made(name, i).A.shape for i in range(len(ch.steps))]
    routes = [H.lanczos_route(name, i) for i in range(len(ch.steps))]
    assert shapes[0][0] > 4096 and shapes[1][0] > 4096 and shapes[2][0] < 4096 and shapes[3][0] < shapes[3][1]
    assert routes == ["transposed", "scatter", "transposed", "transposed", "scatter"]
    assert ch.debug and ch.steps[0].env == {"SAPCA_LANCZOS_TRANSPOSE": "1"} and not ch.steps[1].env
    assert ch.cfg["lanczos_center"] == name.endswith("-centred") and ch.cfg["center"] == ch.cfg["lanczos_center"]


@pytest.mark.parametrize("name", ["S-f32", "S-f64"])
def test_the_setter_chain_crosses_every_setter(name):
    ch = H.CHAINS[name]
    assert [(st.cov, st.scaling) for st in ch.steps] == [(False, None), (True, None), (True, "weights"), (False, "unit_variance"), (False, None), (False, None), (False, None)]
    sizes = [H.made(name, i).A.shape[0] * H.made(name, i).A.shape[1] for i in range(len(ch.steps))]
    assert sizes == sorted(sizes, reverse=True)
    assert H.made(name, 1).A.shape == (513, 257) and H.made(name, 3).A.shape == (320, 208)
    assert ch.cfg["semantics"] == "centred" and H.made(name, 2).d is not None and (H.made(name, 2).d > 0).any()

"""Harmony without a GPU: the numpy restatement (tests/harmony_ref.py) against independent sources -- scikit-learn's Ridge for
the mixture-of-experts coefficients, scipy's softmax for a pass without a diversity penalty, numpy.array_split for the blocks,
its own bookkeeping recomputed from R -- the closed form the library runs against the dense solve, the recorded fixture
(tests/golden/g15_harmony.npz), and the header, the exports and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import harmony_ref as HR
import sapca
from sapca import _lib as L
from sapca import ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g15_harmony.npz")
SYMBOLS = [f"sapca_harmony{stage}_{suf}" for stage in ("_assign_device", "_centroids_device", "_correct_device", "_device", "")
           for suf in ("f32", "f64")]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def state(gold):
    """the fixture after the initialisation and two passes: (Zc, batch, B, Y, R, O, rs, E, dist)"""
    Z, batch = gold["Z"], gold["batch"]
    Zc = HR.normalise_rows(Z)
    Y = HR.normalise_rows(gold["Y0"])
    R = HR.init_R(Zc, Y, 0.1)
    for c in range(2):
        Y, R, O, rs, E, dist = HR.one_pass(Zc, batch, 2, Y, R, 2.0, 0.1, 20, 42, c)
    return Zc, batch, 2, Y, R, O, rs, E, dist


@pytest.mark.parametrize("lam", [1e-3, 1.0, 1e3])
def test_ridge_coefficients_equal_scikit_learn(gold, state, lam):
    from sklearn.linear_model import Ridge
    Z, batch = gold["Z"], gold["batch"]
    R = state[4]
    Phi, _ = HR.design(batch, 2)
    _, W = HR.ridge(Z, R, batch, 2, lam)
    for k in range(R.shape[1]):
        coef = Ridge(alpha=lam, fit_intercept=True, solver="cholesky").fit(Phi.T, Z, sample_weight=R[:, k]).coef_   # d x B
        assert np.abs(W[k][1:] - coef.T).max() <= 1e-9 * max(np.abs(coef).max(), 1.0), k


def test_pass_without_penalty_is_a_softmax(state):
    from scipy.special import softmax
    Zc, batch, B, Y, R = state[:5]
    want = softmax(-HR.distances(Zc, Y) / 0.1, axis=1)
    for n_blocks in (1, 7, 20):
        got = HR.one_pass(Zc, batch, B, Y, R, 0.0, 0.1, n_blocks, 42, 5, recompute=False)[1]
        assert np.abs(got - want).max() <= 1e-14


def test_bookkeeping_equals_its_recomputation_from_R(state):
    Zc, batch, B, Y, R, O, rs, E, dist = state
    Phi, _ = HR.design(batch, B)
    assert np.abs(rs - R.sum(axis=0)).max() <= 1e-11
    assert np.abs(O - Phi @ R).max() <= 1e-11
    assert np.abs(E - np.outer(Phi.sum(axis=1) / len(batch), R.sum(axis=0))).max() <= 1e-11
    assert np.abs(R.sum(axis=1) - 1.0).max() <= 1e-14
    assert np.abs(np.linalg.norm(Y, axis=1) - 1.0).max() <= 1e-14


@pytest.mark.parametrize("lam", [1e-3, 1.0, 1e3])
def test_closed_form_equals_dense_solve(gold, state, lam):
    Z, batch = gold["Z"], gold["batch"]
    R = state[4].copy()
    R[:, 3] = 0.0   # a cluster without weight contributes nothing in either form
    dense, W = HR.ridge(Z, R, batch, 2, lam)
    closed, beta = HR.ridge_closed(Z, R, batch, 2, lam)
    assert np.abs(W[:, 1:, :] - beta).max() <= 1e-9 * max(np.abs(beta).max(), 1.0)
    assert np.abs(dense - closed).max() <= 1e-10 * np.abs(Z).max()
    assert not beta[3].any()


def test_blocks_are_array_split_of_the_stated_order():
    assert HR.STREAM == 61
    for m, n_blocks, seed, c in ((17, 3, 42, 0), (600, 20, 42, 4), (5, 9, 1, 2), (64, 1, 7, 1)):
        u = synth.hash_u01(seed, 61, torch.arange(m, dtype=torch.int64) + c * m).numpy()
        want = sorted(range(m), key=lambda i: (u[i], i))
        got = HR.blocks(seed, c, m, n_blocks)
        assert len(got) == n_blocks and [len(b) for b in got] == [m // n_blocks + (j < m % n_blocks) for j in range(n_blocks)]
        assert np.concatenate(got).tolist() == want


def test_recorded_fixture_is_the_restatements_run(gold):
    Z, batch, Y0 = gold["Z"], gold["batch"], gold["Y0"]
    assert Z.shape == (600, 10) and np.bincount(batch).tolist() == [300, 300] and Y0.shape == (20, 10)
    r = HR.run(Z, batch, 2, Y0)
    assert r["margin"] > 0.1 and abs(r["margin"] - float(gold["f64_margin"])) < 1e-6
    assert r["passes"].tolist() == gold["f64_passes"].tolist() and r["n_iter"] == int(gold["f64_n_iter"]) and r["converged"]
    assert np.abs(r["Zcorr"] - gold["f64_Zcorr"]).max() <= 1e-9
    # what the correction is for: the neighbourhoods mix the batches and keep the cell types
    before = HR.same_label_share(HR.knn_bruteforce(Z, 15), batch)
    after = HR.same_label_share(HR.knn_bruteforce(r["Zcorr"], 15), batch)
    assert before > 0.9 and after < 0.56
    assert HR.same_label_share(HR.knn_bruteforce(r["Zcorr"], 15), gold["kind"]) > 0.99


def test_header_declares_and_library_exports_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "sapca.h")).read()
    for name in SYMBOLS:
        assert re.search(r"sapca_status\s+%s\(" % name, hdr), name
        assert name in L.EXPORTED_SYMBOLS, name
    assert re.search(r"SAPCA_HARMONY_KMEANS = 0, SAPCA_HARMONY_GIVEN = 1", hdr) and L.HARMONY_KMEANS == 0 and L.HARMONY_GIVEN == 1
    assert L.HARMONY_MAX_BATCHES == 1024 and "#define SAPCA_HARMONY_MAX_BATCHES 1024" in hdr
    lib = C.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def test_session_and_class_exist():
    for name in ("harmony_assign", "harmony_centroids", "harmony_correct", "harmony"):
        assert callable(getattr(ops.Session, name))
    hm = sapca.Harmony(theta=1.5, n_blocks=5)
    assert (hm.theta, hm.sigma, hm.lam, hm.n_blocks, hm.max_iter_harmony, hm.max_iter_cluster) == (1.5, 0.1, 1.0, 5, 10, 20)
    assert (hm.epsilon_cluster, hm.epsilon_harmony, hm.n_clusters) == (1e-5, 1e-4, None) and hm.Z_corr_ is None

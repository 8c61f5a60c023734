"""The host solvers of single-algebra_amd/csrc/small_svd.cpp -- sym_eigh_desc (in every f32 randomized fit), jacobi_svd (in every
f64 one), tridiag_eigh in both last_row_only modes (in every Lanczos fit) -- through tools/small_svd_check.cpp, built here with
the host compiler from small_svd.cpp alone, against LAPACK (numpy) and, for n <= 16, a 40-digit mpmath solution.

Unit of error: n 2^-52 |A|_2.  Every figure below is in that unit (the orthogonality of the vectors: in n 2^-52).  The margin
of a check is 16 x the larger of one unit and what LAPACK itself leaves on the same matrix -- for the eigenvalues and singular
values against mpmath (n <= 16; above, the 16-unit floor), for residual and orthogonality LAPACK's own vectors.
Measured over the cases of this file (largest figure per solver, and LAPACK's own on the same matrices; every test prints them):
    values:         LAPACK against mpmath 0.69 (n <= 16); against LAPACK sym_eigh_desc 0.89, tridiag_eigh 0.46, jacobi_svd 1.7
    residual:       sym_eigh_desc 0.58 (LAPACK 0.89), tridiag_eigh 0.75 (0.50), jacobi_svd 4.4 (1.0)
    orthogonality:  sym_eigh_desc 1.3 (LAPACK 1.0), tridiag_eigh 1.0 (1.0), jacobi_svd 4.4 (1.5)
so every margin in force is the 16-unit floor or just above it (24 where LAPACK leaves 1.5).
The matrices scaled by 1e+-300 are what the solvers' range scaling is for (small_svd.cpp, RangeScale): without it jacobi_svd
overflows at 1e300 and sym_eigh_desc leaves V^T V = I off by 80 and 210 units at n = 128 and 270, |A| = 1e-300."""
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 16, 61, 112, 128, 270)
EPS = 2.0 ** -52
MP_MAX_N = 16


def _rng(*key):
    return np.random.default_rng([777, *key])


def _orthogonal(n, rng):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _spectra(n, rng):
    """name -> eigenvalues (or singular values where non-negative) of the families built from a random orthogonal basis"""
    i = np.arange(n)
    return {
        "graded": 10.0 ** (-12.0 * i / max(n - 1, 1)),
        "clustered": np.where(i < (n + 1) // 2, 1.0 + 1e-10 * rng.uniform(0, 1, n), 2.0 + 1e-13 * i),
        "equal": np.full(n, 3.0),
        "rank-deficient": np.where(i < (n + 1) // 2, 1.0 + i, 0.0),
        "indefinite": (1.0 + i) * np.where(i % 2, -1.0, 1.0),
        "scaled 1e300": 1e300 * rng.uniform(0.5, 1.0, n),
        "scaled 1e-300": 1e-300 * rng.uniform(0.5, 1.0, n),
    }


def _wilkinson(n):
    return np.abs((n - 1) / 2.0 - np.arange(n)), np.ones(n)


@functools.lru_cache(maxsize=None)
def symmetric_cases(n):
    rng = _rng(0, n)
    out = {}
    for name, lam in _spectra(n, rng).items():
        Q = _orthogonal(n, rng)
        A = (Q * lam) @ Q.T
        out[name] = (A + A.T) / 2
    out["zero"] = np.zeros((n, n))
    out["diagonal"] = np.diag(rng.permutation(np.arange(n) - n // 2).astype(np.float64))
    d, e = rng.standard_normal(n), rng.standard_normal(n)
    out["tridiagonal"] = np.diag(d) + np.diag(e[1:], 1) + np.diag(e[1:], -1)
    d, e = _wilkinson(n)
    out["Wilkinson"] = np.diag(d) + np.diag(e[1:], 1) + np.diag(e[1:], -1)
    return out


@functools.lru_cache(maxsize=None)
def tridiagonal_cases(n):
    """name -> (d, e), e[i] coupling i - 1 and i, e[0] unused"""
    rng = _rng(1, n)
    i = np.arange(n)
    out = {
        "graded": (10.0 ** (-12.0 * i / max(n - 1, 1)), 10.0 ** (-12.0 * i / max(n - 1, 1)) * 0.3),
        "clustered": (np.ones(n), np.full(n, 1e-9)),
        "equal": (np.full(n, 3.0), np.zeros(n)),
        "rank-deficient": (np.where(i % 2, 0.0, 1.0), np.zeros(n)),
        "zero": (np.zeros(n), np.zeros(n)),
        "scaled 1e300": (1e300 * rng.uniform(0.5, 1.0, n), 1e299 * rng.uniform(-1, 1, n)),
        "scaled 1e-300": (1e-300 * rng.uniform(0.5, 1.0, n), 1e-301 * rng.uniform(-1, 1, n)),
        "indefinite": (rng.standard_normal(n), rng.standard_normal(n)),
        "diagonal": (rng.permutation(i - n // 2).astype(np.float64), np.zeros(n)),
        "tridiagonal": (np.full(n, 2.0), np.full(n, -1.0)),
        "Wilkinson": _wilkinson(n),
    }
    return {k: (np.asarray(d, np.float64).copy(), np.asarray(e, np.float64).copy()) for k, (d, e) in out.items()}


@functools.lru_cache(maxsize=None)
def jacobi_cases(n):
    """general square matrices U diag(s) V^T of the same families, and the upper triangular factors a fit hands it: R of a QR
    of a matrix with singular values down to 1e-14, and one with exact zero columns"""
    rng = _rng(2, n)
    out = {}
    for name, s in _spectra(n, rng).items():
        if name == "indefinite":
            continue
        out[name] = (_orthogonal(n, rng) * s) @ _orthogonal(n, rng).T
    out["zero"] = np.zeros((n, n))
    out["diagonal"] = np.diag(rng.permutation(np.arange(n) - n // 2).astype(np.float64))
    s = 10.0 ** (-14.0 * np.arange(n) / max(n - 1, 1))
    R = np.linalg.qr((_orthogonal(n, rng) * s) @ _orthogonal(n, rng).T)[1]
    out["triangular to 1e-14"] = np.triu(R)
    Z = np.triu(rng.standard_normal((n, n)))
    Z[:, n // 2:] = 0.0                                  # exact zeros: singular values 0, zero columns of U
    out["triangular, zero columns"] = Z
    return out


# ---- the program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("small_svd") / "small_svd_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "small_svd_check.cpp"),
                    os.path.join(ROOT, "single-algebra_amd", "csrc", "small_svd.cpp")], check=True)
    return str(exe)


def _run(program, tmp_path, records):
    """records: [(kind, n, arrays...)] -> the parsed results, one tuple per record"""
    cases, results = tmp_path / "cases.bin", tmp_path / "results.bin"
    with open(cases, "wb") as f:
        for kind, n, *arrays in records:
            f.write(struct.pack("<qq", kind, n))
            for a in arrays:
                f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    subprocess.run([program, str(cases), str(results)], check=True, capture_output=True)
    raw = open(results, "rb").read()
    pos, out = 0, []

    def take_int():
        nonlocal pos
        v = struct.unpack_from("<q", raw, pos)[0]
        pos += 8
        return v

    def take(count, shape):
        nonlocal pos
        a = np.frombuffer(raw, dtype="<f8", count=count, offset=pos).reshape(shape).copy() if count else np.zeros(shape)
        pos += 8 * count
        return a

    for kind, n, *_ in records:
        if kind == 0:
            out.append((take_int(), take(n, (n,)), take(n * n, (n, n))))
        elif kind == 1:
            out.append((take(n, (n,)), take(n * n, (n, n))))
        else:
            out.append((take_int(), take(n, (n,)), take(n * n, (n, n)), take_int(), take(n, (n,)), take(n, (n,))))
    assert pos == len(raw)
    return out


# ---- references
def _mp_eigenvalues(A):
    import mpmath as mp
    with mp.workdps(40):
        w = mp.eigsy(mp.matrix(A.tolist()), eigvals_only=True)
        return sorted((w[i] for i in range(len(w))), reverse=True)


def _mp_singular_values(A):
    import mpmath as mp
    with mp.workdps(40):
        s = mp.svd_r(mp.matrix(A.tolist()), compute_uv=False)
        return sorted((s[i] for i in range(len(s))), reverse=True)


def _against_mp(values, exact, unit):
    import mpmath as mp
    with mp.workdps(40):
        return max((float(abs(mp.mpf(float(v)) - x) / mp.mpf(unit)) for v, x in zip(values, exact)), default=0.0)


def _norm2(A):
    return float(np.linalg.norm(A, 2)) if A.size else 0.0


def _margin(reference_figure):
    return 16.0 * max(1.0, reference_figure)


def _units(err, unit):
    return float(np.max(err) / unit) if unit > 0 and np.size(err) else float(np.max(err, initial=0.0) > 0) * np.inf


FIGURES = {}      # (solver, property) -> (largest figure of the solver, largest of LAPACK) so far, printed by every test


def _note(solver, prop, got, ref):
    a, b = FIGURES.get((solver, prop), (0.0, 0.0))
    FIGURES[(solver, prop)] = (max(a, got), max(b, ref))


def _report(solver):
    print("; ".join(f"{prop}: {solver} {g:.3g}, LAPACK {r:.3g}" for (sv, prop), (g, r) in sorted(FIGURES.items()) if sv == solver))


def _normalised(A):
    """(A 2^-e, 2^-e) with 2^e <= |A|_2 < 2^(e+1): residuals of a matrix at 1e+-300 are formed at this multiple of it"""
    norm = _norm2(A)
    f = 2.0 ** -int(np.floor(np.log2(norm))) if norm > 0 else 1.0
    return A * f, f


def _check_eigen(solver, name, n, A, w, V, ref_w, ref_V, mp_values):
    """w descending with eigenvectors in the columns of V, against LAPACK's (ref_w descending, ref_V)"""
    norm = _norm2(A)
    unit = n * EPS * norm
    tag = f"{solver} {name} n = {n}"
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(V)), tag
    assert np.all(w[:-1] >= w[1:]), tag
    lapack_values = _against_mp(ref_w, mp_values, unit) if mp_values is not None and unit > 0 else 0.0
    An, f = _normalised(A)
    figs = {"values": (_units(np.abs(w - ref_w), unit), lapack_values),
            "residual": (_units(np.linalg.norm(An @ V - V * (w * f), axis=0), unit * f),
                         _units(np.linalg.norm(An @ ref_V - ref_V * (ref_w * f), axis=0), unit * f)),
            "orthogonality": (float(np.abs(V.T @ V - np.eye(n)).max() / (n * EPS)), float(np.abs(ref_V.T @ ref_V - np.eye(n)).max() / (n * EPS)))}
    if unit == 0:
        assert not w.any(), tag
        figs["values"] = figs["residual"] = (0.0, 0.0)
    for prop, (got, ref) in figs.items():
        _note(solver, prop, got, ref)
        assert got <= _margin(ref), f"{tag}: {prop} {got:.3g} units, LAPACK leaves {ref:.3g}"


@pytest.mark.parametrize("n", SIZES)
def test_sym_eigh_desc(program, tmp_path, n):
    """eigenvalues against numpy.linalg.eigvalsh, residual A V - V diag(w), V^T V = I, descending order, convergence"""
    cases = symmetric_cases(n)
    got = _run(program, tmp_path, [(0, n, A) for A in cases.values()])
    for (name, A), (ok, w, Vt) in zip(cases.items(), got):
        assert ok == 1, f"{name} n = {n}: did not converge"
        ref_w, ref_V = np.linalg.eigh(A)
        mp_values = _mp_eigenvalues(A) if n <= MP_MAX_N else None
        _check_eigen("sym_eigh_desc", name, n, A, w, Vt.T, ref_w[::-1], ref_V[:, ::-1], mp_values)
    _report("sym_eigh_desc")


@pytest.mark.parametrize("n", SIZES)
def test_tridiag_eigh_both_modes(program, tmp_path, n):
    """the same checks (ascending order turned round), and last_row_only: identical eigenvalues, and its one row is the bottom
    row of the full eigenvector matrix bit for bit"""
    cases = tridiagonal_cases(n)
    got = _run(program, tmp_path, [(2, n, d, e) for d, e in cases.values()])
    for (name, (d, e)), (ok, w, Z, ok1, w1, z1) in zip(cases.items(), got):
        assert ok == 1 and ok1 == 1, f"{name} n = {n}: did not converge"
        assert w.tobytes() == w1.tobytes() and Z[n - 1].tobytes() == z1.tobytes(), f"{name} n = {n}: last_row_only differs"
        assert np.all(w[:-1] <= w[1:]), f"{name} n = {n}: not ascending"
        T = np.diag(d) + np.diag(e[1:], 1) + np.diag(e[1:], -1)
        ref_w, ref_V = np.linalg.eigh(T)
        mp_values = _mp_eigenvalues(T) if n <= MP_MAX_N else None
        _check_eigen("tridiag_eigh", name, n, T, w[::-1], Z[:, ::-1], ref_w[::-1], ref_V[:, ::-1], mp_values)
    _report("tridiag_eigh")


@pytest.mark.parametrize("n", SIZES)
def test_jacobi_svd(program, tmp_path, n):
    """singular values against numpy.linalg.svd, descending order, orthonormal columns of U where s > 0 and zero columns where
    s = 0, and the residual of the left vectors, A A^T u = s^2 u, through |A^T u| = s"""
    cases = jacobi_cases(n)
    got = _run(program, tmp_path, [(1, n, A) for A in cases.values()])
    for (name, A), (s, U) in zip(cases.items(), got):
        tag = f"jacobi_svd {name} n = {n}"
        norm = _norm2(A)
        unit = n * EPS * norm
        assert np.all(np.isfinite(s)) and np.all(np.isfinite(U)) and np.all(s >= 0) and np.all(s[:-1] >= s[1:]), tag
        ref_U, ref_s, _ = np.linalg.svd(A)
        live = s > 0
        assert not U[:, ~live].any(), tag
        if unit == 0:
            assert not s.any(), tag
            continue
        lapack_values = _against_mp(ref_s, _mp_singular_values(A), unit) if n <= MP_MAX_N else 0.0
        Ul = U[:, live]
        An, f = _normalised(A)
        figs = {"values": (_units(np.abs(s - ref_s), unit), lapack_values),
                "residual": (_units(np.abs(np.linalg.norm(An.T @ Ul, axis=0) - s[live] * f), unit * f),
                             _units(np.abs(np.linalg.norm(An.T @ ref_U, axis=0) - ref_s * f), unit * f)),
                "orthogonality": (float(np.abs(Ul.T @ Ul - np.eye(Ul.shape[1])).max() / (n * EPS)),
                                  float(np.abs(ref_U.T @ ref_U - np.eye(n)).max() / (n * EPS)))}
        for prop, (g, ref) in figs.items():
            _note("jacobi_svd", prop, g, ref)
            assert g <= _margin(ref), f"{tag}: {prop} {g:.3g} units, LAPACK leaves {ref:.3g}"
        if name == "triangular, zero columns":
            assert np.count_nonzero(s == 0) >= n - n // 2 and (n < 2 or not live.all()), tag
    _report("jacobi_svd")

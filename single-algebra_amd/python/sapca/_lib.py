"""ctypes binding of libsapca.so (include/sapca.h).  No fallbacks: if the HIP library is
missing or there is no GPU, calls fail loudly.

The structure classes, the constants and every function's argtypes / restype are built from sapca/_abi.py, the table
tools/gen_sapca_abi.py writes from the header; nothing here restates the header.  After editing include/sapca.h run
`python tools/gen_sapca_abi.py && python tools/gen_sapca_sys.py`."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._abi import CONSTANTS, FUNCTIONS, STRUCTS

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAPCA_LIB_PATH points at another build of the same library (kernel experiments, tools/abl_build.sh)
LIB_PATH = os.environ.get("SAPCA_LIB_PATH") or os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libsapca.so"))
# the variant that reads the SAPCA_* experiment / route switches (csrc/switches.h; the release library reads none of them)
DEBUG_LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libsapca_dbg.so"))

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p)

# by-value C types; a handle is an opaque pointer
_SCALAR = {"int": C.c_int, "sapca_status": C.c_int, "double": C.c_double, "size_t": C.c_size_t, "uint8_t": C.c_uint8,
           "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "sapca_handle": C.c_void_p, "sapca_multi": C.c_void_p, "sapca_allreduce_fn": ALLREDUCE_FN}
_STRUCTS = {}   # sapca_tsne_options -> the class TsneOptions


def _ctype(t):
    """The ctypes twin of a C type of the table: a scalar by value is its exact type, a pointer to a struct of the header
    POINTER(its class), any other pointer (T**, sapca_handle*, ...) c_void_p, which takes None, integers, c_void_p,
    data_as(..) results and byref(..).  A type outside this rule is a KeyError: extend the rule, do not loosen it."""
    t = t.replace("const ", "")
    if t.endswith("*"):
        return C.POINTER(_STRUCTS[t[:-1]]) if t[:-1] in _STRUCTS else C.c_void_p
    return _SCALAR[t]


def _restype(t):
    return None if t == "void" else C.c_char_p if t == "const char*" else _ctype(t)


for _name, _fields in STRUCTS.items():
    _cls = "".join(w.capitalize() for w in _name.split("_")[1:])
    _STRUCTS[_name] = type(_cls, (C.Structure,), {
        "__doc__": _name, "_fields_": [(f, _ctype(t) * n if n else _ctype(t)) for f, t, n in _fields]})
    globals()[_cls] = _STRUCTS[_name]   # Options, Timings, CsrReport, TsneOptions, KmeansOptions, UmapOptions, ...
# the header's enumerators and integer #defines without their SAPCA_ prefix: OK ... ERR_NOMEM, KNN_*, HVG_*, CSR_*, ...
globals().update(CONSTANTS)

# names a caller passes -> the header's values
SPECTRAL_KINDS = {"normalized": CONSTANTS["SPECTRAL_NORMALIZED"], "diffmap": CONSTANTS["SPECTRAL_DIFFMAP"]}
CSR_FLAG_NAMES = {CONSTANTS["CSR_" + n]: n for n in ("BAD_OFFSETS", "COL_RANGE", "UNSORTED", "DUPLICATES", "NONFINITE")}
KNN_METRICS = {"euclidean": CONSTANTS["KNN_EUCLIDEAN"], "cosine": CONSTANTS["KNN_COSINE"], "pearson": CONSTANTS["KNN_PEARSON"]}
HVG_TRANSFORMS = {"clip": CONSTANTS["HVG_CLIP"], "expm1": CONSTANTS["HVG_EXPM1"]}
HVG_FLAVORS = {"seurat_v3": CONSTANTS["HVG_SEURAT_V3"], "seurat": CONSTANTS["HVG_SEURAT"]}
UMAP_INITS = {"panel": CONSTANTS["UMAP_INIT_PANEL"], "random": CONSTANTS["UMAP_INIT_RANDOM"]}

# every symbol include/sapca.h declares (the CPU test checks the library exports each one)
EXPORTED_SYMBOLS = [name for name, _, _ in FUNCTIONS]

# the element types the _f32 / _f64 entry points take, and an array's pointer for an argument
_SUF = {np.dtype(np.float32): ("f32", C.c_float), np.dtype(np.float64): ("f64", C.c_double)}


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


_lib = None


class SapcaError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


def load():
    """dlopen libsapca.so.  torch (if it is going to be used at all) must be imported first so the
    process shares ONE HIP runtime / RCCL: bench.py and the tests import torch at the top."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH) and not os.environ.get("SAPCA_NO_AUTOBUILD"):
        # building the product is not a fallback: same sources, same gfx950 target
        import shutil
        import subprocess
        if shutil.which("make") and (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
            subprocess.call(["make", "-C", os.path.normpath(os.path.join(_HERE, "..", "..")), "-j", "8"])
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C single-algebra_amd` "
            "(or python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    _lib = _open(LIB_PATH)
    return _lib


_debug_lib = None


def load_debug():
    """The -DSAPCA_DEBUG_SWITCHES build of the same sources (make debug): for tests and tools that steer routes through
    SAPCA_* environment variables.  A second library instance beside the release one (its own handles: objects do not cross)."""
    global _debug_lib
    if _debug_lib is None:
        if not os.path.exists(DEBUG_LIB_PATH):
            raise ImportError(f"{DEBUG_LIB_PATH} is missing: build it with `make -C single-algebra_amd debug`")
        _debug_lib = _open(DEBUG_LIB_PATH)
    return _debug_lib


def _open(path):
    lib = C.CDLL(path)
    for name, ret, params in FUNCTIONS:
        fn = getattr(lib, name, None)   # (an older build loaded through SAPCA_LIB_PATH for an A/B run lacks the newer ones)
        if fn is not None:
            fn.restype = _restype(ret)
            fn.argtypes = [_ctype(t) for t in params]
    return lib


def _default(struct):
    """A struct of the header as the library's `<struct>_default` fills it."""
    o = _STRUCTS[struct]()
    getattr(load(), struct + "_default")(C.byref(o))
    return o


def default_options():
    return _default("sapca_options")


def default_tsne_options():
    return _default("sapca_tsne_options")


def default_kmeans_options():
    return _default("sapca_kmeans_options")


def default_umap_options():
    return _default("sapca_umap_options")


def default_louvain_options():
    return _default("sapca_louvain_options")


def default_hvg_options():
    return _default("sapca_hvg_options")


def default_spectral_options():
    return _default("sapca_spectral_options")


def find_ab_params(spread=1.0, min_dist=0.1):
    """sapca_umap_find_ab: (a, b) of the curve 1 / (1 + a x^(2b)) fitted to (spread, min_dist) as umap-learn's find_ab_params
    does.  Pure host code, no device.  Bad arguments raise SapcaError (ERR_ARG), a fit that does not converge ERR_SVD."""
    a, b = C.c_double(), C.c_double()
    st = load().sapca_umap_find_ab(C.c_double(float(spread)), C.c_double(float(min_dist)), C.byref(a), C.byref(b))
    if st != CONSTANTS["OK"]:
        raise SapcaError(st, f"sapca_umap_find_ab(spread={spread}, min_dist={min_dist}): "
                         + ("the fit did not converge in 200 steps" if st == 4 else
                            "spread must be finite and positive, min_dist finite, not negative and below 3 spread"))
    return a.value, b.value


def check(handle, status):
    if status != CONSTANTS["OK"]:
        msg = load().sapca_last_error(handle)
        raise SapcaError(status, (msg or b"").decode() or f"sapca status {status}")


def as_u64(a):
    """A CSR offset / index array in the library's u64 (nalgebra_sparse `usize`) layout: int64 arrays -- what scipy holds for
    large matrices -- are reinterpreted in place (a negative entry reads as an index the library refuses), anything else
    is converted (a copy)."""
    a = np.asarray(a)
    if a.dtype == np.uint64 and a.flags.c_contiguous:
        return a
    if a.dtype == np.int64 and a.flags.c_contiguous:
        return a.view(np.uint64)
    return np.ascontiguousarray(a, dtype=np.uint64)

"""CPU tests of the boundary: the C-ABI library loads, exports every symbol include/sapca.h
declares, refuses to run without a GPU (no CPU fallback), and its host-only code works."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import sapca
from sapca import _lib as L
from sapca import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    declared = set(re.findall(r"\b(sapca_[a-z0-9_]+)\s*\(", header)) - {"sapca_allreduce_fn"}
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/sapca.h but not exported"
    assert declared == set(L.EXPORTED_SYMBOLS)
    assert lib.sapca_abi_version() == 4


def test_options_struct_layout_matches_header():
    o = L.default_options()
    assert o.struct_size == C.sizeof(L.Options)
    # builder defaults: sparse/mod.rs:392-401, pca/mod.rs:64-68
    assert (o.n_components, o.alpha, o.tolerance, o.random_seed, o.center, o.verbose, o.method) == \
        (50, 1.0, 1e-6, 42, 1, 0, L.LANCZOS)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_no_cpu_fallback():
    with pytest.raises(L.SapcaError, match="no HIP device"):
        sapca.SparsePCABuilder.new().build()


def test_builder_defaults_and_fluent_surface():
    b = sapca.SparsePCABuilder.new()
    assert (b._n_components, b._alpha, b._tolerance, b._random_seed, b._center, b._verbose) == (50, 1.0, 1e-6, 42, True, False)
    assert b._svdmethod == sapca.SVDMethod.Lanczos() == sapca.SVDMethod()
    m = sapca.SVDMethod.Random(10, 7, sapca.PowerIterationNormalizer.QR)
    b2 = (sapca.MaskedSparsePCABuilder.new().n_components(5).alpha(1.5).tolerance(1e-4).random_seed(7)
          .center(False).verbose(True).svd_method(m).mask([True, False]))
    assert b2._n_components == 5 and b2._svdmethod.n_power_iterations == 7 and b2._mask.tolist() == [True, False]


def test_partition_rows_balances_nnz():
    rng = np.random.default_rng(0)
    counts = rng.integers(0, 50, 1000)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    for parts in (1, 2, 3, 8):
        b = ops.partition_rows(ptr, parts).astype(np.int64)
        assert b[0] == 0 and b[-1] == 1000 and np.all(np.diff(b) >= 0)
        per = np.diff(ptr[b])
        assert per.sum() == ptr[-1]
        assert per.max() - per.min() <= 2 * counts.max()
    # degenerate: empty matrix and more parts than rows
    assert ops.partition_rows(np.zeros(5, np.int64), 2).tolist() == [0, 2, 4]
    b = ops.partition_rows(np.array([0, 3, 6]), 4).astype(np.int64)
    assert b[0] == 0 and b[-1] == 2 and np.all(np.diff(b) >= 0)


def test_cpp_mirror_compiles(tmp_path):
    """the header-only C++ mirror of the reference interface (estimators + resident workflow) against include/sapca.h"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        import pytest
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "m.cpp"
    src.write_text('#include "%s"\n'
                   'template class sapca::ResidentCsr<float>;\ntemplate class sapca::ResidentCsr<double>;\n'
                   'int main() { auto b = sapca::SparsePCABuilder<float>().n_components(2); (void)b; return 0; }\n'
                   % os.path.join(root, "single-algebra_amd", "host", "cpp", "sapca.hpp"))
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _header_text():
    """include/sapca.h without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sapca.h")).read(), flags=re.S)


def _header_arguments():
    """(name -> the text between its parentheses) of every function include/sapca.h declares: an independent, cruder
    parse than the generators' (comments stripped, `name(args);`)."""
    return {name: args.strip() for name, args in re.findall(r"\b(sapca_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header_text())
            if name != "sapca_allreduce_fn"}


def _header_functions():
    """(name -> argument count), with the commas counted"""
    return {name: 0 if args in ("", "void") else args.count(",") + 1 for name, args in _header_arguments().items()}


STRUCT_CLASSES = (("sapca_options", "Options"), ("sapca_timings", "Timings"), ("sapca_csr_report", "CsrReport"),
                  ("sapca_tsne_options", "TsneOptions"), ("sapca_kmeans_options", "KmeansOptions"),
                  ("sapca_umap_options", "UmapOptions"), ("sapca_louvain_options", "LouvainOptions"),
                  ("sapca_hvg_options", "HvgOptions"), ("sapca_spectral_options", "SpectralOptions"))


def test_python_abi_table_is_what_its_generator_writes():
    """sapca/_abi.py, from which sapca/_lib.py builds every structure, constant and signature, is generated from the
    header (tools/gen_sapca_abi.py): the committed file is what the generator writes today."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_sapca_abi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_every_declared_function_is_typed_as_the_header_has_it():
    """After load() every function of the header carries argtypes: as many as the header has arguments, and each
    argument passed by value (no `*`, no `[n]`) with a ctypes type of its C size."""
    lib = L.load()
    c_size = {"uint64_t": 8, "size_t": 8, "double": 8, "sapca_handle": 8, "sapca_multi": 8, "sapca_allreduce_fn": 8,
              "int32_t": 4, "uint32_t": 4}
    counts, arguments = _header_functions(), _header_arguments()
    assert set(L.EXPORTED_SYMBOLS) == set(counts) and len(L.EXPORTED_SYMBOLS) == len(counts)
    typed = by_value = 0
    for name, n in counts.items():
        argtypes = getattr(lib, name).argtypes
        assert argtypes is not None and len(argtypes) == n, f"{name}: header has {n} arguments, argtypes {argtypes}"
        typed += 1
        for i, arg in enumerate(arguments[name].split(",") if n else ()):
            if "*" in arg or "[" in arg:
                assert C.sizeof(argtypes[i]) == C.sizeof(C.c_void_p), f"{name} argument {i} ({arg.strip()})"
                continue
            ctype = re.match(r"\s*(?:const\s+)?(\w+)\s+\w+\s*$", arg).group(1)
            assert C.sizeof(argtypes[i]) == c_size[ctype], f"{name} argument {i} ({arg.strip()}): {argtypes[i]}"
            assert not issubclass(argtypes[i], C._Pointer), f"{name} argument {i} ({arg.strip()}): {argtypes[i]}"
            by_value += 1
    assert typed == len(counts) >= 186 and by_value >= typed


def test_struct_defaults_write_the_python_class_size():
    """each sapca_*_options_default writes the struct_size of its ctypes class (host-only calls)"""
    lib = L.load()
    defaults = [name for name in _header_functions() if name.endswith("_options_default")]
    assert len(defaults) == 7
    classes = dict(STRUCT_CLASSES)
    for name in defaults:
        cls = getattr(L, classes[name[:-len("_default")]])
        o = cls()
        getattr(lib, name)(C.byref(o))
        assert o.struct_size == C.sizeof(cls), name
    for helper, cls in ((L.default_options, L.Options), (L.default_tsne_options, L.TsneOptions), (L.default_kmeans_options, L.KmeansOptions),
                        (L.default_umap_options, L.UmapOptions), (L.default_louvain_options, L.LouvainOptions),
                        (L.default_hvg_options, L.HvgOptions), (L.default_spectral_options, L.SpectralOptions)):
        o = helper()
        assert type(o) is cls and o.struct_size == C.sizeof(cls)


def test_every_header_constant_is_in_the_binding():
    """every enumerator and integer #define of the header is an attribute of sapca._lib under its name without SAPCA_,
    with the header's value (the test's own regexes, not the generators')"""
    hdr = _header_text()
    want = {name: int(value) for name, value in re.findall(r"^#define[ \t]+SAPCA_(\w+)[ \t]+(\d+)u?[ \t]*$", hdr, flags=re.M)}
    assert want["ABI_VERSION"] == 4 and want["KNN_MAX_NEIGHBORS"] == 128 and want["CSR_NONFINITE"] == 16
    n_defines = len(want)
    for body in re.findall(r"typedef\s+enum\s+\w+\s*\{(.*?)\}", hdr, flags=re.S):
        nxt = 0
        for item in filter(None, (x.strip() for x in body.split(","))):
            m = re.match(r"SAPCA_(\w+)(?:\s*=\s*(\d+))?$", item)
            nxt = int(m.group(2)) if m.group(2) else nxt
            want[m.group(1)] = nxt
            nxt += 1
    assert n_defines >= 17 and len(want) - n_defines >= 28
    for name, value in want.items():
        assert getattr(L, name) == value, name
    assert (L.OK, L.ERR_NOMEM, L.KNN_PEARSON, L.SCALE_WEIGHTS) == (0, 7, 2, 2)


def test_rust_sys_crate_declares_the_whole_header():
    """host/rust/sapca-sys/src/lib.rs is generated from the header (tools/gen_sapca_sys.py): every function, the same
    argument count, and the committed file is what the generator writes today."""
    import subprocess
    import sys
    rs = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca-sys", "src", "lib.rs")).read()
    block = rs[rs.index('extern "C" {'):]
    have = {}
    for name, args in re.findall(r"pub fn (sapca_\w+)\(([^()]*)\)", block):
        args = args.strip()
        have[name] = 0 if not args else args.count(":")
    want = _header_functions()
    assert set(have) == set(want), (sorted(set(want) - set(have)), sorted(set(have) - set(want)))
    for name, n in want.items():
        assert have[name] == n, f"{name}: header has {n} arguments, sapca-sys {have[name]}"
    assert len(want) >= 91
    # struct layouts: field counts and order of the POD structs
    hdr = _header_text()
    assert len(STRUCT_CLASSES) == len(re.findall(r"typedef\s+struct\s+\w+\s*\{", hdr))
    for struct, cls in ((s, getattr(L, c)) for s, c in STRUCT_CLASSES):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}" % struct, hdr, flags=re.S).group(1)
        c_fields = [re.match(r".*?(\w+)\s*(?:\[\d+\])?$", part.strip()).group(1)   # (`uint64_t a, b, c;` declares three)
                    for d in body.split(";") if d.strip() for part in " ".join(d.split()).split(",")]
        r_body = re.search(r"pub struct %s \{(.*?)\}" % struct, rs, flags=re.S).group(1)
        r_fields = re.findall(r"pub (\w+):", r_body)
        assert c_fields == r_fields == [f[0] for f in cls._fields_], struct
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_sapca_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the safe wrapper only calls functions the sys crate declares
    wrapper = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca", "src", "lib.rs")).read()
    for name in set(re.findall(r"ffi::\$?(sapca_[a-z0-9_]+)\b", wrapper) + re.findall(r"\b(sapca_[a-z0-9_]+_f(?:32|64))\b", wrapper)) - \
            {"sapca_handle", "sapca_multi", "sapca_options"}:
        assert name in have, f"host/rust/sapca uses {name}, which include/sapca.h does not declare"


def test_rust_builders_are_infallible_like_the_reference():
    """`SparsePCABuilder::build()` / `MaskedSparsePCABuilder::build()` return the estimator itself
    (/root/reference/src/dimred/pca/sparse/mod.rs:470-483, sparse_masked/mod.rs:146-160; README.md:56-66 writes
    `.build();` and then `pca.fit_transform(..)`): the wrapper must not hand back a Result there."""
    wrapper = open(os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca", "src", "lib.rs")).read()
    assert re.search(r"pub fn build\(self\) -> SparsePCA<T>\s*\{", wrapper)
    assert re.search(r"pub fn build\(self\) -> MaskedSparsePCA<T>\s*\{", wrapper)
    assert "pub fn build(self) -> Result" not in wrapper
    # the reference's constructors, same arity (sparse/mod.rs:63-71, sparse_masked/mod.rs:214-223)
    assert re.search(r"pub fn new\(n_components: usize, alpha: T, tollerance: Option<T>, random_seed: Option<u32>, center: bool, verbose: bool,\s*svdmethod: SVDMethod\) -> Self", wrapper)
    assert re.search(r"pub fn new\(n_components: usize, alpha: T, tollerance: Option<T>, random_seed: Option<u32>, mask: Vec<bool>, center: bool,\s*verbose: bool, svd_method: SVDMethod\) -> Self", wrapper)


def test_generated_sweep_loop_is_what_its_generator_writes(tmp_path):
    """csrc/spmm_dq2_gen.h (10.7 k lines of inline asm) is committed generator output: regenerate and compare."""
    import subprocess
    import sys
    out = tmp_path / "gen.h"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ2_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_spmm_dq2.py"), str(out)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    committed = open(os.path.join(ROOT, "single-algebra_amd", "csrc", "spmm_dq2_gen.h")).read()
    assert out.read_text() == committed, "spmm_dq2_gen.h is stale: run python tools/gen_spmm_dq2.py"


def test_release_library_reads_no_debug_switches():
    """csrc/switches.h: the SAPCA_* route / layout switches exist only in the -DSAPCA_DEBUG_SWITCHES variant.  The release
    library does not even carry their names; what it does read is listed in switches.h (two deployment escapes)."""
    import glob
    src = os.path.join(ROOT, "single-algebra_amd", "csrc")
    sites = []
    for f in glob.glob(os.path.join(src, "*")):
        for i, line in enumerate(open(f, errors="replace"), 1):
            if re.search(r"\bgetenv\s*\(", line):
                sites.append((os.path.basename(f), i, line.strip()))
    names = sorted(set(re.findall(r'getenv\("(SAPCA_\w+)"\)', " ".join(s[2] for s in sites))))
    assert names == ["SAPCA_AT_OVERLAP", "SAPCA_MULTI_INPROCESS"], names
    assert len(sites) <= 8, sites
    rel = open(L.LIB_PATH, "rb").read()
    for name in (b"SAPCA_AT_SORT", b"SAPCA_AT_NATURAL", b"SAPCA_TRANSPOSE_GATHER", b"SAPCA_FILL_DIRECT", b"SAPCA_COMM_FORCE_RCCL",
                 b"SAPCA_RCCL_LIBRARY", b"SAPCA_UP_CHUNK"):   # (the tests' stand-in for librccl is reachable from the debug build only)
        assert name not in rel, f"the release library carries the switch {name.decode()}"
    assert b"SAPCA_AT_OVERLAP" in rel
    if os.path.exists(L.DEBUG_LIB_PATH):
        dbg = open(L.DEBUG_LIB_PATH, "rb").read()
        assert b"SAPCA_AT_SORT" in dbg and b"SAPCA_COMM_FORCE_RCCL" in dbg and b"SAPCA_RCCL_LIBRARY" in dbg
        lib = L.load_debug()
        for name in L.EXPORTED_SYMBOLS:
            assert hasattr(lib, name), name


def test_switch_list_names_every_switch_read():
    """csrc/switches.h lists the switches of the debug variant by file: exactly the names read through dbg_env / dbg_on."""
    import glob
    src = os.path.join(ROOT, "single-algebra_amd", "csrc")
    read = set()
    for f in glob.glob(os.path.join(src, "*")):
        if os.path.basename(f) != "switches.h":
            read |= set(re.findall(r'\bdbg_(?:env|on)\("(SAPCA_\w+)"\)', open(f, errors="replace").read()))
    header = open(os.path.join(src, "switches.h")).read()
    listed = header[header.index("The switches of the debug variant"):header.index("#pragma once")]
    assert read and read == set(re.findall(r"\bSAPCA_\w+", listed)), (sorted(read), sorted(set(re.findall(r"\bSAPCA_\w+", listed))))


def test_stand_in_librccl_is_test_infrastructure_only():
    """tests/fake_rccl is reached through SAPCA_RCCL_LIBRARY by the debug build and by nothing else: no product source, build
    file or Python module names it, and it exports exactly the entry points csrc/comm.cpp binds."""
    import glob
    prod = glob.glob(os.path.join(ROOT, "single-algebra_amd", "**", "*"), recursive=True) + [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for f in prod:
        if os.path.isfile(f) and not f.endswith((".so", ".o")) and "/build" not in f:
            txt = open(f, errors="replace").read()
            assert "fake_rccl" not in txt or f.endswith(("comm.cpp", "switches.h")), f
    src = open(os.path.join(ROOT, "tests", "fake_rccl", "fake_rccl.c")).read()
    exported = set(re.findall(r'extern "C" __attribute__\(\(visibility\("default"\)\)\) [\w\s\*]+?\b(nccl\w+)\(', src))
    bound = set(re.findall(r'dlsym\(a\.so, "(nccl\w+)"\)', open(os.path.join(ROOT, "single-algebra_amd", "csrc", "comm.cpp")).read()))
    assert exported == bound and len(bound) == 8, (exported, bound)


def test_bench_probes_for_the_reference_binary_and_says_why_not(monkeypatch):
    """bench.py looks for cargo + a registry before any GPU call and reports the reference binary as
    unavailable (with the reason) where they are missing -- as in this image."""
    import importlib.util
    import shutil
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(shutil, "which", lambda name: None)
    r = bench.reference_binary_baseline()
    assert r["available"] is False and "cargo" in r["reason"]
    got, why = bench.measure_traffic("c2", 11)      # no rocprofv3 on PATH (patched): the committed figure is used instead
    assert got is None and "rocprofv3" in why
    sweep, total = bench.alg_bytes(200_000, 20_000, 119_990_071, 60, 50, 4)
    assert sweep == 119_990_071 * 8 + 200_001 * 8 + 20_000 * 60 * 4 + 200_000 * 60 * 4 == 1_014_320_576   # SURVEY.md 8d formula at C2


def test_plain_bench_run_measures_the_headline_alone():
    """bench.py without --full runs no CPU baseline, host path, secondary workload, counter pass or copy-rate run; --full
    runs them all unless a --no-* option leaves one out, and the options that only shape a --full run need it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    skipped = ("no_cpu_baseline", "no_extras", "no_traffic")
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and all(getattr(plain, f) for f in skipped)
    assert (plain.steps, plain.warmup, plain.dump_outputs) == (20, 5, None)
    full = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert full.full and not any(getattr(full, f) for f in skipped)
    trimmed = bench.parse_args(["--full", "--no-traffic", "--cpu-sample-rows", "1000"])
    assert trimmed.no_traffic and not trimmed.no_extras and not trimmed.no_cpu_baseline and trimmed.cpu_sample_rows == 1000
    for only_full in (["--weak-c2"], ["--cpu-sample-rows", "1000"]):
        with pytest.raises(SystemExit):
            bench.parse_args(only_full)

"""CPU side of the opt-in centred Lanczos fit (sapca_options.lanczos_center): the option exists at every layer of the
boundary, is off by default and did not move a byte of the options struct."""
import ctypes as C
import os
import re

import torch  # noqa: F401  (first: one HIP runtime per process)

import sapca
from sapca import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_is_off_by_default_and_the_struct_keeps_its_layout():
    o = L.default_options()
    assert o.lanczos_center == 0
    # the field took the place of a padding byte: size and every offset are those of ABI 4 before it
    assert C.sizeof(L.Options) == 80 and o.struct_size == 80
    assert (L.Options.center.offset, L.Options.verbose.offset, L.Options.collect_timings.offset,
            L.Options.lanczos_center.offset, L.Options.method.offset) == (32, 33, 34, 35, 36)
    assert L.Options.lanczos_center.size == 1
    assert L.load().sapca_abi_version() == 4


def test_builder_method_round_trips():
    for cls in (sapca.SparsePCABuilder, sapca.MaskedSparsePCABuilder):
        b = cls.new()
        assert "lanczos_center" not in b._ext                      # default: not set, the estimator's default is off
        assert b.lanczos_center() is b and b._ext["lanczos_center"] is True
        assert b.lanczos_center(False)._ext["lanczos_center"] is False
    import inspect
    assert inspect.signature(sapca.pca._Estimator.__init__).parameters["lanczos_center"].default is False


def test_header_and_the_other_bindings_name_the_field():
    header = open(os.path.join(ROOT, "include", "sapca.h")).read()
    body = re.search(r"typedef\s+struct\s+sapca_options\s*\{(.*?)\}\s*sapca_options;", header, flags=re.S).group(1)
    assert re.search(r"\buint8_t\s+lanczos_center\s*;", body) and "reserved0" not in body
    assert re.search(r"#define\s+SAPCA_ABI_VERSION\s+4\b", header)
    host = os.path.join(ROOT, "single-algebra_amd", "host")
    assert "pub lanczos_center: u8" in open(os.path.join(host, "rust", "sapca-sys", "src", "lib.rs")).read()
    wrapper = open(os.path.join(host, "rust", "sapca", "src", "lib.rs")).read()
    assert len(re.findall(r"pub fn lanczos_center\(mut self, on: bool\) -> Self", wrapper)) == 2    # both builders
    assert "o.lanczos_center = lanczos_center as u8" in wrapper
    hpp = open(os.path.join(host, "cpp", "sapca.hpp")).read()
    assert "BuilderT& lanczos_center(bool on = true)" in hpp and "o.lanczos_center = lanczos_center" in hpp

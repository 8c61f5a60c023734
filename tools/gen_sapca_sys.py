#!/usr/bin/env python3
"""Writes single-algebra_amd/host/rust/sapca-sys/src/lib.rs from include/sapca.h: one `extern "C"` item per function the
header declares (same name, same argument count and order, C types mapped to their Rust FFI twins), the POD structs, the
enum constants and the SAPCA_CSR_* flags.  Run it after editing the header; tests/test_abi_cpu.py::test_rust_sys_crate_declares_the_whole_header
regenerates in memory and compares with the committed file, and checks name + argument-count agreement independently.

    python tools/gen_sapca_sys.py            # rewrite the crate source
    python tools/gen_sapca_sys.py --check    # exit 1 if the committed file is stale
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sapca.h")
OUT = os.path.join(ROOT, "single-algebra_amd", "host", "rust", "sapca-sys", "src", "lib.rs")

SCALARS = {
    "void": "c_void", "char": "c_char", "int": "c_int", "float": "f32", "double": "f64", "size_t": "usize",
    "uint8_t": "u8", "int32_t": "i32", "uint32_t": "u32", "int64_t": "i64", "uint64_t": "u64",
    "sapca_status": "c_int", "sapca_handle": "sapca_handle", "sapca_multi": "sapca_multi",
    "sapca_options": "sapca_options", "sapca_timings": "sapca_timings", "sapca_csr_report": "sapca_csr_report",
    "sapca_tsne_options": "sapca_tsne_options", "sapca_kmeans_options": "sapca_kmeans_options",
    "sapca_umap_options": "sapca_umap_options", "sapca_louvain_options": "sapca_louvain_options",
    "sapca_hvg_options": "sapca_hvg_options", "sapca_spectral_options": "sapca_spectral_options",
    "sapca_allreduce_fn": "sapca_allreduce_fn",
}


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def rust_type(ctype):
    """'const uint64_t*' -> '*const u64'; 'float**' -> '*mut *mut f32'; 'const int64_t**' -> '*mut *const i64'."""
    t = ctype.strip()
    stars = t.count("*")
    t = t.replace("*", " ").split()
    const = "const" in t
    base = [w for w in t if w not in ("const", "struct")]
    assert len(base) == 1, ctype
    r = SCALARS[base[0]]
    for level in range(stars):
        # the innermost pointer carries the const of the pointee; outer levels are out-parameters
        r = ("*const " if (const and level == 0) else "*mut ") + r
    return r


def parse_functions(header_text):
    """[(name, return C type, [(C type, argument name)])] in declaration order."""
    text = strip_comments(header_text)
    text = text[text.index('extern "C" {'):]
    text = re.sub(r"^\s*#[^\n]*$", "", text, flags=re.M)   # preprocessor lines
    # drop typedefs (structs, enums, function pointer types): they are emitted by hand below
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r"typedef\s+enum\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r"typedef[^;]*;", " ", text)
    out = []
    for m in re.finditer(r"([A-Za-z_][\w \t\*]*?)\b(sapca_\w+)\s*\(([^()]*)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        params = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                arr = re.match(r"(.*?)(\w+)\s*\[\s*\d+\s*\]$", a)   # uint8_t id[128] decays to a pointer
                if arr:
                    params.append((arr.group(1).strip() + "*", arr.group(2)))
                    continue
                mm = re.match(r"(.*?)(\w+)$", a)
                params.append((mm.group(1).strip(), mm.group(2)))
        out.append((name, ret, params))
    return out


def parse_enum_constants(header_text):
    text = strip_comments(header_text)
    consts = []
    for m in re.finditer(r"typedef\s+enum\s+\w+\s*\{(.*?)\}", text, flags=re.S):
        value = -1
        for item in m.group(1).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                name, v = [x.strip() for x in item.split("=")]
                value = int(v, 0)
            else:
                name, value = item, value + 1
            consts.append((name, value))
    return consts


def parse_struct(header_text, name):
    text = strip_comments(header_text)
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        arr = re.match(r"(.*?)(\w+)\s*\[\s*(\d+)\s*\]$", decl)
        if arr:
            fields.append((arr.group(2), "[%s; %s]" % (rust_type(arr.group(1)), arr.group(3))))
            continue
        names = [x.strip() for x in decl.split(",")]   # `uint64_t a, b, c`: one type, several fields
        mm = re.match(r"(.*?)(\w+)$", names[0])
        fields.append((mm.group(2), rust_type(mm.group(1))))
        fields.extend((x, rust_type(mm.group(1))) for x in names[1:])
    return fields


def render(header_text):
    fns = parse_functions(header_text)
    abi = re.search(r"#define\s+SAPCA_ABI_VERSION\s+(\d+)", header_text).group(1)
    lines = []
    w = lines.append
    w("//! Raw bindings to `include/sapca.h` (ABI version %s): every function the header declares, GENERATED by" % abi)
    w("//! `tools/gen_sapca_sys.py` (do not edit; `tests/test_abi_cpu.py` checks this file against the header).")
    w("//! UNTESTED SOURCE in the sense that no rustc has compiled it in the build image (there is none).")
    w("#![allow(non_camel_case_types)]")
    w("use std::os::raw::{c_char, c_int, c_void};")
    w("")
    for opaque, alias in (("sapca_handle_s", "sapca_handle"), ("sapca_multi_s", "sapca_multi")):
        w("#[repr(C)]")
        w("pub struct %s {" % opaque)
        w("    _private: [u8; 0],")
        w("}")
        w("pub type %s = *mut %s;" % (alias, opaque))
    w("")
    w("pub const SAPCA_ABI_VERSION: c_int = %s;" % abi)
    for name, value in parse_enum_constants(header_text):
        ty = "c_int" if name.startswith(("SAPCA_OK", "SAPCA_ERR")) else "i32"
        w("pub const %s: %s = %d;" % (name, ty, value))
    w("")
    w("/// `int (*)(void* ctx, void* buf, uint64_t count, int32_t dtype, void* stream)`")
    w("pub type sapca_allreduce_fn = Option<unsafe extern \"C\" fn(*mut c_void, *mut c_void, u64, i32, *mut c_void) -> c_int>;")
    for name, value in re.findall(r"^#define\s+(SAPCA_CSR_\w+)\s+(\d+)u\b", header_text, flags=re.M):
        w("pub const %s: u32 = %s;" % (name, value))
    for struct in ("sapca_options", "sapca_timings", "sapca_csr_report", "sapca_tsne_options", "sapca_kmeans_options",
                   "sapca_umap_options", "sapca_louvain_options", "sapca_hvg_options", "sapca_spectral_options"):
        w("")
        w("#[repr(C)]")
        w("#[derive(Clone, Copy)]")
        w("pub struct %s {" % struct)
        for fname, fty in parse_struct(header_text, struct):
            w("    pub %s: %s," % (fname, fty))
        w("}")
    w("")
    w("extern \"C\" {")
    for name, ret, params in fns:
        args = ", ".join("%s: %s" % (("r#%s" % p if p in ("fn", "type", "ref", "in", "as") else p), rust_type(t)) for t, p in params)
        rt = "" if ret == "void" else " -> %s" % rust_type(ret)
        w("    pub fn %s(%s)%s;" % (name, args, rt))
    w("}")
    return "\n".join(lines) + "\n"


def main():
    text = render(open(HEADER).read())
    if "--check" in sys.argv:
        if not os.path.exists(OUT) or open(OUT).read() != text:
            print("stale: run python tools/gen_sapca_sys.py", file=sys.stderr)
            sys.exit(1)
        return
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote %s (%d functions)" % (OUT, len(parse_functions(open(HEADER).read()))))


if __name__ == "__main__":
    main()

"""The one parser of include/sapca.h: what tools/gen_sapca_sys.py (the Rust sys crate) and tools/gen_sapca_abi.py (the
Python binding's table) both read.  Everything comes back in declaration order, with C types as the header spells them
(one space between words, no space before a `*`)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sapca.h")


def read_header():
    with open(HEADER) as f:
        return f.read()


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def c_type(words):
    """'const  uint64_t *' -> 'const uint64_t*'"""
    return re.sub(r"\s*\*", "*", " ".join(words.split()))


def parse_functions(header_text):
    """[(name, return C type, [(C type, argument name)])] in declaration order."""
    text = strip_comments(header_text)
    text = text[text.index('extern "C" {'):]
    text = re.sub(r"^\s*#[^\n]*$", "", text, flags=re.M)   # preprocessor lines
    # drop typedefs (structs, enums, function pointer types): the other parsers read those
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r"typedef\s+enum\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r"typedef[^;]*;", " ", text)
    out = []
    for m in re.finditer(r"([A-Za-z_][\w \t\*]*?)\b(sapca_\w+)\s*\(([^()]*)\)\s*;", text):
        ret, name, args = c_type(m.group(1)), m.group(2), m.group(3).strip()
        params = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                arr = re.match(r"(.*?)(\w+)\s*\[\s*\d+\s*\]$", a)   # uint8_t id[128] decays to a pointer
                if arr:
                    params.append((c_type(arr.group(1)) + "*", arr.group(2)))
                    continue
                mm = re.match(r"(.*?)(\w+)$", a)
                params.append((c_type(mm.group(1)), mm.group(2)))
        out.append((name, ret, params))
    return out


def parse_enum_constants(header_text):
    """[(name, value)] of every enumerator."""
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


def parse_defines(header_text):
    """[(name, value, written with a `u` suffix)] of every `#define SAPCA_X <integer>`."""
    text = strip_comments(header_text)
    return [(name, int(value), bool(u)) for name, value, u in re.findall(r"^#define\s+(SAPCA_\w+)\s+(\d+)(u?)\s*$", text, flags=re.M)]


def parse_struct_names(header_text):
    """The POD structs the header defines (`typedef struct X { ... } X;`; the opaque handle types have no body)."""
    return re.findall(r"typedef\s+struct\s+(\w+)\s*\{", strip_comments(header_text))


def parse_struct(header_text, name):
    """[(field, C type, array length or 0)]"""
    text = strip_comments(header_text)
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        arr = re.match(r"(.*?)(\w+)\s*\[\s*(\d+)\s*\]$", decl)
        if arr:
            fields.append((arr.group(2), c_type(arr.group(1)), int(arr.group(3))))
            continue
        names = [x.strip() for x in decl.split(",")]   # `uint64_t a, b, c`: one type, several fields
        mm = re.match(r"(.*?)(\w+)$", names[0])
        fields.append((mm.group(2), c_type(mm.group(1)), 0))
        fields.extend((x, c_type(mm.group(1)), 0) for x in names[1:])
    return fields

"""The C ABI as include/r3d_hip.h states it, read once: constants, structs and prototypes.  The header is the single
statement of the ABI; r3d_amd/_lib.py builds its ctypes classes and argtypes from what parse() returns.  The parser
fails loudly and never guesses: text it does not understand raises ValueError quoting that text."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "r3d_hip.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}

_INT = r"\(?\s*(-?\d+)\s*\)?"
_DECL = r"((?:const\s+)?\w+(?:\s*\*(?:\s*const\b)?)*)\s*(\w+)"          # "<type> <name>"; the stars belong to the type


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def ctype_of(ctype, classes=None):
    """The ctypes class of a C type as parse() spells it; `classes` maps the names of structs that appear by value."""
    if ctype.endswith("*"):
        return C.c_char_p if ctype == "char*" else C.c_void_p
    return SCALARS[ctype] if ctype in SCALARS else classes[ctype]


def pointee(ctype):
    """`const uint8_t*` -> `uint8_t`: what a pointer type points to, const dropped."""
    assert ctype.endswith("*"), ctype
    return ctype[:-1].replace("const ", "")


def _ctype(text, where, structs=()):
    ctype = re.sub(r"\s*\*\s*", "*", " ".join(text.split()))
    if not (ctype.endswith("*") or ctype in SCALARS or ctype in structs):
        raise ValueError(f"r3d_hip.h: unknown type {ctype!r} in {where!r}")
    return ctype


def _fields(body, consts, structs):
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = (p.strip() for p in decl.split(","))
        m = re.fullmatch(_DECL + r"(?:\s*\[\s*(\w+)\s*\])?", first)
        if not m or not all(re.fullmatch(r"\w+", p) for p in more):
            raise ValueError(f"r3d_hip.h: cannot parse the struct field declaration {decl!r}")
        n = m.group(3) and (int(m.group(3)) if m.group(3).isdigit() else consts[m.group(3)])
        out += [(name, _ctype(m.group(1), decl, structs), n) for name in (m.group(2), *more)]
    return out


def _params(text, proto):
    out = []
    for p in ([] if text.strip() == "void" else text.split(",")):
        m = re.fullmatch(_DECL, p.strip())
        if not m:
            raise ValueError(f"r3d_hip.h: cannot parse the parameter {p.strip()!r} of {proto!r}")
        out.append((_ctype(m.group(1), proto), m.group(2)))
    return out


def parse(text=None):
    """-> (consts {name: int}, structs [(C name, [(field, C type, array length or None)])],
    functions [(name, return C type, [(C type, parameter name)])]), each in header order."""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    text = strip_comments(text)
    consts = {name: int(v) for name, v in
              re.findall(r"^[ \t]*#[ \t]*define[ \t]+(R3D_\w+)[ \t]+" + _INT + r"[ \t]*$", text, flags=re.M)}
    structs, funcs = [], []

    def enum(m):
        for item in filter(None, (i.strip() for i in m.group(1).split(","))):
            e = re.fullmatch(r"(R3D_\w+)\s*=\s*" + _INT, item)
            if not e:
                raise ValueError(f"r3d_hip.h: cannot parse the enumerator {item!r}")
            consts[e.group(1)] = int(e.group(2))
        return ""

    def struct(m):
        if m.group(1) != m.group(3):
            raise ValueError(f"r3d_hip.h: struct {m.group(1)!r} is typedef'd as {m.group(3)!r}")
        structs.append((m.group(1), _fields(m.group(2), consts, [s for s, _ in structs])))
        return ""

    def proto(m):
        where = " ".join(m.group(0).split())
        funcs.append((m.group(2), _ctype(m.group(1), where), _params(m.group(3), where)))
        return ""

    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)                 # preprocessor lines: the defines are taken above
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    text = re.sub(r"enum\s*\{([^}]*)\}\s*;", enum, text)
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"(\w+)\s+(r3d_\w+)\s*\(([^)]*)\)\s*;", proto, text)
    if text.split() not in ([], ["}"]):                                 # "}" closes extern "C"
        raise ValueError(f"r3d_hip.h: unparsed text {' '.join(text.split())!r}")
    return consts, structs, funcs

"""The ctypes binding (r3d_amd/_lib.py) is derived from include/r3d_hip.h by r3d_amd/_abi.py.  These tests hold the
derivation against the C compiler's own layout of the header, against hand-written pins of representative prototypes,
and against an independent count of the prototypes; and they show that text the parser does not understand raises.
No GPU is needed: nothing here launches a kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from r3d_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "r3d_hip.h")


@pytest.fixture(scope="module")
def parsed():
    return _abi.parse()


@pytest.fixture(scope="module")
def lib():
    from r3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _host_cc():
    if shutil.which("cc"):
        return ["cc"]
    for clang in (shutil.which("clang"), "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        if clang and os.path.exists(clang):
            return [clang, "-x", "c"]
    return None


def test_struct_layout_matches_the_compiler(parsed, tmp_path):
    """sizeof of every struct and offsetof of every field, as the host C compiler lays the header out, equal what ctypes
    computes for the derived classes."""
    from r3d_amd import _lib
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler (cc, or ROCm's clang)")
    _, structs, _ = parsed
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "r3d_hip.h"', "int main(void) {"]
    for cname, fields in structs:
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{n} %zu\\n", offsetof({cname}, {n}));' for n, _, _ in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(cc + ["-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    compared = 0
    assert len(structs) >= 19
    for cname, fields in structs:
        cls = _lib.STRUCTS[cname]
        assert fields and [n for n, _, _ in fields] == [f[0] for f in cls._fields_], cname
        assert int(got[cname]) == C.sizeof(cls), cname
        compared += 1
        for n, _, _ in fields:
            assert int(got[f"{cname}.{n}"]) == getattr(cls, n).offset, (cname, n)
            compared += 1
    assert compared == len(got) == len(structs) + sum(len(f) for _, f in structs) >= 543


_I, _L, _F, _P, _D, _I32, _U64 = C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_double, C.c_int32, C.c_uint64

PINS = {
    "r3d_abi_version": ([], _I),
    "r3d_build_info": ([C.c_char_p, _I], _I),
    "r3d_gemm_partial_floats": ([_I32, _I32, _I32], _L),
    "r3d_token_select": ([_P, _P, _D, _I, _I, _I, _P, _P, _P, _P], _I),
    "r3d_adamw_flat_dropout": ([_P, _P, _P, _P, _L, _P, _P, _F, _F, _F, _F, _F, _P, _L, _F, _U64, _P, _P], _I),
    "r3d_gemm_grouped_launch": ([_P, _P, _P, _I, _I, _I, _I, _P], _I),
    "r3d_layernorm_bwd": ([_P, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _F,
                           _P, _P, _P, _I, _I, _I, _P], _I),
    "r3d_clip_collate_tracks": ([_P, _P], _I),
}


@pytest.mark.parametrize("name", sorted(PINS))
def test_signature_pins(lib, name):
    argtypes, restype = PINS[name]
    fn = getattr(lib, name)
    assert list(fn.argtypes) == argtypes and fn.restype is restype, (name, fn.argtypes, fn.restype)


def test_every_prototype_is_bound(lib, parsed):
    """The parser drops no prototype (an independent regex counts them) and load() types every one."""
    from r3d_amd import _lib
    _, _, funcs = parsed
    declared = set(re.findall(r"\b(r3d_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    declared.discard("r3d_gemm_desc")
    assert len(declared) >= 153 and len(funcs) == len(declared) == len(_lib.EXPORTS)
    assert [f[0] for f in funcs] == list(_lib.EXPORTS) and set(_lib.EXPORTS) == declared
    for name, _, params in funcs:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name


_MINIMAL = '#define R3D_N 2\ntypedef struct r3d_s { const float* a; int32_t b, c; } r3d_s;\nint r3d_f(const r3d_s* s, void* stream);\n'


def test_parser_reads_a_minimal_header():
    assert _abi.parse(_MINIMAL) == ({"R3D_N": 2}, [("r3d_s", [("a", "const float*", None), ("b", "int32_t", None),
                                                                ("c", "int32_t", None)])],
                                    [("r3d_f", "int", [("const r3d_s*", "s"), ("void*", "stream")])])


@pytest.mark.parametrize("extra, quoted", [
    ("typedef struct r3d_t { int32_t n; long double x; } r3d_t;", "long double x"),
    ("int r3d_g(long double x, void* stream);", "long double x"),
    ("int r3d_g(unsigned n, void* stream);", "unsigned"),
    ("typedef struct r3d_t { short n; } r3d_t;", "short"),
    ("static int z;", "static int z;"),
])
def test_parser_fails_loudly(extra, quoted):
    with pytest.raises(ValueError, match=re.escape(quoted)):
        _abi.parse(_MINIMAL + extra + "\n")


def test_constants_come_from_the_header(parsed):
    from r3d_amd import _lib
    consts, _, _ = parsed
    today = {"ABI_VERSION": 2, "GEMM_NT": 0, "GEMM_NN": 1, "GEMM_TN": 2, "CLIP_MAX_TRACKS": 8, "CLIP_WIDE_ROW": 256,
             "CLIP_FRAMES_F32": 0, "CLIP_WORDS_I64": 1, "CLIP_WORDS_F32": 2, "EINVAL": -1, "EALIGN": -2, "ENORCCL": -3,
             "ERCCL_BASE": -100}
    for name, value in today.items():
        assert getattr(_lib, name) == consts["R3D_" + name] == value, name
    with pytest.raises(_lib.R3DHipError, match=re.escape("x failed: R3D_EALIGN (misaligned pointer / leading dimension)")):
        _lib.check(-2, "x")
    with pytest.raises(_lib.R3DHipError, match="x failed: ncclResult_t 5 from RCCL"):
        _lib.check(-105, "x")


def _name_rule(name):
    """The rule the chain blocks used before the header's pointee types were read."""
    return torch.uint8 if name.startswith("drop_") else (torch.int64 if name == "key_label" else torch.float32)


@pytest.mark.parametrize("cname, n_operands, n_planes", [("r3d_fuser_chain_fwd_args", 51, 6), ("r3d_fuser_chain_bwd_args", 64, 6),
                                                         ("r3d_decoder_chain_args", 33, 6)])
def test_chain_blocks_follow_the_header(parsed, cname, n_operands, n_planes):
    """The operand and plane lists of ops' chain argument blocks are the header's pointer fields in order, and the dtype
    read from each pointee is what the earlier name rule gave, for every operand."""
    from r3d_amd import _lib, ops
    fields = dict(parsed[1])[cname]
    pointers = [(n, t) for n, t, _ in fields if t.endswith("*")]
    cls = _lib.STRUCTS[cname]
    cls()                                                       # constructs
    operands, planes = ops.chain_operands(cls)
    assert [n for n, _ in pointers] == list(operands) + ["timeline"] + planes
    assert planes == [n for n, _ in pointers if n.startswith("pl_")] and len(planes) == n_planes
    assert len(operands) == n_operands
    for name, dtype in operands.items():
        assert dtype == _name_rule(name), name
    pointee = {"uint8_t": torch.uint8, "int64_t": torch.int64, "float": torch.float32}
    for n, t in pointers:
        if n in operands:
            assert operands[n] == pointee[t.replace("const ", "").rstrip("*")], n
    users = {"r3d_fuser_chain_fwd_args": ops.FuserChainFwd, "r3d_fuser_chain_bwd_args": ops.FuserChainBwd,
             "r3d_decoder_chain_args": ops.DecoderChain}[cname]
    assert users.STRUCT is cls and users.OPTIONAL <= set(operands)
    assert all(getattr(cls, k).size == 4 for k in users.DIMS)

"""ctypes binding of libr3d_hip.so, derived from include/r3d_hip.h (r3d_amd/_abi.py reads it): the header is the single
statement of the C ABI.  There is NO fallback: if the library is missing or stale the import of the compute path fails
loudly -- the product never runs on a CPU/PyTorch substitute.

Built here at import, from the header alone:
  - every `#define R3D_X n` and enumerator as X (ABI_VERSION, GEMM_NT / NN / TN, CLIP_MAX_TRACKS, CLIP_WIDE_ROW,
    CLIP_FRAMES_F32, CLIP_WORDS_I64, CLIP_WORDS_F32, the error codes, ...);
  - every `struct r3d_some_name` as the ctypes.Structure SomeName (GemmDesc, LnFwdJob, LnBwdJob, GemmLnJob,
    FuserChainFwdArgs, FuserChainBwdArgs, DecoderChainArgs, PlaneJob, MhaJob, MhaBwdJob, RowsumJob, TailLossesArgs,
    LossFinalizeJob, LnFinalizeJob, ClipCollateJob, ClipTrack, ClipTracksJob, AfftHeadArgs, CnnSegArgs); its C_TYPES maps
    each field to the C type the header gives it;
  - EXPORTS and the argtypes / restype that load() sets.
Device addresses travel as integers (tensor.data_ptr()): every pointer but `char*` is a c_void_p."""
import ctypes as C
import os

from . import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "libr3d_hip.so")

_CONSTS, _STRUCTS, _FUNCTIONS = _abi.parse()
globals().update({name[len("R3D_"):]: value for name, value in _CONSTS.items()})

STRUCTS = {}                            # C name -> class, in header order


def _struct(cname, fields):
    def field_class(ctype, length):
        cls = _abi.ctype_of(ctype, STRUCTS)
        return cls * length if length else cls
    return type("".join(p.capitalize() for p in cname[len("r3d_"):].split("_")), (C.Structure,), {
        "__doc__": f"struct {cname} (include/r3d_hip.h).",
        "_fields_": [(n, field_class(t, k)) for n, t, k in fields],
        "C_TYPES": {n: t for n, t, _ in fields}})


for _cname, _fields in _STRUCTS:
    STRUCTS[_cname] = _struct(_cname, _fields)
globals().update({cls.__name__: cls for cls in STRUCTS.values()})

EXPORTS = tuple(name for name, _, _ in _FUNCTIONS)

_lib = None


class R3DHipError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes library.  Raises R3DHipError with build instructions if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise R3DHipError(
            f"{LIB_PATH} is missing: the HIP kernels are the only compute path of r3d_amd (no CPU/PyTorch fallback). "
            f"Build it with `python -m r3d_amd.build` (needs hipcc; cross-compiles for gfx950 without a GPU).")
    lib = C.CDLL(LIB_PATH)
    for name, ret, params in _FUNCTIONS:
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise R3DHipError(f"{LIB_PATH} does not export {name}: stale build, run `python -m r3d_amd.build --force`") from e
        fn.argtypes = [_abi.ctype_of(t) for t, _ in params]
        fn.restype = _abi.ctype_of(ret)
    v = lib.r3d_abi_version()
    if v != _CONSTS["R3D_ABI_VERSION"]:
        raise R3DHipError(f"libr3d_hip.so ABI {v} != expected {_CONSTS['R3D_ABI_VERSION']}: rebuild with "
                          f"`python -m r3d_amd.build --force`")
    _lib = lib
    return lib


_ERR = {_CONSTS["R3D_EINVAL"]: "R3D_EINVAL (rejected argument)",
        _CONSTS["R3D_EALIGN"]: "R3D_EALIGN (misaligned pointer / leading dimension)",
        _CONSTS["R3D_ENORCCL"]: "R3D_ENORCCL (no RCCL mapped into the process)"}


def check(rc, what):
    if rc <= _CONSTS["R3D_ERCCL_BASE"]:
        raise R3DHipError(f"{what} failed: ncclResult_t {_CONSTS['R3D_ERCCL_BASE'] - rc} from RCCL")
    if rc != 0:
        raise R3DHipError(f"{what} failed: {_ERR.get(rc, f'hipError_t {rc}' if rc > 0 else rc)}")


def build_info():
    buf = C.create_string_buffer(128)
    check(load().r3d_build_info(buf, 128), "r3d_build_info")
    return buf.value.decode()

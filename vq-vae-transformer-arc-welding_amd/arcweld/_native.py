"""ctypes binding of the HIP C ABI, read from include/arcweld_amd.h at import.

The header is the single source of the binding: its integer constants, argument structs and prototypes are parsed
here (``parse_header``), nothing is mirrored by hand.  What the parser cannot read it refuses (NativeError).

The library is loaded AFTER ``import torch`` so that its ``libamdhip64.so.7`` dependency resolves (by SONAME) to
the HIP runtime torch already loaded: device pointers, streams and the caching allocator are then shared.
There is no fallback: if the library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch  # noqa: F401  (must precede the library load, see module docstring)

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ARCWELD_LIB overrides the library path (A/B timing of two builds of one ABI in one process tree: tools/ab_bench.sh)
LIB_PATH = os.environ.get("ARCWELD_LIB") or os.path.join(PKG_DIR, "lib", "libarcweld_amd.so")
HEADER = os.path.join(os.path.dirname(PKG_DIR), "include", "arcweld_amd.h")


class NativeError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
            "float": ctypes.c_float, "double": ctypes.c_double}
# <const> <type> <stars, each optionally const> <the rest: declarators or a parameter name>
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)(.*)", re.S)
_PREPROCESSOR_NOISE = re.compile(r"#\s*(?:ifndef\s+\w+|ifdef\s+\w+|endif|include\s*<[\w./]+>|define\s+\w+)")


def parse_header(text: str):
    """(constants, structs, prototypes) of a C header in the dialect of include/arcweld_amd.h.

    constants: name -> int, from ``enum { NAME = n, ... };`` and ``#define NAME <integer>``;
    structs: C name -> ctypes.Structure subclass, from ``typedef struct { ... } name;`` (scalars by type, every
    pointer a c_void_p, ``T name[N]`` an array of N); prototypes: name -> (restype, argtypes), a pointer to one of the
    header's structs as POINTER(that Structure), any other pointer as c_void_p.
    Anything else -- an unknown type, declarator, directive or declaration -- raises NativeError naming it."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    constants, structs, prototypes, code, in_cpp = {}, {}, {}, [], False
    for line in text.splitlines():
        s = line.strip()
        m = re.fullmatch(r"#\s*define\s+(\w+)\s+(-?(?:0[xX][0-9a-fA-F]+|\d+))", s)
        if m:
            constants[m.group(1)] = int(m.group(2), 0)
        elif s.startswith("#"):
            if not _PREPROCESSOR_NOISE.fullmatch(s):
                raise NativeError(f"header: cannot read the directive `{s}`")
            in_cpp = s.split() == ["#ifdef", "__cplusplus"]
        elif not in_cpp:
            code.append(line)
        elif s not in ("", 'extern "C" {', "}"):    # a __cplusplus guard holds one of these two lines
            raise NativeError(f"header: cannot read `{s}` inside #ifdef __cplusplus")
    text = "\n".join(code)

    def ctype(base, stars, what, pointee_structs=False):
        if base not in _SCALARS and base not in structs and not (stars and base in ("void", "char")):
            raise NativeError(f"header: unknown type `{base}` in `{what}`")
        if not stars:
            if base in structs:
                raise NativeError(f"header: a struct by value in `{what}`")
            return _SCALARS[base]
        if pointee_structs and base in structs and stars.count("*") == 1:
            return ctypes.POINTER(structs[base])
        return ctypes.c_void_p

    def fields(body, cname):
        out = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            what = f"{decl}; of {cname}"
            m = _DECL.fullmatch(decl)
            if not m:
                raise NativeError(f"header: cannot read `{what}`")
            base, stars, rest = m.groups()
            names = [d.strip() for d in rest.split(",")]
            if stars and len(names) > 1:
                raise NativeError(f"header: several declarators after a pointer type in `{what}`")
            t = ctype(base, stars, what)
            for d in names:
                m = re.fullmatch(r"(\w+)(?:\s*\[\s*(\w+)\s*\])?", d)
                if not m:
                    raise NativeError(f"header: cannot read the declarator `{d}` in `{what}`")
                name, dim = m.groups()
                if dim is not None and not dim.isdigit() and dim not in constants:
                    raise NativeError(f"header: array size `{dim}` is not defined in `{what}`")
                out.append((name, t if dim is None else t * (int(dim) if dim.isdigit() else constants[dim])))
        return out

    pos = 0
    item = re.compile(r"\s*(?:enum\s*\{(?P<enum>[^{}]*)\}\s*;"
                      r"|typedef\s+struct\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;"
                      r"|(?P<ret>[^;{}()]+?)\b(?P<fn>\w+)\s*\((?P<params>[^;{}()]*)\)\s*;)")
    while text[pos:].strip():
        m = item.match(text, pos)
        if not m:
            raise NativeError("header: cannot read the declaration `"
                              + " ".join(text[pos:].split(";")[0].split()) + "`")
        pos = m.end()
        if m.group("enum") is not None:
            for member in filter(None, (e.strip() for e in m.group("enum").split(","))):
                mm = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", member)
                if not mm:
                    raise NativeError(f"header: cannot read the enum member `{member}`")
                constants[mm.group(1)] = int(mm.group(2))
        elif m.group("struct") is not None:
            cname = m.group("struct")
            structs[cname] = type(cname, (ctypes.Structure,), {"_fields_": fields(m.group("body"), cname),
                                                               "__doc__": f"{cname} (include/arcweld_amd.h)"})
        else:
            fn = m.group("fn")
            what = " ".join(m.group(0).split())
            rm = _DECL.fullmatch(m.group("ret").strip())
            if not rm or rm.group(3).strip():
                raise NativeError(f"header: cannot read the return type of `{what}`")
            base, stars = rm.group(1), rm.group(2)
            restype = ctypes.c_char_p if (base, stars.count("*")) == ("char", 1) else ctype(base, stars, what)
            argtypes = []
            params = m.group("params").strip()
            for p in ([] if params == "void" else params.split(",")):
                pm = _DECL.fullmatch(p.strip())
                if not pm or not re.fullmatch(r"\w*", pm.group(3).strip()):
                    raise NativeError(f"header: cannot read the parameter `{p.strip()}` of `{what}`")
                argtypes.append(ctype(pm.group(1), pm.group(2), what, pointee_structs=True))
            prototypes[fn] = (restype, argtypes)
    return constants, structs, prototypes


def _read_header():
    try:
        with open(HEADER) as f:
            return parse_header(f.read())
    except OSError as e:
        raise NativeError(f"the C ABI header {HEADER} cannot be read: {e}") from e


_CONSTANTS, _STRUCTS, _PROTOTYPES = _read_header()
globals().update(_CONSTANTS)        # AW_F32, AW_RES_CHAIN_MAX, AW_ABI_VERSION, ...: every header constant, by its name
# the short names that tests/ compare with the header's text: the header's values under another name, not copies
OPS_PER_SEG, BEAM_MAX_W = _CONSTANTS["AW_OPS_PER_SEG"], _CONSTANTS["AW_BEAM_MAX_W"]
KNN_MAX_K, KNN_MAX_SPLITS = _CONSTANTS["AW_KNN_MAX_K"], _CONSTANTS["AW_KNN_MAX_SPLITS"]

GemmArgs = _STRUCTS["aw_gemm_args"]
RelayoutJob = _STRUCTS["aw_relayout_job"]
OperandDesc = _STRUCTS["aw_operand_desc"]
ResChainFwdArgs = _STRUCTS["aw_res_chain_fwd_args"]
ResChainBwdArgs = _STRUCTS["aw_res_chain_bwd_args"]
SampleArgs = _STRUCTS["aw_sample_args"]
BeamArgs = _STRUCTS["aw_beam_args"]
EnsembleArgs = _STRUCTS["aw_ensemble_args"]

# name -> argtypes of every prototype the header declares
SIGNATURES = {name: argtypes for name, (_, argtypes) in _PROTOTYPES.items()}

_lib = None


def load(path: str = LIB_PATH):
    """Load (once) and return the ctypes library with typed entry points."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NativeError(f"HIP library not built: {path} is missing (run `python -c 'import __graft_entry__ as g; "
                          f"g.build()'` or `make -C vq-vae-transformer-arc-welding_amd/csrc`)")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    lib.aw_version.restype, lib.aw_version.argtypes = _PROTOTYPES["aw_version"]
    # entry points keep their names across ABI versions while their parameter lists change: a stale build would be
    # called with the wrong arguments, so it is refused before anything else is looked up
    if lib.aw_version() != AW_ABI_VERSION:  # noqa: F821  (a header constant)
        raise NativeError(f"{path} reports C ABI version {lib.aw_version()}, include/arcweld_amd.h declares "
                          f"{AW_ABI_VERSION}: rebuild the library from this tree")  # noqa: F821
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def call(name: str, *args) -> None:
    lib = load()
    status = getattr(lib, name)(*args)
    if status != 0:
        raise NativeError(f"{name} failed ({status}): {lib.aw_last_error().decode(errors='replace')}")


def stream_ptr(stream=None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def ptr(t):
    """Raw device pointer of a tensor (None -> NULL).  CPU tensors are rejected: no host fallback exists."""
    if t is None:
        return None
    if not t.is_cuda:
        raise NativeError("arcweld HIP kernels need device tensors (got a CPU tensor); there is no CPU fallback")
    return t.data_ptr()


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return AW_F32  # noqa: F821
    if dt == torch.bfloat16:
        return AW_BF16  # noqa: F821
    raise NativeError(f"unsupported operand dtype {dt}")

"""CPU-side checks of the C ABI boundary: the library loads (no GPU needed to dlopen) and exports exactly the entry
points that include/arcweld_amd.h declares; the Python binding is read from that header (arcweld/_native.py
parse_header), and what it reads is checked against the host C compiler's view of the same file."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO


def _declared():
    src = open(os.path.join(REPO, "include", "arcweld_amd.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(aw_\w+)\s*\(", src, re.M)))


def test_header_declares_entry_points():
    names = _declared()
    assert "aw_gemm" in names and "aw_vq_forward" in names and len(names) >= 25


def test_library_exports_every_declared_symbol():
    from arcweld import _native
    lib = _native.load()
    missing = [n for n in _declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_binding_covers_every_declared_symbol():
    from arcweld import _native
    missing = [n for n in _declared() if n not in _native.SIGNATURES and n != "aw_last_error"]
    assert not missing, missing


def test_cpu_tensors_are_rejected():
    import torch
    from arcweld import _native
    with pytest.raises(_native.NativeError):
        _native.ptr(torch.zeros(3))


def _tool(*names):
    """The first of `names` that exists (a bare name is looked up on PATH)."""
    for n in names:
        p = n if os.path.isabs(n) and os.access(n, os.X_OK) else shutil.which(n)
        if p:
            return p
    pytest.fail(f"none of {names} found: the check needs one of them")


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof of every struct and offsetof / sizeof of every field the parser found, as the host C compiler lays the
    header out, against the ctypes classes built from it (aw_gemm_args' 47 fields and the chain structs' macro-sized
    arrays included)."""
    from arcweld import _native
    structs = _native._STRUCTS
    assert {"aw_gemm_args", "aw_relayout_job", "aw_operand_desc", "aw_res_chain_fwd_args", "aw_res_chain_bwd_args",
            "aw_sample_args", "aw_beam_args", "aw_ensemble_args"} <= set(structs)
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "arcweld_amd.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} - %zu 0\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu %zu\\n", sizeof((({cname}*)0)->{fname}), '
                         f"offsetof({cname}, {fname}));")
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    cc = _tool("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang")
    subprocess.run([cc, "-std=c99", "-I", os.path.dirname(_native.HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for cname, fname, size, offset in (ln.split() for ln in out.splitlines()):
        cls = structs[cname]
        if fname == "-":
            assert ctypes.sizeof(cls) == int(size), cname
        else:
            f = getattr(cls, fname)
            assert (f.size, f.offset) == (int(size), int(offset)), f"{cname}.{fname}"
        seen += 1
    assert seen == sum(1 + len(c._fields_) for c in structs.values()) and seen > 150


def test_parser_reads_the_header_dialect_from_a_snippet():
    from arcweld import _native
    consts, structs, protos = _native.parse_header(
        "/* a comment with int aw_not_a_prototype(void); inside */\n"
        "#define AW_N 3\n"
        "enum { AW_A = 0, AW_B = -2 };\n"
        "typedef struct {\n  int M, N;   // two declarators\n  const void* A; int64_t lda; int a_trans;\n"
        "  double* w[AW_N]; uint64_t seed[2];\n} aw_t;\n"
        "int64_t aw_f(const aw_t* a, const aw_t* const* many, const float* x, float y, uint32_t* z, void* stream);\n"
        "const char* aw_g(void);\n")
    assert consts == {"AW_N": 3, "AW_A": 0, "AW_B": -2}
    t = structs["aw_t"]
    assert [n for n, _ in t._fields_] == ["M", "N", "A", "lda", "a_trans", "w", "seed"]
    kinds = dict(t._fields_)
    assert kinds["M"] is ctypes.c_int and kinds["A"] is ctypes.c_void_p and kinds["lda"] is ctypes.c_int64
    assert kinds["w"] is ctypes.c_void_p * 3 and kinds["seed"] is ctypes.c_uint64 * 2
    assert protos == {"aw_f": (ctypes.c_int64, [ctypes.POINTER(t), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float,
                                                ctypes.c_void_p, ctypes.c_void_p]),
                      "aw_g": (ctypes.c_char_p, [])}


@pytest.mark.parametrize("snippet, names", [
    ("int aw_f(long n, void* stream);", ("long", "aw_f")),                               # unknown parameter type
    ("long aw_f(int n);", ("long", "aw_f")),                                             # unknown return type
    ("typedef struct { int a; int (*cb)(int); } aw_s;", ("cb", "aw_s")),                 # function pointer field
    ("typedef struct { float w[AW_NOPE]; } aw_s;", ("AW_NOPE", "aw_s")),                 # undefined array size
    ("typedef struct { unsigned n; } aw_s;", ("unsigned", "aw_s")),                      # unknown field type
    ("typedef struct { int* a, b; } aw_s;", ("int* a, b", "aw_s")),                      # is b a pointer?
    ("int aw_f(int (*cb)(int));", ("aw_f",)),                                            # function pointer parameter
    ("int aw_f(int n[4]);", ("n[4]", "aw_f")),                                           # array parameter
    ("enum { AW_A, AW_B };", ("AW_A",)),                                                 # implicit enum values
    ("#define AW_SHIFT (1 << 3)", ("AW_SHIFT",)),                                        # not a plain integer
    ("struct aw_s { int a; };", ("struct aw_s",)),                                       # not the typedef form
    ("int aw_f(int n)", ("aw_f",)),                                                      # no terminating ;
])
def test_parser_refuses_what_it_cannot_read(snippet, names):
    from arcweld import _native
    with pytest.raises(_native.NativeError) as e:
        _native.parse_header(snippet)
    assert all(n in str(e.value) for n in names), str(e.value)


def test_library_exports_only_declared_symbols():
    """Every aw_* dynamic symbol of the built library is declared in the header: no forwarder outlives its
    prototype."""
    from arcweld import _native
    nm = _tool("nm", "llvm-nm", "/opt/rocm/llvm/bin/llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", _native.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("aw_")}
    assert exported and exported == set(_native._PROTOTYPES), sorted(exported ^ set(_native._PROTOTYPES))
    assert set(_native._PROTOTYPES) == set(_declared())


def test_a_library_of_another_abi_version_is_refused(monkeypatch):
    from arcweld import _native
    assert _native.load().aw_version() == _native.AW_ABI_VERSION == 2
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "AW_ABI_VERSION", 3)
    with pytest.raises(_native.NativeError) as e:
        _native.load()
    msg = str(e.value)
    assert "version 2" in msg and "declares 3" in msg and _native.LIB_PATH in msg
    assert _native._lib is None

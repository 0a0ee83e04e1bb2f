"""The kernel library's C ABI has one declaration, ``csrc/kernels/piamd_kernels.h``: the sources
define exactly what it declares, ``ops/_lib.py`` derives the ctypes signatures from it, the
hand-written ctypes struct mirrors match the compiled structs, and a library that lacks a declared
symbol is refused."""
import ctypes
import glob
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_longlong, c_uint64, c_void_p

import pytest

from paddle_infer_amd import _build
from paddle_infer_amd.ops import _lib

HEADER = os.path.join(_build.KDIR, "piamd_kernels.h")


def test_header_declares_what_the_sources_define():
    defined = []
    for src in glob.glob(os.path.join(_build.KDIR, "*.hip")):
        with open(src, encoding="utf-8") as f:
            defined += re.findall(r"^PIAMD_EXPORT\s+[\w\s]+?\b(piamd_\w+)\s*\(", f.read(), re.M)
    declared = _lib.parse_header(HEADER)
    assert len(defined) == len(set(defined)), sorted(n for n in defined if defined.count(n) > 1)
    assert set(defined) == set(declared), sorted(set(defined) ^ set(declared))
    assert len(declared) > 50
    suffixed = [n for n in declared if n[-1].isdigit() or n.endswith("_ex")]
    assert not suffixed, suffixed


def test_parser_pinned_signatures():
    sigs = _lib.parse_header(HEADER)
    assert sigs["piamd_layernorm_fwd"] == (c_int, [c_int] + [c_void_p] * 9 + [
        c_int, c_int, c_float, c_float, c_uint64, c_uint64, c_int, c_void_p])
    assert sigs["piamd_layernorm_bwd_ws"] == (c_longlong, [c_int, c_int])
    assert sigs["piamd_agemm_load"] == (c_int, [c_char_p])
    assert sigs["piamd_fa_fwd"] == (c_int, [POINTER(_lib.FaArgs), c_int, c_void_p])
    assert sigs["piamd_decode_mega"][1][0] is POINTER(_lib.MegaArgs)
    assert sigs["piamd_decode_head_greedy"][1] == [POINTER(_lib.HeadArgs), c_int, c_void_p]
    assert sigs["piamd_fa_asm_loaded"] == (c_int, [])


def test_parser_type_map(tmp_path):
    h = tmp_path / "h.h"
    h.write_text("// PIAMD_EXPORT int piamd_commented_out(int a);\n"
                 "PIAMD_EXPORT long long piamd_a(const long long* p, long long n, unsigned long long s,\n"
                 "                           uint64_t t, float f,  // trailing comment, with a comma\n"
                 "                           const char* name, hipStream_t st);\n"
                 "PIAMD_EXPORT int piamd_b(void);\n")
    assert _lib.parse_header(str(h)) == {
        "piamd_a": (c_longlong, [c_void_p, c_longlong, c_uint64, c_uint64, c_float, c_char_p, c_void_p]),
        "piamd_b": (c_int, [])}
    for bad in ("PIAMD_EXPORT int piamd_bad(double v);", "PIAMD_EXPORT int piamd_bad(int a, size_t n);",
                "PIAMD_EXPORT double piamd_bad(int a);"):
        h.write_text(bad + "\n")
        with pytest.raises(TypeError, match="piamd_bad"):
            _lib.parse_header(str(h))


def test_struct_mirrors_match_compiled_layout(tmp_path):
    mirrors = {"FaArgs": _lib.FaArgs, "MegaArgs": _lib.MegaArgs, "HeadArgs": _lib.HeadArgs}
    # only the plain struct headers: they must compile without any HIP header
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "fa_args.h"', '#include "decode_args.h"',
             "int main() {"]
    for name, cls in mirrors.items():
        lines.append(f'  std::printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  std::printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.cc"
    src.write_text("\n".join(lines + ["}"]) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-Wno-invalid-offsetof", f"-I{_build.KDIR}", str(src), "-o", str(exe)],
                   check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    want = []
    for name, cls in mirrors.items():
        want.append(f"{name} {ctypes.sizeof(cls)}")
        want += [f"{name}.{f} {getattr(cls, f).offset}" for f, _ in cls._fields_]
    assert got == want + [""]
    assert ctypes.sizeof(_lib.HeadArgs) == 136


@pytest.mark.skipif(not os.path.exists(_lib.lib_path()), reason="kernel library not built")
def test_stale_library_is_refused(tmp_path):
    k = _lib._load()  # every declared name resolves in the built library
    for name, (restype, argtypes) in _lib.parse_header(HEADER).items():
        fn = getattr(k, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert _lib.has("piamd_layernorm_fwd") and not _lib.has("piamd_not_declared")
    with pytest.raises(AttributeError, match="piamd_not_declared"):
        _lib.call("piamd_not_declared", 0)
    with pytest.raises(AttributeError, match="hipMalloc"):  # in the process, but not declared
        _lib.lib().hipMalloc
    newer = tmp_path / "piamd_kernels.h"
    with open(HEADER, encoding="utf-8") as f:
        newer.write_text(f.read() + "PIAMD_EXPORT int piamd_added_after_the_build(int rows, hipStream_t st);\n")
    with pytest.raises(ImportError, match="piamd_added_after_the_build") as e:
        _lib._load(str(newer))
    assert _lib.lib_path() in str(e.value) and "rebuild" in str(e.value)

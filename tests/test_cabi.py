"""CPU-only checks of the drop-in boundary: the C-ABI library builds, loads, exports every
symbol include/chicdiff_hip.h declares, and refuses (loudly) to run without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    return hip.load_library()


def test_exports_match_header(lib):
    from chicdiff_amd import hip
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(chicdiff_hip_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted(hip.EXPORTS)
    for sym in declared:
        assert hasattr(lib, sym), sym


def test_argtypes_match_header(lib):
    """Every prototype of include/chicdiff_hip.h against the ctypes declaration of hip.load_library(), position by position and by class:
    an integer or double of the header's width, or a pointer (anything with '*' and the two callback typedefs); a return type other
    than int needs its restype.  An entry point without argtypes would take every Python int as a 32-bit C int."""
    from chicdiff_amd import hip
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    scalars = {"int32_t": C.c_int32, "int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
    assert C.sizeof(C.c_int) == 4                                                   # (the header's plain int and ctypes' default restype)

    def kind(ctype):
        if ctype is None:
            return "void"
        for name, t in scalars.items():
            if ctype is t or (issubclass(ctype, C._SimpleCData) and ctype._type_ == t._type_):
                return "int" if name in ("int", "int32_t") else name
        assert ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, (C._Pointer, C._CFuncPtr, C.Array)), ctype
        return "pointer"

    def kind_of_text(text):
        words = text.replace("const", " ").split()
        if "*" in text or words[0] in ("chicdiff_allreduce_fn", "chicdiff_allgather_fn"):
            return "pointer"
        if words[0] == "void":
            return "void"
        return "int" if words[0] in ("int", "int32_t") else {k: k for k in scalars}[words[0]]

    protos = re.findall(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(chicdiff_hip_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", hdr)
    assert sorted(p[1] for p in protos) == sorted(hip.EXPORTS)
    bad = []
    for ret, name, params in protos:
        fn = getattr(lib, name)
        if fn.argtypes is None:
            bad.append(f"{name}: no argtypes")
            continue
        want = [kind_of_text(p) for p in params.split(",")]
        got = [kind(t) for t in fn.argtypes]
        if want != got:
            bad.append(f"{name}: header {want}, argtypes {got}")
        if kind_of_text(ret + " x") != kind(fn.restype):
            bad.append(f"{name}: header returns {ret.strip()!r}, restype {fn.restype}")
    assert not bad, "\n".join(bad)


def test_no_assert_statement_guards_the_package():
    """``python -O`` strips assert statements: nothing in chicdiff_amd/*.py may rest on one (refusals are ValueError)."""
    import ast
    import glob
    found = []
    for path in sorted(glob.glob(os.path.join(ROOT, "chicdiff_amd", "*.py"))):
        tree = ast.parse(open(path).read(), path)
        found += [f"{os.path.basename(path)}:{node.lineno}" for node in ast.walk(tree) if isinstance(node, ast.Assert)]
    assert not found, found


def test_header_lists_the_options_of_the_librarys_table():
    """The comment block above chicdiff_hip_set_option in include/chicdiff_hip.h is the only documentation a host has: it names
    every option of the library's table (kOptions, chicdiff_amd/csrc/ctx.hip), and no other, in the table's order."""
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    block = hdr[hdr.index("/* Tuning / test options"):hdr.index("int chicdiff_hip_set_option(")]
    documented = re.findall(r'^ \*   "([a-z_]+)"', block, re.M)
    api = open(os.path.join(ROOT, "chicdiff_amd", "csrc", "ctx.hip")).read()
    table = api[api.index("static const OptionDef kOptions[] = {"):]
    table = table[:table.index("\n};")]
    stored = re.findall(r'^    \{"([a-z_]+)",', table, re.M)
    assert stored and len(set(stored)) == len(stored)
    assert documented == stored


def test_struct_layouts_match_header(lib):
    from chicdiff_amd import hip
    o = hip.default_opts()
    assert (o.minDisp, o.dispTol, o.kappa0, o.maxit, o.betaMaxit, o.betaTol, o.minmu, o.outlierSD) == \
        (1e-8, 1e-6, 1.0, 100, 100, 1e-8, 0.5, 2.0)
    assert o.dispPriorVar != o.dispPriorVar and o.trendCoef[0] != o.trendCoef[0]  # NaN = estimate
    assert C.sizeof(hip.Opts) == 88 and o.fitType == 0 and C.sizeof(hip.Out) == 21 * 8 and C.sizeof(hip.Scalars) == 56
    # the compiler's view of the header (gcc, plain C): sizes and a few offsets against the ctypes mirrors
    import subprocess
    import tempfile
    src = r"""
#include <stddef.h>
#include <stdio.h>
#include "chicdiff_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(chicdiff_nbglm_opts), sizeof(chicdiff_nbglm_out), sizeof(chicdiff_nbglm_scalars),
           sizeof(chicdiff_results_info), offsetof(chicdiff_results_info, index), offsetof(chicdiff_results_info, theta),
           offsetof(chicdiff_nbglm_opts, trendCoef));
    return 0;
}
"""
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(td, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(hip.Opts), C.sizeof(hip.Out), C.sizeof(hip.Scalars), C.sizeof(hip.ResultsInfo), hip.ResultsInfo.index.offset,
                   hip.ResultsInfo.theta.offset, hip.Opts.trendCoef.offset]


def test_product_path_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from chicdiff_amd import hip
    with pytest.raises(hip.ChicdiffHipError):
        hip.HipContext(0)
    h = C.c_void_p()
    rc = lib.chicdiff_hip_create(C.byref(h), 0)
    assert rc != 0 and not h.value
    assert b"no CPU fallback" in lib.chicdiff_hip_last_error(None)


def test_product_package_never_imports_oracle():
    pat = re.compile(r"^\s*(from\s+oracle|import\s+oracle|#include\s+[\"<].*oracle)", re.M)
    for dirpath, _, files in os.walk(os.path.join(ROOT, "chicdiff_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                assert not pat.search(open(os.path.join(dirpath, f)).read()), f

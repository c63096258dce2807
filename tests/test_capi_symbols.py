"""CPU: the C-ABI library loads and exports exactly the symbols include/zedo_hip.h declares
(no compute calls without a GPU), and the product path refuses to run without a GPU."""
import ctypes
import os
import re

import pytest

from _shared import ROOT, host_lib  # (imports torch first: it must precede the dlopen of libzedo_hip.so, torch bundles its own HIP runtime)

HDR = os.path.join(ROOT, "include", "zedo_hip.h")


def declared_functions():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(zedo_[a-z_0-9]+)\s*\(", src)))


KINDS = ("int", "long long", "float", "double", "size_t", "pointer", "void")


def c_kind(decl):
    """A return type or one parameter declaration of the header -> its kind.  Anything with a * is a pointer; otherwise the type is
    what is left of the declaration without qualifiers and without the parameter's name."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w not in ("const", "extern")]
    for kind in ("long long", "int", "float", "double", "size_t", "void"):
        n = len(kind.split())
        if words[:n] == kind.split() and len(words) in (n, n + 1):      # the type alone, or the type and a name
            return kind
    raise AssertionError(f"include/zedo_hip.h: no kind for {decl!r}")


def declared_prototypes():
    """Every prototype of include/zedo_hip.h -> {name: (return kind, [argument kinds])}, comments and preprocessor lines stripped."""
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    protos = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(zedo_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src):
        assert name not in protos, name
        args = [a.strip() for a in args.split(",")]
        protos[name] = (c_kind(ret), [] if args == ["void"] else [c_kind(a) for a in args])
    return protos


def ctypes_kind(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    # c_size_t first: ctypes spells it as an alias of an unsigned integer type, which the header does not use under another name
    return {ctypes.c_size_t: "size_t", ctypes.c_int: "int", ctypes.c_longlong: "long long", ctypes.c_float: "float",
            ctypes.c_double: "double"}[t]


@pytest.fixture(scope="module")
def lib():
    return host_lib()


def test_header_declares_the_expected_surface():
    names = declared_functions()
    for n in ("zedo_weights_create", "zedo_schedule_create", "zedo_reproj_prepare", "zedo_reproj_grad",
              "zedo_score_eps", "zedo_sde_step", "zedo_oil_run", "zedo_ipo_fit", "zedo_rotate_init",
              "zedo_min_mpjpe", "zedo_workspace_bytes"):
        assert n in names


def test_library_exports_every_declared_symbol(lib):
    for n in declared_functions():
        assert hasattr(lib, n), f"{n} declared in include/zedo_hip.h but not exported"
    assert lib.zedo_abi_version() == 5
    lib.zedo_error_string.restype = ctypes.c_char_p
    assert b"workspace" in lib.zedo_error_string(-3)


def test_binding_matches_header(lib):
    import zedo_hip
    assert sorted(zedo_hip.SIGNATURES) == declared_functions()
    lib.zedo_workspace_bytes.restype = ctypes.c_size_t
    assert zedo_hip.workspace_bytes(1000) == 1024 * (64 + 2048) * 4
    assert zedo_hip.param_names() == [n for n, _ in __import__("lib.dataset.synthetic", fromlist=["x"]).state_dict_layout()]


def test_the_header_parser_reads_what_it_is_given():
    """The parser on the shapes the header uses: qualifiers, pointers to pointers, (void), a pointer return, long long."""
    assert c_kind("const float *d_x") == c_kind("const float *const *h_z") == c_kind("zedo_weights_t **out") == c_kind("void *stream") == "pointer"
    assert c_kind("const char *") == "pointer" and c_kind("void") == "void" and c_kind("size_t") == c_kind("size_t n_floats") == "size_t"
    assert c_kind("long long row_offset") == "long long" and c_kind("int B") == "int" and c_kind("double normaliser") == "double"
    assert c_kind("float ipo_T") == "float"
    with pytest.raises(AssertionError):
        c_kind("unsigned flags")
    protos = declared_prototypes()
    assert protos["zedo_abi_version"] == ("int", []) and protos["zedo_error_string"] == ("pointer", ["int"])
    assert protos["zedo_weights_destroy"] == ("void", ["pointer"]) and protos["zedo_workspace_bytes"] == ("size_t", ["int"])
    assert protos["zedo_profile_shader_ghz"] == ("double", [])


def test_binding_argument_types_match_the_header():
    """zedo_hip.SIGNATURES is written by hand; test_binding_matches_header compares its names only.  Here every prototype of the
    header as (return kind, [argument kinds]) over int, long long, float, double, size_t, pointer, void against the ctypes table -
    c_void_p, POINTER(...) and c_char_p all count as pointer.  A c_int where the header has `long long row_offset`, a c_float for
    `double normaliser` or a swapped pair would hand the library garbage in that argument and pass every other CPU test.  No GPU call."""
    import zedo_hip
    protos = declared_prototypes()
    assert sorted(protos) == declared_functions() == sorted(zedo_hip.SIGNATURES)
    assert {k for r, a in protos.values() for k in [r] + a} == set(KINDS)          # every kind occurs: the comparison is not one-sided
    for name, (res, args) in zedo_hip.SIGNATURES.items():
        got = (ctypes_kind(res), [ctypes_kind(a) for a in args])
        assert got == protos[name], (name, [(i, g, w) for i, (g, w) in enumerate(zip(got[1], protos[name][1])) if g != w], got[0],
                                     protos[name][0], len(got[1]), len(protos[name][1]))
    ipo, resume = protos["zedo_ipo_fit"][1], protos["zedo_ipo_fit_resume"][1]      # the two longest entries, spelled out once
    assert len(ipo) == 21 and len(resume) == 23 and ipo[10] == resume[10] == "double" and ipo[19] == resume[21] == "long long"
    assert ipo[6:9] == resume[6:9] == ["float"] * 3 and resume[15] == "pointer" and resume[16] == "int"


def test_no_cpu_fallback():
    import torch
    import zedo_hip
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(zedo_hip.ZedoError):
        zedo_hip.reproj_prepare(torch.zeros(2, 17, 2), torch.zeros(2, 3, 3))
    with pytest.raises(zedo_hip.ZedoError):
        zedo_hip.Weights({})

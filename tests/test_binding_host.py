"""The ctypes binding (maua_amd/_lib.py) against include/maua_hip.h, without a device: every declared function has a signature and the
right number of arguments, one hand-stated signature per kind of type, the parser's refusal of a type it does not know, calls through
the real library that only come out right when restype and argtypes are honoured, the nine struct mirrors field by field, and the rule
that nothing else under maua_amd/ declares a signature or wraps a scalar."""
import ctypes
import re
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flow_ref as FR  # noqa: E402

from maua_amd import _lib as L  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "maua_hip.h").read_text()
RAW = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)      # comments only: the independent view of the declarations
p, i, g, f, d, z, u, s = (ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_size_t,
                          ctypes.c_ulonglong, ctypes.c_char_p)
MIRRORS = {"maua_gemm_desc": L.GemmDesc, "maua_conv_desc": L.ConvDesc, "maua_modconv_desc": L.ModconvDesc, "maua_attn_desc": L.AttnDesc,
           "maua_attn_vjp_desc": L.AttnVjpDesc, "maua_gn_desc": L.GnDesc, "maua_gn_vjp_desc": L.GnVjpDesc,
           "maua_farneback_desc": L.FbDesc, "maua_nca_desc": L.NcaDesc}


@pytest.fixture(scope="module")
def table():
    return L.parse_header(HEADER)


@pytest.fixture(scope="module")
def lib():
    from maua_amd.build import build
    build()
    return L.lib()


def test_every_declared_function_has_a_signature(table):
    names = sorted(set(re.findall(r"\b(maua_[a-z0-9_]+)\s*\(", RAW)))      # what declared_symbols() was before it read the table
    assert sorted(table) == names == L.declared_symbols()
    stated = re.search(r"\*\*(\d+) entry points\*\*", (ROOT / "DESIGN.md").read_text())
    assert stated and int(stated.group(1)) == len(table), (stated and stated.group(1), len(table))
    for name, (_, argtypes) in table.items():
        params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, RAW).group(1)
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name


def test_one_signature_per_kind_of_type(table):
    assert table["maua_resample_linear"] == (i, [p, p, i, g, i, p])
    assert table["maua_synth_load"] == (i, [p, s, p, z])
    assert table["maua_tensor2bytes"] == (i, [p, p, p, i, i, i, i, d, d])
    assert table["maua_correlation_workspace"] == (g, [i, i, i])
    assert table["maua_last_error"] == (s, []) and table["maua_version"] == (s, [])
    assert table["maua_vgg_destroy"] == (None, [p])
    assert table["maua_ctx_create"] == (i, [i, p, p])
    assert table["maua_philox_normal"] == (i, [p, u, u, u, p, g, f, f])
    assert table["maua_philox_clip_audio"] == (i, [p, u, g, d, p])
    assert table["maua_nca_step"] == (i, [p, p])
    assert table["maua_synth_forward"] == (i, [p, p, p, p, i, p])        # const float* const*, const long*
    assert table["maua_onset_from_mel"][1][7] is i                       # a comment between the parameter and its comma


def test_an_unknown_scalar_type_is_refused():
    with pytest.raises(L.MauaHipError) as e:
        L.parse_header("/* c */\n#define X 1\nenum { A = 0 };\ntypedef struct { int a; } t;\nint maua_ok(int a);\nint maua_x(short a);\n")
    assert "maua_x" in str(e.value) and "short" in str(e.value)
    with pytest.raises(L.MauaHipError) as e:
        L.parse_header("short maua_y(void);")
    assert "maua_y" in str(e.value) and "short" in str(e.value)
    with pytest.raises(L.MauaHipError, match="maua_z"):
        L.parse_header("int maua_ok(int a);\nint maua_z(int (*f)(int));")     # not a plain declaration: an error, not a guess
    with pytest.raises(L.MauaHipError, match="maua_ok is not declared"):
        L.signature("/* int maua_ok(int a); */ int maua_other(void);", "maua_ok")
    assert L.parse_header("void maua_v(const char* s, const char** t, unsigned  long long n);") == {"maua_v": (None, [s, p, u])}


def test_calls_through_the_library(lib):
    assert lib.maua_farneback_levels(40, 48) == FR.pyramid_levels(40, 48) + 1 == 2
    h, w = ctypes.c_int(), ctypes.c_int()
    assert lib.maua_farneback_level_size(40, 48, 1, ctypes.byref(h), ctypes.byref(w)) == 0
    assert (h.value, w.value) == FR.level_size(40, 48, 1) == (32, 38)
    # video_features.hip corr_ws_bytes: six float64 arrays, each rounded up to 256 bytes - mean, cs, col [F], rn [2 T], G, Gn [F][F] -
    # with F = Fx + Fy = 2 and T = 2^28: 3 x 256 + 2^32 + 2 x 256.  Cut to an int it would be 1280.
    assert lib.maua_correlation_workspace(1 << 28, 1, 1) == (1 << 32) + 1280
    assert lib.maua_version().decode()
    assert lib.maua_magnitude(None, None, 0, 1.0, None) == -1 and lib.maua_last_error() == b"maua_magnitude: NULL argument"
    with pytest.raises(ctypes.ArgumentError):
        lib.maua_resample_linear(None, None, 1, ctypes.c_int(1), 1, None)            # an int where the header says long
    with pytest.raises(ctypes.ArgumentError):
        lib.maua_magnitude(None, None, 0, ctypes.c_double(1.0), None)                # a double where the header says float
    with pytest.raises(ctypes.ArgumentError):
        lib.maua_farneback_levels(40.0, 48)
    with pytest.raises(L.MauaHipError, match="maua_not_there"):
        lib.maua_not_there
    assert isinstance(L.lib(), ctypes.CDLL) and L.lib() is lib


def struct_fields(name):
    """[(field, ctypes type)] of a `typedef struct { ... } name;` of the header, one entry per declarator"""
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, RAW).group(1)
    fields = []
    for decl in filter(None, (x.strip() for x in body.split(";"))):
        first, *rest = decl.split(",")
        ctype, field = re.fullmatch(r"(.*?)(\w+)", first.strip()).groups()
        fields.append((field, L.ctype_of(ctype, name)))
        base = ctype.rstrip("* \t\n")                           # `const float *w1, *b1`: the stars belong to each declarator
        for more in rest:
            stars, field = re.fullmatch(r"([*\s]*)(\w+)", more.strip()).groups()
            fields.append((field, L.ctype_of(base + stars, name)))
    return fields


def test_struct_parser_on_multi_declarators():
    assert struct_fields("maua_nca_desc")[:7] == [("x", p), ("B", i), ("H", i), ("W", i), ("w1", p), ("b1", p), ("w2", p)]
    assert struct_fields("maua_nca_desc")[11:14] == [("seed", u), ("stream", u), ("step0", u)]


@pytest.mark.parametrize("name", sorted(MIRRORS))
def test_struct_mirror_follows_the_header(name):
    assert list(MIRRORS[name]._fields_) == struct_fields(name)


def test_every_by_value_struct_has_a_mirror():
    structs = re.findall(r"typedef\s+struct\s*\{[^}]*\}\s*(\w+)\s*;", RAW)
    assert sorted(structs) == sorted(list(MIRRORS) + ["maua_comm_id"])      # maua_comm_id: 128 opaque bytes, passed as a char array
    from maua_amd import nca
    assert nca.NcaDesc is L.NcaDesc


def test_one_binding_style_only():
    pkg = ROOT / "maua_amd"
    files = sorted(set(pkg.glob("*.py")) | set(pkg.glob("**/*.py")))
    assert len(files) > 40
    for path in files:
        text = path.read_text()
        if path != pkg / "_lib.py":
            assert not re.search(r"\.(argtypes|restype)\s*=", text), path
        wraps = re.findall(r"\b(?:C|ctypes)\.c_(?:int|float|long|double|size_t|ulonglong)\(\s*[^)\s][^\n]*", text)
        assert not wraps, (path, wraps)

"""The kernel library's C ABI has one declaration, csrc/pda_api.h: these tests hold the ctypes
bindings (ops/ext.py, read from that header) and the built library to it. CPU only: the library is
the one cross-compiled for gfx950, loaded but never launched."""
import ctypes as C
import shutil
import subprocess

import pytest

from pytorch_distributed_amd.ops import ext

V = C.c_void_p


@pytest.fixture(scope="module")
def api():
    return ext.read_api(ext.api_text())


@pytest.fixture()
def fresh_load(monkeypatch):
    """ext.load() binds again inside the test and the session's binding comes back afterwards."""
    monkeypatch.setattr(ext, "_LIB", None)
    monkeypatch.delenv("PDA_KERNEL_LIB", raising=False)
    return monkeypatch


# ------------------------------------------------------------------ the reader, on literal strings
def test_reader_maps_every_allowed_type():
    text = """
    // int pda_in_a_comment(int x);
    extern "C" {
    /* int pda_in_a_block_comment(int x); */
    unsigned long long pda_all(int a, unsigned b, float c, double d, long long e, unsigned long long f,
                               hipStream_t st, hipEvent_t ev, const int* pa, unsigned* pb,
                               const float* pc, double* pd, const long long* pe,
                               unsigned long long* pf, hipStream_t* ps, hipEvent_t* pev,
                               const void* v, void* w, const ConvDesc* d0, const BwdArgsC* d1,
                               const BnEpi* d2, const BnFwdOut* d3, const BnBwdOut* d4,
                               const RedDescC* d5, const SegRow* d6, const BlkRow* d7,
                               EmaRange* d8);
    int pda_none();
    float pda_f(float *x);
    }
    """
    api = ext.read_api(text)
    assert sorted(api) == ["pda_all", "pda_f", "pda_none"]
    restype, args = api["pda_all"]
    assert restype is C.c_ulonglong
    assert args == [C.c_int, C.c_uint, C.c_float, C.c_double, C.c_longlong, C.c_ulonglong, V, V,
                    V, V, V, V, V, V, V, V, V, V,
                    C.POINTER(ext.ConvDesc), C.POINTER(ext.BwdArgs), C.POINTER(ext.BnEpi),
                    C.POINTER(ext.BnFwdOut), C.POINTER(ext.BnBwdOut), C.POINTER(ext.RedDescC),
                    C.POINTER(ext.SegRow), C.POINTER(ext.BlkRow), C.POINTER(ext.EmaRange)]
    assert api["pda_none"] == (C.c_int, [])
    assert api["pda_f"] == (C.c_float, [V])


@pytest.mark.parametrize("proto", [
    "int pda_x(short a);", "int pda_x(char* s);", "int pda_x(size_t n);", "int pda_x(void v);",
    "int pda_x(float** pp);", "int pda_x(ConvDesc d);", "int pda_x(const Unknown* u);",
    "int pda_x(int);", "int pda_x(long n);", "void pda_x(int a);", "hipStream_t pda_x(int a);"])
def test_reader_refuses_other_types(proto):
    with pytest.raises(ValueError):
        ext.read_api(proto)


# ------------------------------------------------------------------ header vs library
def test_header_and_library_export_the_same_names(api):
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm (binutils) is not installed")
    ext.load(required=True)     # builds the library when it is not there yet
    out = subprocess.run([nm, "-D", "--defined-only", str(ext.LIBPATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("pda_")}
    assert exported - set(api) == set(), "exported but not declared in pda_api.h"
    assert set(api) - exported == set(), "declared in pda_api.h but not exported"


# ------------------------------------------------------------------ struct layouts
def test_struct_layouts_match_the_header():
    layouts = ext.read_layouts(ext.api_text())
    assert sorted(layouts) == sorted(ext.STRUCTS) and len(layouts) == 9
    for cname, (size, last, off) in layouts.items():
        cls = ext.STRUCTS[cname]
        assert cls._fields_[-1][0] == last, cname
        assert (C.sizeof(cls), getattr(cls, last).offset) == (size, off), cname


# ------------------------------------------------------------------ what load() bound
def test_every_declared_function_is_bound(api):
    L = ext.load(required=True)
    assert sorted(vars(L)) == sorted(api) and len(api) >= 60
    for name, (restype, args) in api.items():
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(args) and list(fn.argtypes) == args, name
        assert fn.restype is restype, name
    assert L.pda_track_count.restype is C.c_ulonglong
    assert ext.has("pda_conv_fwd") and not ext.has("pda_no_such_launcher")
    with pytest.raises(AttributeError):     # an undeclared name never reaches C
        L.pda_no_such_launcher


def test_a_declared_symbol_the_library_lacks(fresh_load):
    """Raises at load; only an A/B variant library (PDA_KERNEL_LIB) may hold a subset."""
    text = ext.api_text()
    at = text.rindex('}  // extern "C"')
    fresh_load.setattr(ext, "api_text", lambda: text[:at] + "int pda_not_in_the_library(int a);\n" + text[at:])
    assert "pda_not_in_the_library" in ext.read_api(ext.api_text())
    with pytest.raises(RuntimeError, match="pda_not_in_the_library"):
        ext.load()
    fresh_load.setenv("PDA_KERNEL_LIB", ext.LIBPATH.name)
    L = ext.load(required=True)
    assert not hasattr(L, "pda_not_in_the_library") and hasattr(L, "pda_conv_fwd")

"""CPU-only checks that the binding derives the C ABI from the headers that
state it (turbopfor_amd.prototypes / declare over include/turbopfor_gpu.h and
include/turbopfor_capi.h): every declared tpf_* function gets a prototype and
nothing else does, declare() gives every exported one its argtypes, five
prototypes are pinned as literals, and a declaration the parse cannot read or
type is refused, never passed over."""
import ctypes
import os
import subprocess

import pytest

import turbopfor_amd as tpf
from test_capi_cpu import declared_c_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
vp, u64, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t
i32, u = ctypes.c_int, ctypes.c_uint

PINS = {
    "tpf_enc_batch": (i32, [i32, vp, u64, u, i32, vp, u64, vp, u64, vp, vp, sz, vp]),
    "tpf_p4ndec256v32_lists_units": (i32, [vp, u64, vp, u64, vp, vp, u64, i32, vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, sz, vp, vp]),
    "tpf_lists_append": (i32, [vp, u64, vp, u64, vp, vp, u64, i32, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, vp, vp, vp, sz, vp, vp]),
    "tpf_lists_remove_workspace_size": (sz, [u64] * 5),
    "tpf_last_error": (ctypes.c_char_p, []),
}


def test_every_declared_function_has_a_prototype_and_nothing_else():
    assert set(tpf.prototypes()) == declared_c_symbols()


def test_declare_gives_every_exported_function_its_argtypes():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    raw = ctypes.CDLL(LIB)
    L = tpf.declare(raw)
    assert L is raw
    exported = 0
    for name, (restype, argtypes) in tpf.prototypes().items():
        if not hasattr(L, name):
            continue
        exported += 1
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == len(argtypes), name
        assert list(f.argtypes) == argtypes and f.restype is restype, name
    assert exported == len(tpf.prototypes())  # the in-tree build exports all of them (test_capi_cpu holds that too)


def test_declare_skips_what_a_library_lacks():
    libc = tpf.declare(ctypes.CDLL(None))  # exports no tpf_* symbol: an older build lacks some in the same way
    assert not hasattr(libc, "tpf_lists_remove")


@pytest.mark.parametrize("name", sorted(PINS))
def test_pinned_prototypes(name):
    assert tpf.prototypes()[name] == PINS[name]


def test_the_measurement_header_goes_through_the_same_parse():
    P = tpf.prototypes([os.path.join(tpf.PKG_DIR, "measure", "tpf_measure.h")])
    assert len(P) == 8 and all(name.startswith("tpfm_") for name in P)
    assert P["tpfm_enc256v32_workspace_size"] == (sz, [i32, u64])
    assert P["tpfm_probe_hbm"] == (i32, [i32, vp, vp, u64, vp])


def _header(tmp_path, text):
    p = tmp_path / "bad.h"
    p.write_text("#include <stdint.h>\n/* a header */\nint tpf_fine(const uint8_t *d_in, uint64_t n, void *stream);\n" + text)
    return str(p)


def test_a_readable_header_parses(tmp_path):
    p = _header(tmp_path, "void tpf_quiet(void); // nothing\nconst char *tpf_text(unsigned n);\nunsigned char *tpf_ptr(int64_t x);\n")
    assert tpf.prototypes([p]) == {"tpf_fine": (i32, [vp, u64, vp]), "tpf_quiet": (None, []), "tpf_text": (ctypes.c_char_p, [u]),
                                   "tpf_ptr": (vp, [ctypes.c_int64])}


@pytest.mark.parametrize("decl", [
    "int tpf_bad(double x);",                          # a parameter type outside the table
    "int tpf_bad(unsigned long n);",                   # a two-word type is not `unsigned` with a name
    "float tpf_bad(int x);",                           # a return type outside the table
    "int tpf_bad(uint64_t n, void (*cb)(int));",       # a function pointer: not one flat parameter list
    "int tpf_bad(int x)\nint tpf_worse(int y);",       # two declarations run together
    "int tpf_bad(int x, uint64_t",                     # cut off
    "int tpf_bad();",                                  # no parameter list to read
    "static inline int tpf_bad(int x) { return x; }",  # a definition
])
def test_an_unreadable_declaration_is_refused(tmp_path, decl):
    with pytest.raises(tpf.TpfError) as e:
        tpf.prototypes([_header(tmp_path, decl + "\n")])
    assert "bad.h" in str(e.value) and "tpf_bad" in str(e.value)


def test_a_missing_header_is_refused(tmp_path):
    with pytest.raises(tpf.TpfError) as e:
        tpf.prototypes([str(tmp_path / "absent.h")])
    assert "absent.h" in str(e.value)

"""CPU checks of tpf_lists_extract (include/turbopfor_gpu.h): the numpy
definition the GPU tests compare against (tests/lists_extract_ref.py) -- a
byte slice with rebased offsets -- equals the oracle's encoding of the sliced
values with the starts it yields, for every unit range of the matrix; the
matrix tells the two likely mistakes from the definition; and the entry point's
host side: its argument checks before any device call, its workspace export,
its symbol and its prototype."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lists_extract_ref as xr
import lists_ref as ref
import ref_lib
import turbopfor_amd as tpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
EINVAL = -1
MODES = [(True, True), (True, False), (False, False)]  # (d1, with d_start0)
MODE_IDS = ["d1-start0", "d1-null", "plain"]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for d1, st in MODES:
        src = xr.matrix_source(d1, st)
        sel = xr.matrix_selection(src)
        out[d1, st] = (src, sel, xr.extract(src, *sel))
    return out


def same_stream(a, packed, offs, ptr):
    return np.array_equal(a.packed, packed) and np.array_equal(a.offs, offs) and np.array_equal(a.ptr, ptr)


@pytest.mark.parametrize("d1,st", MODES, ids=MODE_IDS)
def test_definition_is_the_oracles_encoding_of_the_sliced_values(cases, d1, st):
    """Every (ufirst, ucount) of lists of 0, 1, 255, 256, 257 and 513 values, a
    sample for 256 * 17 + 3 and every range of a list that wraps 2^32: bytes,
    offsets and pointers are lists_ref.compose of the sliced lists with
    start0_out, and the sliced lists have the lengths the header states."""
    src, (sel, uf, uc), r = cases[d1, st]
    for n in xr.LENS:
        j = [len(v) for v in src.lists].index(n)
        got = {(a, c) for k, a, c in zip(sel, uf, uc) if k == j}
        assert got == set(xr.ranges(n)), n
    packed, offs, ptr, _ = ref.compose(r.lists, d1, r.start0)
    assert same_stream(r, packed, offs, ptr)
    assert np.array_equal(r.base, np.asarray(ref.units_loop(r.ptr)[1], dtype=np.uint32))
    for k, (j, a, c) in enumerate(zip(sel, uf, uc)):
        n = len(src.lists[j])
        tail = c != 0 and a + c == ref.n_units(n) and n % 256 != 0
        assert len(r.lists[k]) == (256 * (c - 1) + n % 256 if tail else 256 * c), (j, a, c)
    kinds = ref.block_kinds(src.packed, src.offs, src.ptr)
    assert kinds["vbyte"] and (kinds["bitmap"] or not d1), kinds


@pytest.mark.skipif(not ref_lib.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("d1,st", MODES, ids=MODE_IDS)
def test_definition_against_the_reference(cases, d1, st):
    """The same, held against the reference's own encoder: every list of the
    result is what a reference caller writes for the sliced values."""
    _, _, r = cases[d1, st]
    for k, v in enumerate(r.lists):
        want = ref_lib.encn256v32_stream(v, d1=d1, start0=int(r.start0[k]) if d1 else 0)
        got = r.packed[int(r.offs[r.base[k]]): int(r.offs[r.base[k + 1]])]
        assert bytes(got) == want, k


@pytest.mark.parametrize("st", [True, False], ids=["start0", "null"])
def test_table_is_unit_last_of_the_result(cases, st):
    _, _, r = cases[True, st]
    assert np.array_equal(r.table, xr.table(r.lists))
    assert len(r.table) == r.nunits


@pytest.mark.parametrize("d1,st", MODES, ids=MODE_IDS)
def test_matrix_tells_the_mutants_apart(cases, d1, st):
    """A start taken from d_start0[j] at ufirst > 0 changes what the result
    decodes to (the oracle's encoding with those starts is no longer the
    definition's bytes), and an offset that is not rebased changes the
    offsets: the matrix sees both."""
    src, sel, r = cases[d1, st]
    m = xr.extract(src, *sel, rebase=False)
    assert not np.array_equal(m.offs, r.offs)
    if d1:
        m = xr.extract(src, *sel, start_mutant=True)
        assert not np.array_equal(m.start0, r.start0)
        packed, offs, ptr, _ = ref.compose(r.lists, True, m.start0)
        assert not same_stream(r, packed, offs, ptr)


# ---- the entry point's host side ------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    return tpf.declare(ctypes.CDLL(LIB))


ARGS = ["d_in", "in_bytes", "d_off", "nunits", "d_list_ptr", "d_list_unit", "nlists", "d1", "d_start0", "d_unit_last", "d_sel",
        "d_ufirst", "d_ucount", "nsel", "d_out", "out_cap", "d_off_out", "units_cap", "d_list_ptr_out", "d_list_unit_out",
        "d_start0_out", "d_unit_last_out", "d_ws", "ws_bytes", "d_err", "stream"]
COUNTS = {"in_bytes": 64, "nunits": 4, "nlists": 2, "d1": 1, "nsel": 2, "out_cap": 64, "units_cap": 4}
BIG = 0x80000000
# one change to a call whose every pointer is set: (name, {argument: value}); None is a null pointer
REFUSED = [
    ("null-d_off_out", {"d_off_out": None}),
    ("null-d_list_ptr_out", {"d_list_ptr_out": None}),
    ("null-d_list_unit_out", {"d_list_unit_out": None}),
    ("null-outputs-at-nsel-0", {"d_off_out": None, "nsel": 0}),
    ("null-d_sel", {"d_sel": None}),
    ("null-d_list_ptr", {"d_list_ptr": None}),
    ("null-d_list_unit", {"d_list_unit": None}),
    ("null-d_ws", {"d_ws": None}),
    ("null-d_out-with-out_cap", {"d_out": None}),
    ("null-d_in-with-nunits", {"d_in": None}),
    ("null-d_off-with-nunits", {"d_off": None}),
    ("null-d_ucount-with-d_ufirst", {"d_ucount": None}),
    ("null-d_start0_out-with-d1", {"d_start0_out": None}),
    ("null-d_unit_last-with-d1-and-d_ufirst", {"d_unit_last": None}),
    ("ws_bytes-one-short", {"ws_bytes": -1}),
    ("nunits-over", {"nunits": BIG}),
    ("nlists-over", {"nlists": BIG}),
    ("nsel-over", {"nsel": BIG}),
    ("units_cap-over", {"units_cap": BIG}),
]


@pytest.mark.parametrize("name,change", REFUSED, ids=[r[0] for r in REFUSED])
def test_extract_checks_arguments_before_the_device(lib, name, change):
    """Every TPF_EINVAL condition of the header, one per case, from a call
    whose other arguments are in order: refused on the host before any device
    is touched -- the same answer with or without a GPU (the pointers are
    host memory and never followed)."""
    lib.tpf_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_uint64 * 64)()
    a = {k: ctypes.addressof(buf) for k in ARGS if k.startswith("d_")}
    a.update(COUNTS, stream=None)
    a.update({k: v for k, v in change.items() if k != "ws_bytes"})
    a["ws_bytes"] = lib.tpf_lists_extract_workspace_size(a["nsel"]) + change.get("ws_bytes", 0)
    assert lib.tpf_lists_extract(*[a[k] for k in ARGS]) == EINVAL, lib.tpf_last_error()
    assert b"tpf_lists_extract" in lib.tpf_last_error()


def test_workspace_export_is_a_multiple_of_256_and_non_decreasing(lib):
    sizes = [lib.tpf_lists_extract_workspace_size(n) for n in
             list(range(0, 300)) + [4095, 4096, 4097, 64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1, 1 << 20, (1 << 20) + 1, 0x7FFFFFFF]]
    assert sizes[0] == 0 and all(s % 256 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    # O(nsel): a few dozen bytes per selection
    assert sizes[-1] <= 64 * 0x7FFFFFFF


def test_symbol_is_exported_and_its_prototype_parses():
    protos = tpf.prototypes()
    restype, argtypes = protos["tpf_lists_extract"]
    assert restype is ctypes.c_int and len(argtypes) == len(ARGS)
    ints = {"in_bytes", "nunits", "nlists", "nsel", "out_cap", "units_cap"}
    for name, ty in zip(ARGS, argtypes):
        want = ctypes.c_uint64 if name in ints else ctypes.c_int if name == "d1" else ctypes.c_size_t if name == "ws_bytes" else ctypes.c_void_p
        assert ty is want, name
    assert protos["tpf_lists_extract_workspace_size"] == (ctypes.c_size_t, [ctypes.c_uint64])
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"tpf_lists_extract", "tpf_lists_extract_workspace_size"} <= exported


def test_term_shard_names_a_ranks_lists():
    import tpf_shard

    got = [tpf_shard.term_shard(11, 4, r).tolist() for r in range(4)]
    assert got == [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7]]
    assert tpf_shard.term_shard(2, 4, 3).numel() == 0 and tpf_shard.term_shard(5, 1, 0).dtype.is_floating_point is False

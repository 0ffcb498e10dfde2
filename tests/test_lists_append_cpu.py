"""CPU-only checks of the host surface of the append to a resident index
(include/turbopfor_gpu.h tpf_lists_append): the symbols are exported, the
arguments are judged before any device call (TPF_EINVAL, with the cause in the
message), the two bound functions never decrease, and they cover the oracle's
composition of every (old, added) pair of the GPU matrix
(tests/test_gpu_lists_append.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import lists_ref as ref
import turbopfor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
EINVAL, ENODEV = -1, -3
P = 0x1000  # a non-null pointer that is never followed: every call below is refused on the host
STEPS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 10 ** 6, 0x3FFFFFFF]
OLD = [0, 1, 255, 256, 257, 511, 512, 513, 256 * 17 + 3]
ADD = [0, 1, 255, 256, 257, 600]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    return turbopfor_amd.declare(ctypes.CDLL(LIB))


def _no_device():
    return subprocess.run([sys.executable, "-c", "import torch,sys;sys.exit(0 if torch.cuda.is_available() else 1)"]).returncode != 0


def test_symbols_exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"tpf_lists_append", "tpf_lists_append_bound", "tpf_lists_append_units_bound", "tpf_lists_append_workspace_size"} <= exported
    with open(os.path.join(ROOT, "turbopfor-cpp_amd", "python", "turbopfor_amd.py")) as f:
        src = f.read()
    assert "def lists_append(" in src and "def lists_append_bound(" in src and "def lists_append_units_bound(" in src


def _call(lib, d_in=P, d_off=P, nunits=10, ptr=P, lu=P, nlists=5, d1=1, st=None, ul=P, add=P, add_values=100, aptr=P, nout=7, out=P,
          out_cap=1000, off_out=P, units_cap=20, lptr_out=P, lunit_out=P, ul_out=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.tpf_lists_append_workspace_size(min(nunits, 1 << 20), min(nout, 1 << 20), min(add_values, 1 << 20))
    return lib.tpf_lists_append(d_in, 100, d_off, nunits, ptr, lu, nlists, d1, st, ul, add, add_values, aptr, nout, out, out_cap, off_out,
                                units_cap, lptr_out, lunit_out, ul_out, ws, ws_bytes, None, None)


def _msg(lib, *words):
    m = lib.tpf_last_error()
    assert b"tpf_lists_append" in m
    for w in words:
        assert w in m, (w, m)


def test_fewer_lists_than_the_old_index_is_einval(lib):
    assert _call(lib, nlists=8, nout=7) == EINVAL
    _msg(lib, b"nlists_out", b"below nlists")


@pytest.mark.parametrize("d1", [0, 1])
@pytest.mark.parametrize("arg", ["d_in", "d_off", "ptr", "lu", "aptr", "out", "off_out", "lptr_out", "lunit_out", "ws", "add"])
def test_null_pointer_is_einval(lib, arg, d1):
    assert _call(lib, d1=d1, **{arg: None}) == EINVAL
    _msg(lib, b"null")


def test_null_tables_are_refused_only_with_d1(lib):
    for kw in (dict(ul=None), dict(ul_out=None)):
        assert _call(lib, d1=1, **kw) == EINVAL
        _msg(lib, b"d_unit_last")
        # the plain form ignores both tables: the call gets past them to the workspace check
        assert _call(lib, d1=0, ws_bytes=0, **kw) == EINVAL
        _msg(lib, b"workspace")
    # d_start0 is optional with d1 too
    assert _call(lib, d1=1, st=None, ws_bytes=0) == EINVAL
    _msg(lib, b"workspace")


def test_null_old_index_and_additions_are_allowed_when_empty(lib):
    # an empty old index needs none of its pointers, not even the table; no additions need no d_add
    for kw in (dict(nlists=0), dict(nunits=0)):
        assert _call(lib, d_in=None, d_off=None, ptr=None, lu=None, ul=None, ws_bytes=0, **kw) == EINVAL
        _msg(lib, b"workspace")
    assert _call(lib, add=None, add_values=0, ws_bytes=0) == EINVAL
    _msg(lib, b"workspace")


def test_small_workspace_is_einval(lib):
    need = lib.tpf_lists_append_workspace_size(10, 7, 100)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == EINVAL
    _msg(lib, b"workspace")


@pytest.mark.parametrize("kw", [dict(nunits=0x80000000), dict(nout=0x80000000), dict(units_cap=0x80000000), dict(add_values=0x80000000)])
def test_limits_are_einval(lib, kw):
    assert _call(lib, ws_bytes=2 ** 62, **kw) == EINVAL
    _msg(lib, b"0x7FFFFFFF")


def test_no_cpu_fallback_without_device(lib):
    if not _no_device():
        pytest.skip("a HIP device is visible")
    for call in (lambda: _call(lib), lambda: _call(lib, d1=0, ul=None, ul_out=None),
                 lambda: _call(lib, nlists=0, nout=0, aptr=None, add=None, add_values=0, ws=None, ws_bytes=0)):
        assert call() == ENODEV
        assert b"no CPU fallback" in lib.tpf_last_error()


def test_bounds_and_workspace_never_decrease(lib):
    for f in (lib.tpf_lists_append_units_bound, lib.tpf_lists_append_bound, lib.tpf_lists_append_workspace_size):
        for x, y in ((0, 0), (1, 1), (1000, 10), (10, 1000), (10 ** 6, 10 ** 6)):
            for a, b in zip(STEPS, STEPS[1:]):
                assert f(a, x, y) <= f(b, x, y), (f, 0, a, b, x, y)
                assert f(x, a, y) <= f(x, b, y), (f, 1, a, b, x, y)
                assert f(x, y, a) <= f(x, y, b), (f, 2, a, b, x, y)
    assert lib.tpf_lists_append_units_bound(7, 5, 0) == 7 and lib.tpf_lists_append_bound(123, 5, 0) >= 123
    assert lib.tpf_lists_append_units_bound(7, 5, 1000) == 7 + 3 + 5
    assert lib.tpf_lists_append_workspace_size(10, 0, 100) == 0  # nlists_out == 0 is a no-op


def test_bounds_cover_the_matrix(lib):
    """Every (old, added) pair alone, and all of them as one index: the bounds are at least the byte length and the
    unit count of the oracle's composition of the concatenated lists."""
    rng = np.random.default_rng(3)
    for d1 in (True, False):
        olds, fulls = [], []
        for o in OLD:
            for a in ADD:
                v = ref.d1_values(o + a, 0, rng, outliers=True) if d1 else ref.plain_values(o + a, rng)
                po, oo, _, _ = ref.compose([v[:o]], d1)
                px, ox, _, _ = ref.compose([v], d1)
                assert lib.tpf_lists_append_bound(len(po), 1, a) >= len(px), (o, a)
                assert lib.tpf_lists_append_units_bound(len(oo) - 1, 1, a) >= len(ox) - 1, (o, a)
                olds.append(v[:o]), fulls.append(v)
        po, oo, _, _ = ref.compose(olds, d1)
        px, ox, _, _ = ref.compose(fulls, d1)
        nadd = sum(len(f) - len(o) for f, o in zip(fulls, olds))
        assert lib.tpf_lists_append_bound(len(po), len(olds), nadd) >= len(px)
        assert lib.tpf_lists_append_units_bound(len(oo) - 1, len(olds), nadd) >= len(ox) - 1

"""CPU-only checks of the host surface of the block-range reads of a resident
index (include/turbopfor_gpu.h tpf_lists_unit_last, tpf_lists_range_units,
tpf_p4ndec256v32_lists_units): the symbols are exported, the workspace-size
functions are pure host functions, the arguments are judged before any device
call (TPF_EINVAL), and the entry points report TPF_ENODEV instead of falling
back to a CPU codec."""
import ctypes
import os
import subprocess
import sys

import pytest

import turbopfor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
EINVAL, ENODEV = -1, -3
P = 0x1000  # a non-null pointer that is never followed: every call below is refused on the host


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
    assert {"tpf_lists_unit_last", "tpf_lists_unit_last_workspace_size", "tpf_lists_range_units", "tpf_p4ndec256v32_lists_units",
            "tpf_p4ndec256v32_lists_units_workspace_size"} <= exported
    # the range search is one kernel over its arguments: it needs no workspace, so it has no size companion
    assert "tpf_lists_range_units_workspace_size" not in exported
    with open(os.path.join(ROOT, "turbopfor-cpp_amd", "python", "turbopfor_amd.py")) as f:
        src = f.read()
    for name in ("def lists_unit_last(", "def lists_range_units(", "def decn256v32_lists_units("):
        assert name in src


STEPS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 10 ** 6, 0x3FFFFFFF]


@pytest.mark.parametrize("which", ["unit_last", "units"])
def test_workspace_size_is_a_pure_host_function(lib, which):
    f = lib.tpf_lists_unit_last_workspace_size if which == "unit_last" else lib.tpf_p4ndec256v32_lists_units_workspace_size
    for fixed in (0, 1, 1000, 10 ** 6):
        for a, b in zip(STEPS, STEPS[1:]):
            assert 0 < f(a, fixed) <= f(b, fixed), ("first", a, b, fixed)
            assert 0 < f(fixed, a) <= f(fixed, b), ("second", a, b, fixed)
    assert f(1000, 10 ** 6) == f(1000, 10 ** 6)  # no state


def test_unit_last_workspace_is_linear_in_units_and_lists(lib):
    """O(nunits + nlists): a few words per unit and per list, nothing sized by the values."""
    f = lib.tpf_lists_unit_last_workspace_size
    assert f(10 ** 6, 10 ** 6) < 64 * 2 * 10 ** 6 + (1 << 16)
    assert f(10 ** 6, 10) < f(10 ** 7, 10) and f(10, 10 ** 6) < f(10, 10 ** 7)


def test_units_workspace_grows_with_the_unit_cap(lib):
    f = lib.tpf_p4ndec256v32_lists_units_workspace_size
    # sized by the unit cap out_values / 256 + nsel: 256 more values are one more unit
    assert f(10, 256 * 1000) < f(10, 256 * 100000)
    assert f(10, 256 * 100000) - f(10, 256 * 1000) >= 4 * 99000


# ---- tpf_p4ndec256v32_lists_units ------------------------------------------------
def _units(lib, d_in=P, d_off=P, nunits=10, ptr=P, lu=P, nlists=5, d1=0, ul=P, sel=P, uf=P, uc=P, nsel=3, out=P, out_values=1000,
           out_ptr=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.tpf_p4ndec256v32_lists_units_workspace_size(min(nsel, 1 << 20), min(out_values, 1 << 30))
    return lib.tpf_p4ndec256v32_lists_units(d_in, 100, d_off, nunits, ptr, lu, nlists, d1, None, ul, sel, uf, uc, nsel, out, out_values,
                                            out_ptr, ws, ws_bytes, None, None)


@pytest.mark.parametrize("arg", ["d_in", "d_off", "ptr", "lu", "sel", "uf", "uc", "out", "out_ptr", "ws"])
@pytest.mark.parametrize("d1", [0, 1])
def test_units_null_pointer_is_einval(lib, arg, d1):
    assert _units(lib, d1=d1, **{arg: None}) == EINVAL
    assert b"tpf_p4ndec256v32_lists_units" in lib.tpf_last_error() and b"null" in lib.tpf_last_error()


def test_units_d1_needs_the_table(lib):
    assert _units(lib, d1=1, ul=None) == EINVAL
    assert b"d_unit_last" in lib.tpf_last_error() and b"null" in lib.tpf_last_error()
    # plain ignores it: the call gets past the argument checks (no device here, or a refusal later -- never this one)
    assert _units(lib, d1=0, ul=None, ws_bytes=0) == EINVAL and b"workspace" in lib.tpf_last_error()


def test_units_small_workspace_is_einval(lib):
    need = lib.tpf_p4ndec256v32_lists_units_workspace_size(3, 1000)
    assert _units(lib, ws_bytes=need - 1) == EINVAL
    assert b"workspace" in lib.tpf_last_error()


@pytest.mark.parametrize("kw", [dict(nlists=0x80000000), dict(nunits=0x80000000), dict(nsel=0x80000000),
                                dict(nsel=2, out_values=256 * 0x7FFFFFFE), dict(nsel=1, out_values=2 ** 64 - 1)])
def test_units_limits_are_einval(lib, kw):
    assert _units(lib, ws_bytes=2 ** 62, **kw) == EINVAL
    assert b"0x7FFFFFFF" in lib.tpf_last_error()


# ---- tpf_lists_unit_last ------------------------------------------------------------
def _unit_last(lib, d_in=P, d_off=P, nunits=10, ptr=P, nlists=5, out=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.tpf_lists_unit_last_workspace_size(min(nunits, 1 << 20), min(nlists, 1 << 20))
    return lib.tpf_lists_unit_last(d_in, 100, d_off, nunits, ptr, nlists, None, out, ws, ws_bytes, None, None)


@pytest.mark.parametrize("arg", ["d_in", "d_off", "ptr", "out", "ws"])
def test_unit_last_null_pointer_is_einval(lib, arg):
    assert _unit_last(lib, **{arg: None}) == EINVAL
    assert b"tpf_lists_unit_last" in lib.tpf_last_error() and b"null" in lib.tpf_last_error()


def test_unit_last_small_workspace_and_limits(lib):
    need = lib.tpf_lists_unit_last_workspace_size(10, 5)
    assert _unit_last(lib, ws_bytes=need - 1) == EINVAL and b"workspace" in lib.tpf_last_error()
    for kw in (dict(nunits=0x80000000), dict(nlists=0x80000000)):
        assert _unit_last(lib, ws_bytes=2 ** 62, **kw) == EINVAL and b"0x7FFFFFFF" in lib.tpf_last_error()


# ---- tpf_lists_range_units ------------------------------------------------------------
def _range(lib, lu=P, ul=P, nlists=5, nunits=10, ql=P, lo=P, hi=P, nq=3, uf=P, uc=P):
    return lib.tpf_lists_range_units(lu, ul, nlists, nunits, ql, lo, hi, nq, uf, uc, None, None)


@pytest.mark.parametrize("arg", ["lu", "ul", "ql", "lo", "hi", "uf", "uc"])
def test_range_null_pointer_is_einval(lib, arg):
    assert _range(lib, **{arg: None}) == EINVAL
    assert b"tpf_lists_range_units" in lib.tpf_last_error() and b"null" in lib.tpf_last_error()


@pytest.mark.parametrize("kw", [dict(nlists=0x80000000), dict(nunits=0x80000000), dict(nq=0x80000000)])
def test_range_limits_are_einval(lib, kw):
    assert _range(lib, **kw) == EINVAL
    assert b"0x7FFFFFFF" in lib.tpf_last_error()


def test_no_cpu_fallback_without_device(lib):
    if not _no_device():
        pytest.skip("a HIP device is visible")
    for call in (lambda: _units(lib), lambda: _units(lib, d1=1),
                 lambda: _units(lib, nsel=0, sel=None, uf=None, uc=None, out=None, ws=None, ws_bytes=0),
                 lambda: _unit_last(lib), lambda: _range(lib), lambda: _range(lib, nq=0, ql=None)):
        assert call() == ENODEV
        assert b"no CPU fallback" in lib.tpf_last_error()

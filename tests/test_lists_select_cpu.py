"""CPU-only checks of the host surface of the read side of a resident index
(include/turbopfor_gpu.h tpf_lists_unit_base, tpf_p4ndec256v32_lists_select):
the symbols are exported, the workspace-size functions are pure host
functions, the arguments are judged before any device call (TPF_EINVAL), and
the entry points report TPF_ENODEV instead of falling back to a CPU codec."""
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
    assert {"tpf_lists_unit_base", "tpf_lists_unit_base_workspace_size", "tpf_p4ndec256v32_lists_select",
            "tpf_p4ndec256v32_lists_select_workspace_size"} <= exported


STEPS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 10 ** 6, 0x3FFFFFFF]


def test_unit_base_workspace_size_is_a_pure_host_function(lib):
    f = lib.tpf_lists_unit_base_workspace_size
    for a, b in zip(STEPS, STEPS[1:]):
        assert 0 < f(a) <= f(b), (a, b)
    assert f(1000) == f(1000)  # no state


def test_select_workspace_size_is_a_pure_host_function(lib):
    f = lib.tpf_p4ndec256v32_lists_select_workspace_size
    for fixed in (0, 1, 1000, 10 ** 6):
        for a, b in zip(STEPS, STEPS[1:]):
            assert 0 < f(a, fixed) <= f(b, fixed), ("nsel", a, b, fixed)
            assert 0 < f(fixed, a) <= f(fixed, b), ("out_values", a, b, fixed)
    # sized by the unit cap out_values / 256 + nsel: 256 more values are one more unit
    assert f(10, 256 * 1000) < f(10, 256 * 100000)
    assert f(1000, 10 ** 6) == f(1000, 10 ** 6)  # no state


def _select(lib, d_in=P, d_off=P, nunits=10, ptr=P, lu=P, nlists=5, sel=P, nsel=3, out=P, out_values=1000, out_ptr=P, ws=P,
            ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.tpf_p4ndec256v32_lists_select_workspace_size(min(nsel, 1 << 20), min(out_values, 1 << 30))
    return lib.tpf_p4ndec256v32_lists_select(d_in, 100, d_off, nunits, ptr, lu, nlists, 0, None, sel, nsel, out, out_values, out_ptr, ws,
                                             ws_bytes, None, None)


@pytest.mark.parametrize("arg", ["d_in", "d_off", "ptr", "lu", "sel", "out", "out_ptr", "ws"])
def test_select_null_pointer_is_einval(lib, arg):
    assert _select(lib, **{arg: None}) == EINVAL
    assert b"tpf_p4ndec256v32_lists_select" in lib.tpf_last_error() and b"null" in lib.tpf_last_error()


def test_select_small_workspace_is_einval(lib):
    need = lib.tpf_p4ndec256v32_lists_select_workspace_size(3, 1000)
    assert _select(lib, ws_bytes=need - 1) == EINVAL
    assert b"workspace" in lib.tpf_last_error()


@pytest.mark.parametrize("kw", [dict(nlists=0x80000000), dict(nunits=0x80000000), dict(nsel=0x80000000),
                                dict(nsel=2, out_values=256 * 0x7FFFFFFE), dict(nsel=1, out_values=2 ** 64 - 1)])
def test_select_limits_are_einval(lib, kw):
    assert _select(lib, ws_bytes=2 ** 62, **kw) == EINVAL
    assert b"0x7FFFFFFF" in lib.tpf_last_error()


def test_unit_base_einval(lib):
    f = lib.tpf_lists_unit_base
    need = lib.tpf_lists_unit_base_workspace_size(7)
    assert f(P, 7, None, P, need, None, None) == EINVAL and b"null" in lib.tpf_last_error()
    assert f(None, 7, P, P, need, None, None) == EINVAL and b"null" in lib.tpf_last_error()
    assert f(P, 7, P, None, need, None, None) == EINVAL and b"null" in lib.tpf_last_error()
    assert f(P, 7, P, P, need - 1, None, None) == EINVAL and b"workspace" in lib.tpf_last_error()
    assert f(P, 0x80000000, P, P, 2 ** 62, None, None) == EINVAL and b"0x7FFFFFFF" in lib.tpf_last_error()
    assert f(None, 0, None, None, 0, None, None) == EINVAL  # even nlists == 0 writes d_list_unit[0]


def test_no_cpu_fallback_without_device(lib):
    if not _no_device():
        pytest.skip("a HIP device is visible")
    assert _select(lib) == ENODEV
    assert b"no CPU fallback" in lib.tpf_last_error()
    assert _select(lib, nsel=0, sel=None, out=None, ws=None, ws_bytes=0) == ENODEV
    need = lib.tpf_lists_unit_base_workspace_size(7)
    assert lib.tpf_lists_unit_base(P, 7, P, P, need, None, None) == ENODEV
    assert b"no CPU fallback" in lib.tpf_last_error()

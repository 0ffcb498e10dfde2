"""CPU-only checks of the host surface of the positional read of a resident
index (include/turbopfor_gpu.h tpf_lists_gather): the symbols are exported,
the workspace-size function is a pure host function, the arguments are judged
before any device call (TPF_EINVAL), and the entry point reports TPF_ENODEV
instead of falling back to a CPU codec."""
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
STEPS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 10 ** 6, 0x3FFFFFFF]


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
    assert {"tpf_lists_gather", "tpf_lists_gather_workspace_size"} <= exported
    with open(os.path.join(ROOT, "turbopfor-cpp_amd", "python", "turbopfor_amd.py")) as f:
        assert "def lists_gather(" in f.read()


def test_workspace_size_is_a_pure_host_function(lib):
    f = lib.tpf_lists_gather_workspace_size
    for fixed in (0, 1, 1000, 10 ** 6):
        for a, b in zip(STEPS, STEPS[1:]):
            assert 0 < f(a, fixed) <= f(b, fixed), ("nq", a, b, fixed)
            assert 0 < f(fixed, a) <= f(fixed, b), ("pos_values", a, b, fixed)
    assert f(1000, 10 ** 6) == f(1000, 10 ** 6)  # no state


def test_workspace_is_linear_in_the_positions(lib):
    """A few words per position: nothing sized by the index (the function does not even see it), and at most 32 bytes per position
    (four words of plan and items, the run scan's 8 bytes per 64 positions, the alignment of each array)."""
    f = lib.tpf_lists_gather_workspace_size
    assert f(10 ** 6, 10 ** 6) < 32 * 10 ** 6 + 65536
    assert f(10, 10 ** 6) < f(10, 10 ** 7) < 11 * f(10, 10 ** 6)
    assert f(10, 10 ** 6) >= 16 * 10 ** 6  # the four words are there
    assert f(1, 10 ** 6) == f(10 ** 6, 10 ** 6)  # the queries are read where they lie


def _call(lib, d_in=P, d_off=P, nunits=10, ptr=P, lu=P, nlists=5, d1=1, st=None, ul=P, pos=P, pos_values=100, pos_ptr=P, qlist=P, nq=3,
          out=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.tpf_lists_gather_workspace_size(min(nq, 1 << 20), min(pos_values, 1 << 20))
    return lib.tpf_lists_gather(d_in, 100, d_off, nunits, ptr, lu, nlists, d1, st, ul, pos, pos_values, pos_ptr, qlist, nq, out, ws,
                                ws_bytes, None, None)


@pytest.mark.parametrize("d1", [0, 1])
@pytest.mark.parametrize("arg", ["d_in", "d_off", "ptr", "lu", "pos_ptr", "qlist", "ws", "pos", "out"])
def test_null_pointer_is_einval(lib, arg, d1):
    assert _call(lib, d1=d1, **{arg: None}) == EINVAL
    assert b"tpf_lists_gather" in lib.tpf_last_error() and b"null" in lib.tpf_last_error()


def test_null_unit_last_is_refused_only_with_d1(lib):
    assert _call(lib, d1=1, ul=None) == EINVAL
    assert b"tpf_lists_gather" in lib.tpf_last_error() and b"d_unit_last" in lib.tpf_last_error()
    # the plain form ignores the table and the starts: the call gets past them to the workspace check
    assert _call(lib, d1=0, ul=None, st=None, ws_bytes=0) == EINVAL
    assert b"workspace" in lib.tpf_last_error()
    # ... and d_start0 is optional with d1 too
    assert _call(lib, d1=1, st=None, ws_bytes=0) == EINVAL
    assert b"workspace" in lib.tpf_last_error()


def test_null_pos_and_out_are_allowed_when_empty(lib):
    # with nothing to read or write the two pointers may be null: the call gets past them to the workspace check
    assert _call(lib, pos=None, pos_values=0, out=None, ws_bytes=0) == EINVAL
    assert b"workspace" in lib.tpf_last_error()


def test_small_workspace_is_einval(lib):
    need = lib.tpf_lists_gather_workspace_size(3, 100)
    assert _call(lib, ws_bytes=need - 1) == EINVAL
    assert b"tpf_lists_gather" in lib.tpf_last_error() and b"workspace" in lib.tpf_last_error()


@pytest.mark.parametrize("kw", [dict(nlists=0x80000000), dict(nunits=0x80000000), dict(nq=0x80000000), dict(pos_values=0x80000000)])
def test_limits_are_einval(lib, kw):
    assert _call(lib, ws_bytes=2 ** 62, **kw) == EINVAL
    assert b"tpf_lists_gather" in lib.tpf_last_error() and b"0x7FFFFFFF" in lib.tpf_last_error()


def test_no_cpu_fallback_without_device(lib):
    if not _no_device():
        pytest.skip("a HIP device is visible")
    for call in (lambda: _call(lib), lambda: _call(lib, d1=0, ul=None),
                 lambda: _call(lib, nq=0, qlist=None, pos_ptr=None, pos=None, pos_values=0, out=None, ws=None, ws_bytes=0)):
        assert call() == ENODEV
        assert b"no CPU fallback" in lib.tpf_last_error()

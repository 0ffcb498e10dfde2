"""CPU-only checks of the many-lists decode's host surface
(include/turbopfor_gpu.h tpf_p4ndec256v32_lists): the symbols are exported,
the workspace-size function is a pure host function, the entry point reports
TPF_ENODEV instead of falling back to a CPU codec, and the binding's
lists_units (numpy only, no library) agrees with a plain loop."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import lists_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    return ctypes.CDLL(LIB)


def test_symbols_exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"tpf_p4ndec256v32_lists", "tpf_p4ndec256v32_lists_workspace_size"} <= exported


def test_workspace_size_is_a_pure_host_function(lib):
    f = lib.tpf_p4ndec256v32_lists_workspace_size
    f.restype = ctypes.c_size_t
    f.argtypes = [u64, u64]
    steps = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 4095, 4096, 4097, 10 ** 6, 0x7FFFFFFF]
    for a in steps:
        assert f(a, 1) > 0 and f(1, a) > 0
    for fixed in (1, 1000, 10 ** 6):
        for a, b in zip(steps, steps[1:]):
            assert f(a, fixed) <= f(b, fixed), ("nunits", a, b, fixed)
            assert f(fixed, a) <= f(fixed, b), ("nlists", a, b, fixed)
    assert f(1000, 10) == f(1000, 10)  # no state


def test_no_cpu_fallback_without_device(lib):
    if subprocess.run([sys.executable, "-c", "import torch,sys;sys.exit(0 if torch.cuda.is_available() else 1)"]).returncode == 0:
        pytest.skip("a HIP device is visible")
    lib.tpf_p4ndec256v32_lists.restype = ctypes.c_int
    lib.tpf_last_error.restype = ctypes.c_char_p
    rc = lib.tpf_p4ndec256v32_lists(None, u64(0), None, u64(1), None, u64(1), 0, None, None, u64(0), None,
                                    ctypes.c_size_t(0), None, None)
    assert rc == -3  # TPF_ENODEV
    assert b"no CPU fallback" in lib.tpf_last_error()


def test_lists_units_matches_a_plain_loop():
    import turbopfor_amd as tpf

    lens = [0, 1, 255, 256, 257, 512, 0, 0, 511, 513, 256 * 64 + 1, 0]
    ptr = np.concatenate([[7], 7 + np.cumsum(lens)]).astype(np.int64)
    want_units, want_base = lists_ref.units_loop(ptr)
    units, base = tpf.lists_units(ptr)
    assert units.tolist() == want_units and base.tolist() == want_base
    assert base[-1] == sum(want_units) and len(base) == len(ptr)
    torch = pytest.importorskip("torch")
    units_t, base_t = tpf.lists_units(torch.from_numpy(ptr))
    assert units_t.tolist() == want_units and base_t.tolist() == want_base
    units_u, _ = tpf.lists_units(ptr.astype(np.uint64))
    assert units_u.tolist() == want_units
    with pytest.raises(ValueError):
        tpf.lists_units(np.array([0, 5, 3]))
